"""fm_host.h (the device objects' buffers, holders and fail function) under AddressSanitizer and UBSan.

tests/host/fm_host_selftest.cpp is a stand-alone host program: it defines the few HIP entry points the
header uses on top of malloc, fails each allocation in turn, and checks that buffers are empty after a
failure and that nothing stays allocated.  Built here with ROCm's clang++; no GPU, no libamdhip64.
"""
import os
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
ROCM = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
CLANG = ROCM / "lib" / "llvm" / "bin" / "clang++"


@pytest.mark.skipif(not CLANG.exists(), reason="ROCm's clang++ not found")
def test_fm_host_selftest(tmp_path):
    exe = tmp_path / "fm_host_selftest"
    build = subprocess.run(
        [str(CLANG), "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM / 'include'}", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-g", "-Wall", "-o", str(exe), str(ROOT / "tests/host/fm_host_selftest.cpp")],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "12 failing positions, 0 errors" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
