"""bench.py as it is run for every change: a plain `--gpus 1 --steps K --warmup W` line, and `--dump-outputs DIR`
(the last timed step's results as .npy files) against the oracle on the same seeded frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, S, T, STEPS, WARMUP = 320, 240, 2, 8, 2, 1


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs_equal_the_oracle(oracle_lib, tmp_path):
    from find_motion_amd import make_gaussian
    from find_motion_amd.synthetic import batch
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--width", str(W),
           "--height", str(H), "--streams", str(S), "--batch", str(T), "--ring", str(T), "--ring-period", str(T),
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    # ms_per_step is the time of one timed step (the line rounds it to 0.1 us)
    assert line["value"] == pytest.approx(S * T / (line["ms_per_step"] / 1e3), rel=1e-2)
    assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("frames/s", True, "u8+f64")
    # a plain run carries none of the figures that take runs of their own (--full)
    assert line["full"] is False and "copy_peak_measured" not in line["roofline"]
    assert [line[k] for k in ("cpu_baseline", "side_configs", "host_fed_per_gpu", "mjpeg_fed_per_gpu")] == [None] * 4

    # the ring is one batch of T frames per stream, submitted WARMUP + STEPS times: the background keeps evolving
    k = make_gaussian(W, W // 5)
    cfg = oracle_lib.OracleConfig(H=H, W=W, box=W, ksize=k)
    orc = [oracle_lib.OracleStream(cfg) for _ in range(S)]
    frames = batch(W, H, S, 0, T)
    for _ in range(WARMUP + STEPS):
        last = [[orc[s].step(frames[t, s]) for s in range(S)] for t in range(T)]
    got = {n: np.load(tmp_path / f"{n}.npy") for n in line["dumped_outputs"]["arrays"]}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["counts"], [[last[t][s]["count"] for s in range(S)] for t in range(T)])
    assert np.array_equal(got["background"], np.stack([o.bg for o in orc]))
    rows = [(t, s, *b, *o) for t in range(T) for s in range(S)
            for b, o in zip(last[t][s]["boxes"], last[t][s]["origins"])]
    assert got["contours"].tolist() == [list(map(float, r)) for r in rows] and rows
    for i, (t, s) in enumerate(got["mask_frames"].astype(int)):
        assert np.array_equal(got["masks"][i], last[t][s]["mask"]), (t, s)
