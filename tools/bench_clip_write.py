#!/usr/bin/env python3
"""Write side of the drop-in, end to end: VideoMotion over an all-motion synthetic 1080p source (every frame is
written), codec MJPG with gpu_encode=True, batch 64, the default pre-motion cache (2 s at 30 fps = 60 frames), with
and without resident_cache.  Two sources: host-fed BGR (an in-memory array) and an NV12 AVI (converted on the GPU).

Legs (--mode off|on|both): `off` is gpu_encode alone and uses nothing resident_cache added, so this script also runs
from a checkout that does not have the option (there a writer's encode_calls is its frame count: one call per
frame); `on` adds resident_cache=True.  Per source and leg: frames/s of find_motion() (the engine and the source are
set up before the clock starts; the clock stops after cleanup(), when the file is closed) and the writers' encoder
calls, as medians of --rounds rounds after one warm-up round, the legs alternating within a round.  One JSON line
on stdout; the log (every round) goes to --log.
Usage: tools/bench_clip_write.py [--mode both] [--frames 256] [--rounds 3] [--log profiles/clip_write_bench.log]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (torch's HIP runtime first, as bench.py)

from find_motion_amd import motion, videoio  # noqa: E402
from find_motion_amd.synthetic import SyntheticVideo  # noqa: E402

W, H, BATCH = 1920, 1080, 64


def nv12_of(f):
    g = f.astype(np.int32)
    y = ((g[..., 2] * 77 + g[..., 1] * 150 + g[..., 0] * 29) >> 8).astype(np.uint8)
    return np.concatenate([y.ravel(), np.stack([f[::2, ::2, 0], f[::2, ::2, 2]], -1).ravel()])


def one_run(source, frames, nv12_path, outdir, resident):
    writers = []
    real = videoio.open_writer
    videoio.open_writer = lambda *a, **k: writers.append(real(*a, **k)) or writers[-1]
    try:
        cap = videoio.ArrayCapture(frames) if source == "bgr" else videoio.RawAviCapture(nv12_path)
        vm = motion.VideoMotion(filename=os.path.join(outdir, "clip"), capture=cap, outdir=outdir, batch=BATCH,
                                codec="MJPG", gpu_encode=True, **({"resident_cache": True} if resident else {}))
        t0 = time.perf_counter()
        vm.find_motion()  # ends in cleanup(): the writer released, every encode collected
        dt = time.perf_counter() - t0
    finally:
        videoio.open_writer = real
    written = len(vm.written_indices)
    calls = sum(getattr(w, "encode_calls", w.device_frames + w.host_frames + w.fallback_frames) for w in writers)
    return dict(fps=len(frames) / dt, seconds=dt, written=written, encode_calls=calls,
                device_frames=sum(w.device_frames for w in writers), host_frames=sum(w.host_frames for w in writers))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["off", "on", "both"], default="both")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sources", default="bgr,nv12")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "clip_write_bench.log"))
    a = ap.parse_args()
    legs = ["off", "on"] if a.mode == "both" else [a.mode]
    vid = SyntheticVideo(W, H, 0)
    frames = np.stack([vid.frame(i) for i in range(a.frames)])
    tmp = tempfile.mkdtemp(prefix="clip_write_")
    lines = []

    def say(s):
        lines.append(s)
        print(s, file=sys.stderr, flush=True)

    out = {"frames": a.frames, "width": W, "height": H, "batch": BATCH, "rounds": a.rounds, "mode": a.mode}
    try:
        nv12_path = os.path.join(tmp, "src_nv12.avi")
        sources = a.sources.split(",")
        if "nv12" in sources:
            yw = videoio.RawAviWriter(nv12_path, 30, (W, H), fourcc="NV12")
            for f in frames:
                yw.write(nv12_of(f))
            yw.release()
        say(f"# {time.strftime('%Y-%m-%d %H:%M:%S')} bench_clip_write: {a.frames} frames {W}x{H}, batch {BATCH}, "
            f"cache 60, MJPG gpu_encode, legs {legs}, {a.rounds} rounds after a warm-up round")
        for source in sources:
            res = {leg: [] for leg in legs}
            for rnd in range(a.rounds + 1):  # round 0: warm-up
                for leg in (legs if rnd % 2 == 0 else legs[::-1]):
                    r = one_run(source, frames, nv12_path, tmp, leg == "on")
                    say(f"{source} round {rnd}{' (warm-up)' if rnd == 0 else ''} {leg}: {r['fps']:.1f} frames/s "
                        f"({r['seconds']:.3f} s), written {r['written']}, encode_calls {r['encode_calls']}, "
                        f"device_frames {r['device_frames']}, host_frames {r['host_frames']}")
                    if rnd:
                        res[leg].append(r)
            out[source] = {leg: dict(fps=round(float(np.median([r["fps"] for r in v])), 1),
                                     fps_min=round(min(r["fps"] for r in v), 1),
                                     fps_max=round(max(r["fps"] for r in v), 1),
                                     encode_calls=int(np.median([r["encode_calls"] for r in v])),
                                     written=v[0]["written"], host_frames=v[0]["host_frames"])
                           for leg, v in res.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
