#!/usr/bin/env python3
"""Gaussian sizes above 49 (the reference's default blur scale -b 20 with a raised box), one stream, frames
resident in device memory, fm_max_inflight batches kept in flight:

    1080p  -B 1920 -b 20   k = 97
    2160p  -B 3840 -b 20   k = 193
    1080p  k = 51          (the first size past k_fused)

Per shape one JSON line: frames/s through submit and wait, the engine's pixel path, the per-launch device time of
the pixel kernels (FM_FLAG_PROFILE_PIX: `wide_blur` and `wide_scan` by in-kernel stamps; the per-frame path's
`pixel` by events on sampled launches), and for the scan the bytes per second it moves -- 1 B of blur and 1/8 B
of threshold bits per pixel-frame plus 16 B per pixel per launch (the f64 background in and out) -- beside a
device-to-device copy measured in the same run (bench.py's copy_peak_measured).

The tool uses only calls that predate the wide path, so a checkout of an earlier commit (built) can be measured
with the same script: --tree DIR imports find_motion_amd from DIR.

Usage: tools/bench_wide_blur.py [--tree DIR] [--batch T] [--seconds S] [--shapes 1080p97,2160p193,1080p51]
                                [--label NAME] [--log FILE]      (the lines are appended to FILE as well)
"""
import argparse
import json
import os
import platform
import sys
import time

SHAPES = {"1080p97": (1920, 1080, 97), "2160p193": (3840, 2160, 193), "1080p51": (1920, 1080, 51)}
PIXEL_KERNELS = ("wide_blur", "wide_scan", "wide_blur_init", "wide_scan_init", "pixel")


def copy_peak_gbs(torch):
    """GB/s (read + write) of ten 256 MiB device-to-device copies, timed by HIP events (as bench.py)."""
    a = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 10 * 2 * a.numel() / (e0.elapsed_time(e1) / 1e3) / 1e9


def run_shape(torch, fm, name, T, seconds):
    from find_motion_amd.synthetic import SyntheticVideo

    W, H, k = SHAPES[name]
    assert fm.make_gaussian(W, 20) == k or name == "1080p51"
    vid = SyntheticVideo(W, H, 0)
    distinct = torch.from_numpy(__import__("numpy").stack([vid.frame(40 + 12 * i) for i in range(4)])).cuda()
    # a ring of two resident batches [T][1][H][W][3], each cycling over the distinct frames from another start
    ring = [distinct[(torch.arange(T, device="cuda") + r) % 4].unsqueeze(1).contiguous() for r in range(2)]
    eng = fm.MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=W, ksize=k, threshold=12, avg=0.1, max_batch=T,
                          profile="pix")
    depth = eng.max_inflight
    t0 = time.perf_counter()
    for i in range(depth):  # every slot once (and the stream's first frame)
        eng.submit_device(ring[i % 2].data_ptr(), T)
    for i in range(depth):
        eng.wait()
    warm = (time.perf_counter() - t0) / depth
    n = max(2 * depth, min(400, int(seconds / max(warm, 1e-6))))
    if warm > seconds:
        n = depth
    eng.reset_kernel_times()
    contours = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sub = done = 0
    while done < n:
        while sub < n and sub - done < depth:
            eng.submit_device(ring[sub % 2].data_ptr(), T)
            sub += 1
        eng.wait()
        contours += int(eng.counts().sum())
        done += 1
    dt = time.perf_counter() - t0
    times = {kn: v for kn, v in eng.kernel_times().items() if kn in PIXEL_KERNELS and v[1] > 0}
    foot = eng.footprint()
    path = getattr(eng, "pixel_path", "pixel")
    eng.close()
    out = {"bench": "wide_blur", "shape": name, "W": W, "H": H, "ksize": k, "batch": T, "batches": n,
           "pixel_path": path, "max_inflight": depth, "frames_per_s": round(n * T / dt, 1),
           "ms_per_batch": round(dt / n * 1e3, 3), "contours_per_frame": round(contours / (n * T), 2),
           "launch_ms": {kn: round(ms / cnt, 4) for kn, (ms, cnt) in times.items()},
           "launches_timed": {kn: int(cnt) for kn, (ms, cnt) in times.items()},
           "footprint_GB": {kk: round(v / 1e9, 3) for kk, v in foot.items()} if isinstance(foot, dict) else None}
    if "wide_scan" in times:
        ms, cnt = times["wide_scan"]
        moved = W * H * (T * (1 + 1 / 8) + 16)
        out["scan_bytes_per_launch"] = int(moved)
        out["scan_GBps"] = round(moved / (ms / cnt) / 1e6, 1)
    if "wide_blur" in times:
        ms, cnt = times["wide_blur"]
        out["blur_frames_per_s"] = round(T / (ms / cnt) * 1e3)
    del ring, distinct
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=5.0, help="timed seconds per shape (at least max_inflight batches)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--label", default="")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch  # torch's HIP runtime first, as bench.py

    import find_motion_amd as fm

    fm.use_hw_queues()
    lines = [{"bench": "wide_blur_env", "label": a.label, "host": platform.node(), "device": torch.cuda.get_device_name(0),
              "tree": os.path.abspath(a.tree), "copy_peak_measured_GBps": round(copy_peak_gbs(torch), 1)}]
    print(json.dumps(lines[0]), flush=True)
    for name in a.shapes.split(","):
        r = run_shape(torch, fm, name, a.batch, a.seconds)
        r["label"] = a.label
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.log:
        with open(a.log, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
