#!/usr/bin/env python3
"""The Gaussian-mixture background model (mog2, fm_mog2.hip) against the gray chain in the same run: one stream,
1080p frames resident in device memory, 64-frame batches, fm_max_inflight batches kept in flight:

    1080p   -B 1920 -b 384   k = 5, the frame is the work image (k_wide_blur in front of the scan)
    modeD   -B 100           k = 5, INTER_AREA to 100 x 56 (the reference CLI's default; k_small_blur in front)

Three alternating rounds, mog2 then gray; the gray path is code the option does not touch, so it is the yardstick of
the run.  Per (shape, mode, round) one JSON line: frames/s through submit and wait, the engine's pixel path and, for
mog2, the per-launch device time of the blur and of `mog2_scan` (FM_FLAG_PROFILE_PIX: in-kernel stamps) with the
fraction of 8 TB/s the scan reaches on the byte model of DESIGN.md §3.11: per pixel-frame 1 blur byte, 1/8 byte of
bits and 2 (1 + 12 n) / T bytes of state, n the clip's mean modes in use (read back with fm_mog2_read_model and
printed).  A last line per shape holds the medians and the mog2 / gray ratio.

Usage: tools/bench_mog2.py [--batch T] [--seconds S] [--rounds R] [--shapes 1080p,modeD] [--log FILE]
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

SHAPES = {"1080p": (1920, 1080, 1920, 384), "modeD": (1920, 1080, 100, 20)}  # W, H, -B, -b
HBM_PEAK = 8e12  # B/s
MOG2_KERNELS = ("small_blur", "wide_blur", "mog2_scan")


def run(torch, fm, ring, W, H, box, k, T, seconds, mog2):
    eng = fm.MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=box, ksize=k, threshold=12, avg=0.1, max_batch=T,
                          profile="pix", **({"mog2": True} if mog2 else {}))
    depth = eng.max_inflight
    t0 = time.perf_counter()
    for i in range(depth):  # every slot once (and the stream's first frame)
        eng.submit_device(ring[i % 2].data_ptr(), T)
    for i in range(depth):
        eng.wait()
    warm = (time.perf_counter() - t0) / depth
    n = max(2 * depth, min(2000, int(seconds / max(warm, 1e-6))))
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
    times = {kn: v for kn, v in eng.kernel_times().items() if kn in MOG2_KERNELS and v[1] > 0}
    h, w = eng.work_shape
    nbar = float(eng.mog2_model(0)["nmodes"].mean()) if mog2 else None
    out = {"mode": "mog2" if mog2 else "gray", "pixel_path": eng.pixel_path, "work": [w, h], "ksize": k, "batch": T,
           "batches": n, "max_inflight": depth, "frames_per_s": round(n * T / dt, 1),
           "contours_per_frame": round(contours / (n * T), 2),
           "device_GB": round(eng.footprint()["device_bytes"] / 1e9, 3)}
    eng.close()
    if mog2 and "mog2_scan" in times:
        out["launch_ms"] = {kn: round(ms / cnt, 4) for kn, (ms, cnt) in times.items()}
        out["mean_modes_in_use"] = round(nbar, 3)
        moved = h * w * (T * (1 + 1 / 8) + 2 * (1 + 12 * nbar))  # the scan alone
        scan = times["mog2_scan"][0] / times["mog2_scan"][1] / 1e3
        out["scan_model_bytes_per_launch"] = int(moved)
        out["scan_fraction_of_8TBps"] = round(moved / scan / HBM_PEAK, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=2.0, help="timed seconds per run (at least 2 x max_inflight batches)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch  # torch's HIP runtime first, as bench.py

    import find_motion_amd as fm
    from find_motion_amd.synthetic import SyntheticVideo

    fm.use_hw_queues()
    lines = [{"bench": "mog2_env", "host": platform.node(), "device": torch.cuda.get_device_name(0),
              "batch": a.batch, "rounds": a.rounds}]
    print(json.dumps(lines[0]), flush=True)
    for name in a.shapes.split(","):
        W, H, box, bscale = SHAPES[name]
        k = fm.make_gaussian(box, bscale)
        vid = SyntheticVideo(W, H, 0)
        distinct = torch.from_numpy(np.stack([vid.frame(40 + 12 * i) for i in range(4)])).cuda()
        T = a.batch
        # a ring of two resident batches [T][1][H][W][3], each cycling over the distinct frames from another start
        ring = [distinct[(torch.arange(T, device="cuda") + r) % 4].unsqueeze(1).contiguous() for r in range(2)]
        got = {"mog2": [], "gray": []}
        for rnd in range(a.rounds):
            for mog2 in (True, False):
                r = run(torch, fm, ring, W, H, box, k, T, a.seconds, mog2)
                r.update(bench="mog2", shape=name, round=rnd)
                got[r["mode"]].append(r)
                lines.append(r)
                print(json.dumps(r), flush=True)
        med = {m: statistics.median(x["frames_per_s"] for x in rs) for m, rs in got.items()}
        s = {"bench": "mog2_median", "shape": name, "frames_per_s": med,
             "mog2_over_gray": round(med["mog2"] / med["gray"], 3)}
        for kn in MOG2_KERNELS:
            v = [x["launch_ms"][kn] for x in got["mog2"] if kn in x.get("launch_ms", {})]
            if v:
                s[kn + "_ms"] = statistics.median(v)
        for key in ("scan_fraction_of_8TBps", "mean_modes_in_use"):
            v = [x[key] for x in got["mog2"] if key in x]
            if v:
                s[key] = statistics.median(v)
        lines.append(s)
        print(json.dumps(s), flush=True)
        del ring, distinct
    if a.log:
        with open(a.log, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
