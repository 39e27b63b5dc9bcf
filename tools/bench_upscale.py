#!/usr/bin/env python3
"""A box wider than the frame (MotionEngine(area_upscale=True)): one stream of 1280 x 720 frames enlarged to
1920 x 1080 (-B 1920 -b 384, k = 5), batches resident in device memory, fm_max_inflight batches kept in flight,
beside the same run's native 1080p mode F (1920 x 1080 frames, the same box and k: no resize).

Three JSON lines: the environment, the enlarged stream and the native one.  The enlarged stream's line has
  launch_ms.resize_area_up   the per-launch device time of k_resize_area_up (FM_FLAG_PROFILE_PIX: in-kernel stamps)
  copy_ms                    a device-to-device copy that reads plus writes as many bytes as one launch does
                             (T * 3 * (1280 * 720 + 1920 * 1080)), timed by HIP events in the same run
  resize_vs_copy             copy_ms / launch_ms: 1 would be the copy's rate
  frames_per_s               through submit and wait, next to the native line's

Usage: tools/bench_upscale.py [--batch T] [--seconds S] [--label NAME] [--log FILE]   (lines are appended to FILE)
"""
import argparse
import json
import os
import platform
import sys
import time

SRC = (1280, 720)
BOX = 1920
BLUR_SCALE = 384


def copy_ms(torch, nbytes, reps=10):
    """ms of one device-to-device copy of nbytes (nbytes read and nbytes written), HIP events over reps copies."""
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(torch, fm, W, H, T, seconds, upscale):
    import numpy as np

    from find_motion_amd.synthetic import SyntheticVideo

    k = fm.make_gaussian(BOX, BLUR_SCALE)
    vid = SyntheticVideo(W, H, 0)
    distinct = torch.from_numpy(np.stack([vid.frame(40 + 12 * i) for i in range(4)])).cuda()
    # a ring of two resident batches [T][1][H][W][3], each cycling over the distinct frames from another start
    ring = [distinct[(torch.arange(T, device="cuda") + r) % 4].unsqueeze(1).contiguous() for r in range(2)]
    eng = fm.MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=BOX, ksize=k, threshold=12, avg=0.1, max_batch=T,
                          profile="pix", area_upscale=upscale)
    depth = eng.max_inflight
    t0 = time.perf_counter()
    for i in range(depth):  # every slot once (and the stream's first frame)
        eng.submit_device(ring[i % 2].data_ptr(), T)
    for i in range(depth):
        eng.wait()
    warm = (time.perf_counter() - t0) / depth
    n = max(2 * depth, min(400, int(seconds / max(warm, 1e-6))))
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
    times = {kn: v for kn, v in eng.kernel_times().items() if v[1] > 0}
    out = {"bench": "upscale", "mode": "enlarged" if upscale else "native", "W": W, "H": H, "box": BOX, "ksize": k,
           "work_shape": list(eng.work_shape), "batch": T, "batches": n, "pixel_path": eng.pixel_path,
           "max_inflight": depth, "frames_per_s": round(n * T / dt, 1), "ms_per_batch": round(dt / n * 1e3, 3),
           "contours_per_frame": round(contours / (n * T), 2),
           "launch_ms": {kn: round(ms / cnt, 4) for kn, (ms, cnt) in times.items()},
           "launches_timed": {kn: int(cnt) for kn, (ms, cnt) in times.items()}}
    h, w = eng.work_shape
    eng.close()
    del ring, distinct
    if upscale and "resize_area_up" in times:
        ms, cnt = times["resize_area_up"]
        moved = T * 3 * (W * H + w * h)
        cms = copy_ms(torch, moved // 2)
        out.update(resize_bytes_per_launch=moved, resize_GBps=round(moved / (ms / cnt) / 1e6, 1), copy_ms=round(cms, 4),
                   copy_GBps=round(moved / cms / 1e6, 1), resize_vs_copy=round(cms / (ms / cnt), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=5.0, help="timed seconds per mode (at least 2 x max_inflight batches)")
    ap.add_argument("--label", default="")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # torch's HIP runtime first, as bench.py

    import find_motion_amd as fm

    fm.use_hw_queues()
    lines = [{"bench": "upscale_env", "label": a.label, "host": platform.node(), "device": torch.cuda.get_device_name(0)}]
    print(json.dumps(lines[0]), flush=True)
    for W, H, up in ((SRC[0], SRC[1], True), (BOX, 1080, False)):
        r = run(torch, fm, W, H, a.batch, a.seconds, up)
        r["label"] = a.label
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.log:
        with open(a.log, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
