#!/usr/bin/env python3
"""Contour points (MotionEngine(contour_points=True), fm_trace.hip) at 1080p, mode F, 256-frame batches from a
device-resident ring, on three workloads:
  synthetic  the bench's content (64 synthetic frames cycled), k 5, threshold 12;
  lattice    a pitch-6 dot lattice (57,600 contours per frame) on 4 frames of the batch, the rest empty;
  ragged     one full-frame blob per frame whose border zigzags along 100 slits (>= 10k points, asserted):
             the unstaged path.
Per workload: device time of the count and emit passes (FM_FLAG_PROFILE, HIP events), fm_wait wall time with
the flag on, off, and with FM_FLAG_CONTOUR_AREA alone (k_contour_area: the same walk with global probes), the
host route the flag replaces (fm_read_mask of every frame + oracle.find_contours_ext(with_points=True) on one
core; measured on a sample of each kind of frame and summed over the batch), points and bytes copied per batch
and the staged / unstaged counts.  Every time is the median of ROUNDS repetitions after 2 warm-up batches, with
[min, max] beside it.  Writes one JSON line to profiles/contour_points_bench.log.
Usage: tools/bench_contour_points.py [rounds] [out.log]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (torch's HIP runtime first, as bench.py)

import oracle  # noqa: E402
from find_motion_amd import MotionEngine  # noqa: E402
from find_motion_amd.synthetic import batch  # noqa: E402

ROUNDS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "contour_points_bench.log")
W, H, T = 1920, 1080, 256


def med(v):
    return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]


def ragged_blob():
    m = np.full((H, W), 255, np.uint8)
    for j in range(100):
        for b in range(125):
            x0 = 100 + 16 * j + 3 * (b % 2)
            m[8 * b:8 * b + 8, x0:x0 + 9] = 0
    return m


def workloads():
    uniq = batch(W, H, 1, 0, 64)
    yield "synthetic", np.concatenate([uniq] * (T // 64)), dict(ksize=5, threshold=12, avg=0.1), \
        [(list(range(1, T, 32)), T)]
    fr = np.zeros((T, 1, H, W, 3), np.uint8)
    lat = np.zeros((H, W), np.uint8)
    lat[2::6, 2::6] = 255
    for t in (40, 100, 160, 220):
        fr[t, 0] = lat[..., None]
    yield "lattice", fr, dict(ksize=1, threshold=0, avg=0.0), [([40], 4), ([41], T - 4)]
    fr = np.zeros((T, 1, H, W, 3), np.uint8)
    fr[1:, 0] = ragged_blob()[None, ..., None]
    yield "ragged", fr, dict(ksize=1, threshold=0, avg=0.0), [([1, 2], T - 1), ([0], 1)]


def timed(eng, ptr, rounds, each=None):
    wait, whole = [], []
    for i in range(2 + rounds):
        eng.reset_kernel_times()
        t0 = time.perf_counter()
        eng.submit_device(ptr, T)
        t1 = time.perf_counter()
        eng.wait()
        t2 = time.perf_counter()
        if i >= 2:
            wait.append((t2 - t1) * 1e3)
            whole.append((t2 - t0) * 1e3)
            if each:
                each(eng)
    return med(wait), med(whole)


out = {"width": W, "height": H, "batch": T, "rounds": ROUNDS, "times": "ms: [median, min, max]"}
for name, frames, cfg, sample in workloads():
    print(f"{name}: ring to the device", flush=True)
    ring = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    kw = dict(n_streams=1, src_w=W, src_h=H, box_size=W, max_batch=T, max_contours=1 << 14, **cfg)
    r = {}
    for mode, flags in (("off", {}), ("points", {"contour_points": True}), ("area", {"contour_area": True})):
        eng = MotionEngine(**flags, **kw)
        r[f"wait_ms_{mode}"], r[f"batch_ms_{mode}"] = timed(eng, ring.data_ptr(), ROUNDS)
        if mode == "points":
            st = eng.trace_stats()
            npts = [sum(len(c.points) for c in eng.contours(t, 0)) for t in range(T)]
            r.update(contours=int(eng.counts().sum()), points=int(sum(npts)), bytes_copied=int(sum(npts)) * 8,
                     staged=st["staged"], unstaged=st["unstaged"], steps=st["steps"],
                     max_npts=max((len(c.points) for t in (1, 40) for c in eng.contours(t, 0)), default=0))
            # the host route on a sample of each kind of frame: read the mask back, trace it on one core
            host = 0.0
            for idx, weight in sample:
                ts = []
                for t in idx:
                    t0 = time.perf_counter()
                    m = eng.mask(t, 0)
                    first = oracle.find_contours_ext(m, cap=1 << 16)
                    cap = max([c["npts"] for c in first], default=0) + 1
                    oracle.find_contours_ext(m, cap=len(first) + 1, with_points=True, pts_cap=cap)
                    ts.append((time.perf_counter() - t0) * 1e3)
                host += float(np.mean(ts)) * weight
            r["host_route_ms"] = round(host, 1)
            r["host_route_frames_sampled"] = sum(len(i) for i, _ in sample)
        eng.close()
        print(f"{name}: {mode} {r[f'wait_ms_{mode}']}", flush=True)
    eng = MotionEngine(contour_points=True, profile=True, **kw)
    dev = {"trace_count": [], "trace_emit": []}
    paths = {}

    def kernel_ms(e):
        kt = e.kernel_times()
        for k in dev:  # a pass = its launches, one per path (register, LDS, big LDS window, unstaged)
            dev[k].append(sum(ms for n, (ms, _) in kt.items() if n.startswith(k)))
        for n, (ms, _) in kt.items():
            if n.startswith("trace_"):
                paths.setdefault(n, []).append(ms)

    timed(eng, ring.data_ptr(), ROUNDS, kernel_ms)
    eng.close()
    r["count_pass_device_ms"], r["emit_pass_device_ms"] = med(dev["trace_count"]), med(dev["trace_emit"])
    r["path_device_ms"] = {n: med(v)[0] for n, v in sorted(paths.items())}
    if name == "ragged":
        assert r["max_npts"] >= 10000 and r["unstaged"] >= T - 1, r
    out[name] = r
    print(f"{name}: {json.dumps(r)}", flush=True)
    del ring
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(line + "\n")
