#!/usr/bin/env python3
"""find_objects with M cascades: one CascadeBank call against the loop of M CascadeClassifier.detect_frames
calls (the drop-in's path before the bank), in one process on one GPU.

Cascades: the reference's files (tests/golden/haarcascades) with their trained thresholds, M = 1, 2, 5, 9.
Frames: 1080p with haar_cases.draw_faces faces; n = 1 from host memory (what find_objects passes), n = 1
resident in HBM, n = 17 resident (the configs[4] call size).  Each cell: a warm-up call of both arms, then
three alternating rounds of --iters calls; a round's figure is wall time per call (every call ends in a stream
synchronisation) and device time per call (last_ms: the HIP events around gray .. window sweep, summed over
the loop's detectors).  The arms' results are compared once per cell.

The decision rule for the drop-in is printed last: on the two rows n = 1 from host memory with M = 2 and with
M = 9, the bank's median over the three rounds must beat the loop's by more than the larger of the two arms'
spreads (slowest minus fastest round).

Usage: python tools/bench_haar_bank.py [--iters 30] > profiles/haar_bank_bench.log
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# M = k runs the first k: the two the decision row names first, then the other windows and the tilted ones
ORDER = ["frontalface_default", "fullbody", "frontalcatface", "profileface", "lowerbody", "frontalface_alt",
         "frontalface_alt2", "frontalface_alt_tree", "frontalcatface_extended"]
MS = (1, 2, 5, 9)
ROUNDS = 3


def face_frames(n, W=1920, H=1080):
    from haar_cases import draw_faces
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        faces = [(480 + 37 * (i % 7), 420 + 23 * (i % 5), 300), (1380 - 29 * (i % 6), 600 + 17 * (i % 4), 230)]
        draw_faces(out[i], faces[:1 + i % 2] if i % 3 else faces, seed=i)
    return out


def rects(a):
    return [tuple(r) for r in np.asarray(a).reshape(-1, 4).tolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30, help="calls per round")
    args = ap.parse_args()
    import torch  # noqa: F401  (torch's HIP runtime first, then libfm_hip)
    from find_motion_amd import CascadeBank, CascadeClassifier
    from find_motion_amd.cascade import parse
    from golden_cases import cascade_xml

    if not torch.cuda.is_available():
        raise SystemExit("bench_haar_bank: no GPU")
    cascades = [parse(cascade_xml(name)) for name in ORDER]
    frames = face_frames(17)
    dev = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    sets = [("n=1 host", frames[:1]), ("n=1 resident", dev[:1]), ("n=17 resident", dev)]
    print(f"# {torch.cuda.get_device_name(0)}; {args.iters} calls per round, {ROUNDS} alternating rounds per cell; ms per call")
    print("# cascades in order: " + ", ".join(f"{n} {c.win_w}x{c.win_h}{' tilted' if c.has_tilted else ''}"
                                              for n, c in zip(ORDER, cascades)))
    print(f"{'frames':14s} {'M':>2s}  {'bank wall (rounds)':>26s} {'median':>7s}  {'loop wall (rounds)':>26s} {'median':>7s}"
          f"  {'bank dev':>8s} {'loop dev':>8s}  detections")
    rows = {}
    for M in MS:
        bank = CascadeBank(cascades[:M], roi_upscale=True)
        dets = [CascadeClassifier(c, roi_upscale=True) for c in cascades[:M]]

        def run_bank(src):
            out = bank.detect_frames(src, 300, 1.1, 5)
            return out, bank.last_ms()

        def run_loop(src):
            out, ms = [], 0.0
            for d in dets:
                out.append(d.detect_frames(src, 300, 1.1, 5))
                ms += d.last_ms()
            return out, ms

        for label, src in sets:
            ob, _ = run_bank(src)  # warm-up of both arms (allocations, tables), and the results compared
            ol, _ = run_loop(src)
            if [[rects(r) for r in per] for per in ob] != [[rects(r) for r in per] for per in ol]:
                raise SystemExit(f"bench_haar_bank: the bank's results differ from the loop's ({label}, M={M})")
            wall = {"bank": [], "loop": []}
            devms = {"bank": [], "loop": []}
            for _ in range(ROUNDS):
                for arm, fn in (("bank", run_bank), ("loop", run_loop)):
                    ms = 0.0
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        ms += fn(src)[1]
                    wall[arm].append((time.perf_counter() - t0) * 1e3 / args.iters)
                    devms[arm].append(ms / args.iters)
            row = {arm: dict(rounds=[round(v, 4) for v in wall[arm]], median=statistics.median(wall[arm]),
                             spread=max(wall[arm]) - min(wall[arm]), device_ms=statistics.median(devms[arm]))
                   for arm in wall}
            rows[(label, M)] = row
            fmt = lambda v: " ".join(f"{x:8.3f}" for x in v)  # noqa: E731
            print(f"{label:14s} {M:2d}  {fmt(wall['bank'])} {row['bank']['median']:7.3f}  {fmt(wall['loop'])} "
                  f"{row['loop']['median']:7.3f}  {row['bank']['device_ms']:8.3f} {row['loop']['device_ms']:8.3f}  "
                  f"{sum(len(r) for per in ob for r in per)}", flush=True)
        bank.close()
        for d in dets:
            d.close()
    verdict = {}
    for M in (2, 9):
        r = rows[("n=1 host", M)]
        margin = max(r["bank"]["spread"], r["loop"]["spread"])
        verdict[M] = dict(bank_median=round(r["bank"]["median"], 4), loop_median=round(r["loop"]["median"], 4),
                          larger_spread=round(margin, 4),
                          bank_wins=bool(r["loop"]["median"] - r["bank"]["median"] > margin))
    use = all(v["bank_wins"] for v in verdict.values())
    print(json.dumps({"rule": "n=1 host, M=2 and M=9: loop median - bank median > larger spread, on both rows",
                      "rows": {f"M={m}": v for m, v in verdict.items()}, "find_objects_uses_bank": use}))


if __name__ == "__main__":
    main()
