#!/usr/bin/env python3
"""Time of the YOLOv3 object stage (fm_yolo_detect_frames) per call: 17 frames of 1080p -> INTER_AREA to
width 300 -> 416 x 416 blob -> the network -> the decode.

The layer list is yolov3-tiny's (or, with --model yolov3, the full Darknet-53 stack), from the generators the tests
use (tests/yolo_ref.py); the weights are random (no trained file is needed to time a network; the objectness biases
are pushed down, yet how many rows the decode keeps -- `rows_kept` -- is an accident of the weights, not a trained
network's few dozen).
Reported per call: ms per stage (HIP
events), the convolutions' FLOPs over the network stage's time against the 157 TFLOP/s f32-matrix peak, and the
same convolution stack through torch.nn.functional.conv2d in the same run -- a yardstick only: torch picks
its own algorithms and may not keep f32 products exact.

--precision f16 times the half-precision mode (fm_yolo_create_precision) against the f16 matrix peak; --precision
both times the two modes in one process in alternating rounds (f32, f16, f32, f16, ...; at least three rounds of
--iters calls each) and reports for either the median of its rounds' medians and the ratio of the network stages.

Usage: python tools/bench_yolo.py [--model yolov3-tiny|yolov3] [--frames 17] [--iters 10] [--log FILE]
                                  [--precision f32|f16|both] [--rounds 3]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # yolo_ref: the one copy of the two cfg generators

PEAK_TFLOPS = 157.0  # f32-input MFMA, MI355X
PEAK_TFLOPS_F16 = 16 * PEAK_TFLOPS  # v_mfma_f32_32x32x16_f16: 16 x the f32-input instruction's rate


def random_params(layers, seed=0):
    from find_motion_amd import darknet as dk
    rng = np.random.default_rng(seed)
    params = [None] * len(layers)
    for ly in layers:
        if ly["kind"] != dk.CONV:
            continue
        n, c, s = ly["filters"], ly["in_c"], ly["size"]
        w = (rng.standard_normal((n, c, s, s)) * math.sqrt(2.0 / (c * s * s))).astype(np.float32)
        b = (rng.standard_normal(n) * 0.1).astype(np.float32)
        nxt = layers[ly["index"] + 1] if ly["index"] + 1 < len(layers) else None
        if nxt is not None and nxt["kind"] == dk.YOLO:
            b[4::85] -= np.float32(6.0)
        params[ly["index"]] = (w, b)
    return params


def conv_shapes(layers, net=416):
    """(cin, cout, size, stride, pad, leaky, h_in, w_in, source) per convolution, walking the shapes."""
    from find_motion_amd import darknet as dk
    hw, out = [], []
    for ly in layers:
        h = hw[-1] if hw else net
        k = ly["kind"]
        if k == dk.CONV:
            out.append((ly["in_c"], ly["filters"], ly["size"], ly["stride"], ly["pad"], ly["activation"] == "leaky", h))
            h = (h + 2 * ly["pad"] - ly["size"]) // ly["stride"] + 1
        elif k == dk.MAXPOOL:
            h = h if ly["stride"] == 1 else (h + 1) // 2
        elif k == dk.UPSAMPLE:
            h *= 2
        elif k == dk.ROUTE:
            h = hw[ly["layers"][0]]
        hw.append(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov3-tiny", choices=("yolov3-tiny", "yolov3"))
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=None, help="append the result lines to this file")
    ap.add_argument("--precision", default="f32", choices=("f32", "f16", "both"))
    ap.add_argument("--rounds", type=int, default=3, help="with --precision both: alternating rounds per mode (>= 3)")
    a = ap.parse_args()
    if a.precision == "both" and a.rounds < 3:
        ap.error("--precision both takes at least 3 rounds")
    import torch
    import torch.nn.functional as F

    from yolo_ref import full_cfg, tiny_cfg

    from find_motion_amd import YoloDetector
    from find_motion_amd import darknet as dk

    _, layers = dk.parse_cfg(tiny_cfg() if a.model == "yolov3-tiny" else full_cfg())
    params = random_params(layers)
    modes = ("f32", "f16") if a.precision == "both" else (a.precision,)
    dets = {m: YoloDetector(layers, params, [str(i) for i in range(80)], max_frames=a.frames, precision=m) for m in modes}
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (a.frames, 1080, 1920, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    shapes = conv_shapes(layers)
    flops = sum(2.0 * ci * s * s * co * (((h + 2 * p - s) // st + 1) ** 2) for ci, co, s, st, p, _, h in shapes) * a.frames
    names = ("blob", "network", "decode", "total")
    per_round = {m: {k: [] for k in names} for m in modes}  # each round's median
    kept = {}
    for _ in range(a.rounds if a.precision == "both" else 1):
        for m in modes:
            stages = {k: [] for k in names}
            for it in range(a.iters + 2):
                res, _ = dets[m].candidates(dev)
                if it >= 2:
                    ms = dets[m].last_ms()
                    for k in names:
                        stages[k].append(ms[k])
                    kept[m] = sum(len(r) for r in res)
            for k in names:
                per_round[m][k].append(float(np.median(stages[k])))
    meds = {m: {k: float(np.median(v)) for k, v in per_round[m].items()} for m in modes}
    # the same convolutions through torch, layer by layer on inputs of the right shape
    tw = [(torch.from_numpy(params[ly["index"]][0]).cuda(), torch.from_numpy(params[ly["index"]][1]).cuda())
          for ly in layers if ly["kind"] == dk.CONV]
    xs = [torch.randn(a.frames, ci, h, h, device="cuda") for ci, _, _, _, _, _, h in shapes]
    tms = []
    for it in range(a.iters + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for (w, b), x, (_, _, s, st, p, leaky, _) in zip(tw, xs, shapes):
            y = F.conv2d(x, w, b, stride=st, padding=p)
            if leaky:
                y = F.leaky_relu(y, 0.1)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            tms.append(e0.elapsed_time(e1))
    tmed = float(np.median(tms))
    lines = []
    for m in modes:
        med, peak = meds[m], PEAK_TFLOPS_F16 if m == "f16" else PEAK_TFLOPS
        tf = flops / (med["network"] * 1e-3) / 1e12
        out = {"model": a.model, "precision": m, "frames": a.frames, "source": "1920x1080", "layers": len(layers),
               "convs": len(shapes), "ms_blob": round(med["blob"], 3), "ms_network": round(med["network"], 3),
               "ms_decode": round(med["decode"], 3), "ms_total": round(med["total"], 3),
               "conv_gflop_per_call": round(flops / 1e9, 2), "conv_tflops_over_network_ms": round(tf, 2),
               f"fraction_of_{peak:.0f}_tf_peak": round(tf / peak, 4),
               "torch_conv2d_ms": round(tmed, 3), "torch_conv2d_tflops": round(flops / (tmed * 1e-3) / 1e12, 2),
               "rows_kept": kept[m], "iters": a.iters}
        if a.precision == "both":
            out["rounds"] = a.rounds
            out["ms_network_per_round"] = [round(v, 3) for v in per_round[m]["network"]]
        lines.append(json.dumps(out))
    if a.precision == "both":
        lines.append(json.dumps({"model": a.model, "device": torch.cuda.get_device_name(0),
                                 "f32_over_f16_network": round(meds["f32"]["network"] / meds["f16"]["network"], 3),
                                 "f32_over_f16_total": round(meds["f32"]["total"] / meds["f16"]["total"], 3)}))
    for line in lines:
        print(line)
    if a.log:
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    for d in dets.values():
        d.close()


if __name__ == "__main__":
    main()
