#!/usr/bin/env python3
"""Write side: GPU baseline JPEG encode rate at 1080p (MJpegEncoder), beside Pillow's libjpeg-turbo on one
host core on the same machine.  Frames: 64 frames of the synthetic video, 4:2:0, at quality 95 and 75, resident
in HBM (a torch tensor), one call per 64 frames.  Per quality: device ms per call and frames/s (HIP events, the
two host round trips that size the buffers included), call-level frames/s (the call plus the copy of every
frame's bytes to the host), bytes per frame, Pillow frames/s on one core, and whether the bytes equal Pillow's.
Usage: tools/bench_mjpeg_encode.py [n_frames] [rounds]"""
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (torch's HIP runtime first, as bench.py)
from PIL import Image  # noqa: E402

from find_motion_amd import MJpegEncoder  # noqa: E402
from find_motion_amd.synthetic import SyntheticVideo  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H = 1920, 1080
v = SyntheticVideo(W, H, 0)
raw = np.stack([v.frame(t) for t in range(N)])
dev = torch.from_numpy(raw).to("cuda:0")
torch.cuda.synchronize()
out = {"frames": N, "width": W, "height": H, "subsampling": "4:2:0", "rounds": ROUNDS}
for q in (95, 75):
    t0 = time.perf_counter()
    ref = []
    for f in raw[:16]:
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(b, "JPEG", quality=q, subsampling=2)
        ref.append(b.getvalue())
    r = {"pillow_1core_fps": round(16 / (time.perf_counter() - t0), 1)}
    enc = MJpegEncoder(W, H, max_frames=N, quality=q, subsampling=2)
    jp = enc.encode_device(dev)  # warm-up (buffers grow to their working size)
    r["equals_pillow"] = jp[:16] == ref
    r["bytes_per_frame"] = int(np.mean([len(j) for j in jp]))
    ms, wall = [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        enc.encode_device(dev)
        wall.append(time.perf_counter() - t0)
        ms.append(enc.last_ms())
    r["device_ms_per_call"] = round(float(np.median(ms)), 3)
    r["device_ms_min"] = round(float(np.min(ms)), 3)
    r["device_fps"] = round(N / (np.median(ms) / 1e3), 1)
    r["call_fps"] = round(N / float(np.median(wall)), 1)
    r["device_fps_over_16_pillow_cores"] = round(r["device_fps"] / (16 * r["pillow_1core_fps"]), 2)
    r["call_fps_over_16_pillow_cores"] = round(r["call_fps"] / (16 * r["pillow_1core_fps"]), 2)
    enc.close()
    out[f"q{q}"] = r
print(json.dumps(out))
