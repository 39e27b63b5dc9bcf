#!/usr/bin/env python3
"""YUV input (fm_submit_yuv) at 1080p with 256-frame batches, one stream, mode D (box 100):

(a) device time of the `yuv2bgr` kernel per batch and the bytes per second it moves (YUV in + BGR out), per
    format, frames resident in HBM -- beside a device-to-device copy that moves the same number of bytes
    (reads half of them, writes half), timed in the same run: the copy is the yardstick, not the HBM peak;
(b) host-fed end-to-end frames/s through BatchFeeder (decoder thread -> page-locked batches -> engine), the
    same frames fed as BGR, as NV12 and as YUY2, alternating over a few rounds in one run on one box (every run
    is printed, the ratios are between the medians), and each stage alone: the copy threads filling a
    page-locked batch, and the engine fed from one filled batch (DMA + conversion + hot path).

Usage: tools/bench_yuv_input.py [--batches N] [--rounds R] [--log FILE]      (the lines are appended to FILE as well)
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (torch's HIP runtime first, as bench.py)

import find_motion_amd  # noqa: E402
from find_motion_amd import MotionEngine, videoio  # noqa: E402
from find_motion_amd.feeder import BatchFeeder  # noqa: E402
from find_motion_amd.synthetic import SyntheticVideo  # noqa: E402

W, H, T, BOX = 1920, 1080, 256, 100
FORMATS = ("NV12", "I420", "YUY2", "UYVY")


def to_yuv(bgr, fmt):
    """A BGR frame as a tight YUV frame (BT.601 luma, chroma by dropping samples: the content only has to move)."""
    f = bgr.astype(np.int32)
    Y = (16 + ((f[..., 2] * 66 + f[..., 1] * 129 + f[..., 0] * 25 + 128) >> 8)).astype(np.uint8)
    U = (128 + ((-f[..., 2] * 38 - f[..., 1] * 74 + f[..., 0] * 112 + 128) >> 8)).astype(np.uint8)
    V = (128 + ((f[..., 2] * 112 - f[..., 1] * 94 - f[..., 0] * 18 + 128) >> 8)).astype(np.uint8)
    if fmt == "NV12":
        return np.concatenate([Y.ravel(), np.stack([U[::2, ::2], V[::2, ::2]], -1).ravel()])
    if fmt == "I420":
        return np.concatenate([Y.ravel(), U[::2, ::2].ravel(), V[::2, ::2].ravel()])
    u, v = U[:, ::2], V[:, ::2]
    q = [Y[:, ::2], u, Y[:, 1::2], v] if fmt == "YUY2" else [u, Y[:, ::2], v, Y[:, 1::2]]
    return np.stack(q, -1).ravel()


class CycleCapture:
    """n frames cycling over a few distinct ones held in RAM: BGR arrays (read) or YUV byte frames (read_yuv)."""

    def __init__(self, frames, n, yuv_format=None):
        self.frames, self.n, self.i = frames, n, 0
        if yuv_format:
            self.yuv_format = yuv_format
            self.read_yuv = self.read

    def isOpened(self):  # noqa: N802
        return True

    def read(self):
        if self.i >= self.n:
            return False, None
        f = self.frames[self.i % len(self.frames)]
        self.i += 1
        return True, f

    def get(self, prop):
        return {videoio.CAP_PROP_FRAME_WIDTH: W, videoio.CAP_PROP_FRAME_HEIGHT: H,
                videoio.CAP_PROP_FRAME_COUNT: self.n}.get(prop, 0.0)

    def release(self):
        pass


def engine(**kw):
    return MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=BOX, ksize=find_motion_amd.make_gaussian(BOX, 20),
                        threshold=12, avg=0.1, max_batch=T, **kw)


def kernel_bench(fmt, src_frames, reps):
    """(a): yuv2bgr on a resident batch, `reps` launches after one pass over the slot ring; the copy yardstick
    alongside."""
    fb = find_motion_amd.yuv_frame_bytes(W, H, fmt)
    host = np.stack([src_frames[t % len(src_frames)] for t in range(T)])
    dev = torch.from_numpy(host).cuda()
    eng = engine(profile=True)
    for _ in range(eng.max_inflight):  # a slot's input buffer is allocated on its first use: warm every slot
        eng.submit_yuv_device(dev.data_ptr(), T, fmt)
        eng.wait()
    eng.reset_kernel_times()
    for _ in range(reps):
        eng.submit_yuv_device(dev.data_ptr(), T, fmt)
        eng.wait()
    ms, launches = eng.kernel_times()["yuv2bgr"]
    eng.close()
    moved = T * (fb + W * H * 3)  # bytes read + bytes written by one launch
    # the yardstick: a device copy that moves the same bytes (reads moved / 2, writes moved / 2)
    a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        b.copy_(a)
    ev[1].record()
    torch.cuda.synchronize()
    copy_ms = ev[0].elapsed_time(ev[1]) / reps
    del a, b, dev
    k_ms = ms / launches
    return {"bench": "yuv2bgr_kernel", "format": fmt, "frames": T, "launches": int(launches),
            "kernel_ms_per_batch": round(k_ms, 4), "bytes_moved_per_batch": moved,
            "kernel_GBps": round(moved / k_ms / 1e6, 1), "copy_same_bytes_ms": round(copy_ms, 4),
            "copy_GBps": round(moved / copy_ms / 1e6, 1), "kernel_over_copy_time": round(k_ms / copy_ms, 3),
            "kernel_frames_per_s": round(T / k_ms * 1e3)}


def host_fed(name, frames, fmt, n_batches, depth):
    """(b): n_batches batches through BatchFeeder from frames in RAM; the buffers are page-locked beforehand."""
    eng = engine()
    cap = CycleCapture(frames, T * n_batches, fmt)
    bufs = [eng.host_buffer_yuv(T, fmt) if fmt else eng.host_buffer(T) for _ in range(depth + 2)]
    t0 = time.perf_counter()
    feeder = BatchFeeder(eng, [cap], T, depth=depth, buffers=bufs)
    assert feeder.yuv == fmt
    n = total = 0
    for b in feeder:
        n += b.T
        total += int(eng.counts().sum())
    dt = time.perf_counter() - t0
    eng.close()
    bpf = find_motion_amd.yuv_frame_bytes(W, H, fmt) if fmt else W * H * 3
    return {"bench": "host_fed", "input": name, "frames": n, "seconds": round(dt, 3), "frames_per_s": round(n / dt, 1),
            "bytes_per_frame": bpf, "input_GBps": round(n * bpf / dt / 1e9, 2), "contours": total,
            "copy_threads": feeder._copiers._max_workers, "depth": depth}


def bounds(name, frames, fmt, n_batches, depth):
    """What bounds (b), each stage alone on the same buffers: the copy threads filling one page-locked batch
    (no GPU), and the engine fed from one already-filled batch (the host-to-device copy + the kernels, no host
    copy)."""
    from concurrent.futures import ThreadPoolExecutor
    eng = engine()
    buf = eng.host_buffer_yuv(T, fmt) if fmt else eng.host_buffer(T)
    workers = max(1, min(8, len(os.sched_getaffinity(0))))  # as BatchFeeder sizes its pool
    pool = ThreadPoolExecutor(workers)

    def put(t):
        np.copyto(buf[t, 0], frames[t % len(frames)].reshape(buf[t, 0].shape))

    list(pool.map(put, range(T)))  # touch the pages
    t0 = time.perf_counter()
    for _ in range(4):
        list(pool.map(put, range(T)))
    fill = 4 * T / (time.perf_counter() - t0)
    pool.shutdown()
    sub = (lambda: eng.submit_yuv(buf, fmt)) if fmt else (lambda: eng.submit(buf))
    for _ in range(2):
        sub()
        eng.wait()
    t0 = time.perf_counter()
    inflight = 0
    for _ in range(n_batches):
        if inflight == depth:
            eng.wait()
            inflight -= 1
        sub()
        inflight += 1
    while inflight:
        eng.wait()
        inflight -= 1
    fed = n_batches * T / (time.perf_counter() - t0)
    eng.close()
    bpf = find_motion_amd.yuv_frame_bytes(W, H, fmt) if fmt else W * H * 3
    return {"bench": "host_fed_stage", "input": name, "fill_frames_per_s": round(fill, 1),
            "fill_GBps": round(fill * bpf / 1e9, 2), "fill_threads": workers, "submit_frames_per_s": round(fed, 1),
            "submit_GBps": round(fed * bpf / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, default=48, help="256-frame batches per host-fed run")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the host-fed runs")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per format in the kernel part")
    ap.add_argument("--depth", type=int, default=3, help="batches in flight in the host-fed runs")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    find_motion_amd.use_hw_queues(8, force=True)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    emit({"bench": "yuv_input", "device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
          "cpus_usable": len(os.sched_getaffinity(0)), "frame": f"{W}x{H}", "batch": T, "box": BOX,
          "torch": torch.__version__, "hip": torch.version.hip})
    vid = SyntheticVideo(W, H, 0)
    bgr = [vid.frame(t * 4) for t in range(8)]
    yuv = {fmt: [to_yuv(f, fmt) for f in bgr] for fmt in FORMATS}
    for fmt in FORMATS:
        emit(kernel_bench(fmt, yuv[fmt], args.reps))
    # what the host-fed BGR run sees: the frames the YUV runs' conversion produces, so every run has the same content
    conv = {fmt: [videoio.yuv_to_bgr(f, W, H, fmt) for f in yuv[fmt]] for fmt in ("NV12",)}
    runs = [("BGR", conv["NV12"], None), ("NV12", yuv["NV12"], "NV12"), ("YUY2", yuv["YUY2"], "YUY2")]
    # other work shares the host and its PCIe links: the inputs alternate within a round, the rounds repeat,
    # every run is printed and the ratios are taken between the medians
    fed = {name: [] for name, _, _ in runs}
    sub = {name: [] for name, _, _ in runs}
    for rnd in range(args.rounds):
        for name, frames, fmt in runs:
            r = host_fed(name, frames, fmt, args.batches, args.depth)
            r["round"] = rnd
            fed[name].append(r["frames_per_s"])
            emit(r)
        for name, frames, fmt in runs:
            r = bounds(name, frames, fmt, args.batches, args.depth)
            r["round"] = rnd
            sub[name].append(r["submit_frames_per_s"])
            emit(r)
    med = lambda v: float(np.median(v))  # noqa: E731
    emit({"bench": "host_fed_ratio", "rounds": args.rounds,
          "feeder_median_frames_per_s": {k: round(med(v), 1) for k, v in fed.items()},
          "feeder_nv12_over_bgr": round(med(fed["NV12"]) / med(fed["BGR"]), 3),
          "feeder_yuy2_over_bgr": round(med(fed["YUY2"]) / med(fed["BGR"]), 3),
          "submit_median_frames_per_s": {k: round(med(v), 1) for k, v in sub.items()},
          "submit_nv12_over_bgr": round(med(sub["NV12"]) / med(sub["BGR"]), 3),
          "submit_yuy2_over_bgr": round(med(sub["YUY2"]) / med(sub["BGR"]), 3),
          "byte_ratio_nv12": 2.0, "byte_ratio_yuy2": 1.5})
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
