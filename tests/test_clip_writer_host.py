"""The resident pre-motion cache and the queued writer on a machine without a GPU: MjpegAviWriter.queue_device /
flush with a stub encoder (Pillow behind it), and the drop-in's resident_cache state machine on an engine stand-in
whose retain / release / read_retained are numpy-backed and whose "device memory" forgets a slot at the next wait
and a retained copy at its release, so a stale address fails the run.
"""
import itertools
import logging
from argparse import ArgumentParser

import numpy as np
import pytest

import jpeg_cases as jc
from find_motion_amd import _native, cli, motion, videoio
from find_motion_amd._native import FM_EINVAL, FM_ENOMEM, Contour, FMError
from test_jpeg_encode_host import DEVICE, DeviceOracleEngine

pytestmark = pytest.mark.skipif(jc.Image is None, reason="Pillow (libjpeg-turbo) is the reference encoder")

W, H = 53, 37
ADDRESS = itertools.count(0x900000)  # "device addresses" handed out here: never reused


class StubEncoder:
    """MJpegEncoder's surface with Pillow behind it; calls = the frames of every encoder call."""
    quality, subsampling, restart_interval = 95, 2, 0
    made = []

    def __init__(self, width=0, height=0, max_frames=1, device=0, **kw):
        self.max_frames, self.calls, self.refuse, self.closed = max_frames, [], None, False
        StubEncoder.made.append(self)

    def _run(self, frames):
        self.calls.append(len(frames))
        if len(frames) > self.max_frames:
            raise FMError(FM_EINVAL, "more frames than max_frames")
        if self.refuse is not None and self.refuse(len(frames)):
            raise FMError(FM_EINVAL, "refused")
        return [jc.encode(np.asarray(f), quality=95, subsampling=2) for f in frames]

    def encode(self, frames):
        return self._run(list(frames))

    def encode_device(self, ptrs, n=None):
        return self._run([DEVICE[p] for p in ptrs])

    def close(self):
        self.closed = True


def device_frames(n, seed=0):
    """n frames "in device memory": their addresses and the frames."""
    frames = [jc.image(H, W, "smooth", seed + i) for i in range(n)]
    ptrs = []
    for f in frames:
        ptrs.append(next(ADDRESS))
        DEVICE[ptrs[-1]] = f
    return ptrs, frames


def host_file(path, frames, jpegs=()):
    """The host writer's file of `frames` (arrays, or bytes for write_jpeg) in order."""
    w = videoio.MjpegAviWriter(path, 25, (W, H))
    for f in frames:
        w.write_jpeg(f) if isinstance(f, bytes) else w.write(f)
    w.release()
    return open(path, "rb").read()


# --- the writer ------------------------------------------------------------------------------------------------

def test_file_order_is_call_order(tmp_path):
    ptrs, fr = device_frames(5)
    extra = jc.image(H, W, "noise", 77)
    jpeg = jc.encode(jc.image(H, W, "noise", 78), quality=60)
    enc = StubEncoder(max_frames=8)
    w = videoio.MjpegAviWriter(str(tmp_path / "q.avi"), 25, (W, H), encoder=enc)
    w.queue_device(ptrs[0])
    w.queue_device(ptrs[1])
    assert w.n == 0 and w.device_frames == 0  # nothing written or counted before the flush
    w.write(extra)                            # flushes the two, then the host frame
    assert w.n == 3 and w.device_frames == 2
    w.queue_device(ptrs[2])
    w.write_jpeg(jpeg)
    w.queue_device(ptrs[3])
    w.write_device(ptrs[4])
    w.flush()                                 # nothing left: no encoder call
    w.release()
    assert enc.calls == [2, 1, 1, 1, 1] and w.encode_calls == 5
    assert (w.device_frames, w.host_frames, w.fallback_frames) == (5, 1, 0)
    want = host_file(str(tmp_path / "h.avi"), [fr[0], fr[1], extra, fr[2], jpeg, fr[3], fr[4]])
    assert open(str(tmp_path / "q.avi"), "rb").read() == want


@pytest.mark.parametrize("max_frames,calls", [(1, [1] * 7), (3, [3, 3, 1]), (100, [7])])
def test_flush_chunks_by_max_frames(tmp_path, max_frames, calls):
    ptrs, fr = device_frames(7, seed=10)
    enc = StubEncoder(max_frames=max_frames)
    w = videoio.MjpegAviWriter(str(tmp_path / "q.avi"), 25, (W, H), encoder=enc)
    for p in ptrs:
        w.queue_device(p)
    w.flush()
    assert enc.calls == calls and w.encode_calls == len(calls) and w.device_frames == 7
    w.release()
    assert open(str(tmp_path / "q.avi"), "rb").read() == host_file(str(tmp_path / "h.avi"), fr)


def test_refused_chunk_falls_back_frame_by_frame(tmp_path):
    ptrs, fr = device_frames(4, seed=20)
    enc = StubEncoder(max_frames=4)
    enc.refuse = lambda n: True
    w = videoio.MjpegAviWriter(str(tmp_path / "q.avi"), 25, (W, H), encoder=enc)
    fetched = []
    for i, p in enumerate(ptrs):  # raw as an array, and as a callable that fetches it
        w.queue_device(p, fr[i] if i % 2 else (lambda i=i: fetched.append(i) or fr[i]))
    w.flush()
    assert enc.calls == [4, 1, 1, 1, 1] and fetched == [0, 2]
    assert (w.device_frames, w.fallback_frames, w.n) == (0, 4, 4)
    enc.refuse = lambda n: n > 1  # the chunk is refused, its frames one by one are not
    for p in ptrs:
        w.queue_device(p)
    w.flush()
    assert (w.device_frames, w.fallback_frames, w.n) == (4, 4, 8)
    enc.refuse = lambda n: True
    w.queue_device(ptrs[0], fr[0])
    w.queue_device(ptrs[1])  # refused and nothing to fall back on
    with pytest.raises(FMError):
        w.flush()
    assert not w._pending
    w.release()
    want = host_file(str(tmp_path / "h.avi"), fr + fr + fr[:1])
    assert open(str(tmp_path / "q.avi"), "rb").read() == want


def test_release_flushes_first(tmp_path):
    ptrs, fr = device_frames(3, seed=30)
    enc = StubEncoder(max_frames=2)
    w = videoio.MjpegAviWriter(str(tmp_path / "q.avi"), 25, (W, H), encoder=enc)
    w.own_encoder = True
    for p in ptrs:
        w.queue_device(p)
    w.release()
    assert enc.calls == [2, 1] and enc.closed and w.device_frames == 3
    assert open(str(tmp_path / "q.avi"), "rb").read() == host_file(str(tmp_path / "h.avi"), fr)
    with pytest.raises(ValueError):
        videoio.MjpegAviWriter(str(tmp_path / "n.avi"), 25, (W, H)).queue_device(ptrs[0])


def test_open_writer_encode_batch(tmp_path, monkeypatch):
    monkeypatch.setattr(_native, "MJpegEncoder", StubEncoder)
    p = str(tmp_path / "o.avi")
    w = videoio.open_writer(p, "MJPG", 25, (W, H), gpu_encode=True)
    assert w.encoder.max_frames == 1  # the default stays one frame per call
    w.release()
    w = videoio.open_writer(p, "MJPG", 25, (W, H), gpu_encode=True, encode_batch=13)
    assert w.encoder.max_frames == 13 and w.own_encoder
    w.release()


# --- the drop-in -------------------------------------------------------------------------------------------------

class RetainingEngine(DeviceOracleEngine):
    """DeviceOracleEngine with a numpy-backed pool of retained frames.  A slot address lives until the next wait(),
    a retained one until its release: DEVICE forgets them then, so encoding from a stale address is a KeyError."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.capacity, self.pool, self.peak, self.retain_calls, self.reads = 0, {}, 0, 0, 0
        self._slot_keys = []

    def wait(self):
        super().wait()
        for k in self._slot_keys:
            DEVICE.pop(k, None)
        self._slot_keys = []

    def frame_device_ptr(self, t, s):
        self._slot_keys.append(next(ADDRESS))
        DEVICE[self._slot_keys[-1]] = self._cur[t, s].copy()
        return self._slot_keys[-1]

    def reserve_retained(self, n):
        assert not self.pool
        self.capacity = int(n)

    def retain(self, pairs):
        self.retain_calls += 1
        if len(self.pool) + len(pairs) > self.capacity:
            raise FMError(FM_ENOMEM, "pool exhausted")
        out = []
        for t, s in pairs:
            key = next(ADDRESS)
            DEVICE[key] = self.pool[key] = self._cur[t, s].copy()
            out.append(key)
        self.peak = max(self.peak, len(self.pool))
        return out

    def release(self, ptrs):
        if len(set(ptrs)) != len(ptrs) or any(p not in self.pool for p in ptrs):
            raise FMError(FM_EINVAL, "not a retained frame")
        for p in ptrs:
            del self.pool[p], DEVICE[p]

    def read_retained(self, ptr):
        self.reads += 1
        return self.pool[ptr].copy()

    @property
    def retained(self):
        return len(self.pool), self.capacity


# contours per frame: quiet (the cache fills and evicts), a burst shorter than min_movement_frames (3), quiet again,
# motion (the cache is written, then frame after frame), quiet past the decay, and a second clip's motion
SCRIPT = [0] * 22 + [1] * 2 + [0] * 7 + [1] * 9 + [0] * 14 + [1] * 6 + [0] * 3


class ScriptedEngine(RetainingEngine):
    """... whose frames carry SCRIPT's contour counts instead of the oracle's."""

    def wait(self):
        self._base = getattr(self, "_base", 0) + len(getattr(self, "_cur", ()))
        super().wait()

    def contours(self, t, s):
        return [Contour(1, 1, 4, 4, (1, 1), None)] * SCRIPT[self._base + t]


def run_dropin(tmp_path, monkeypatch, name, engine_cls, host_writer=False, n=len(SCRIPT), batch=4, cache_time=0.3, **kw):
    w, h = 64, 48
    eng = engine_cls(n_streams=1, src_w=w, src_h=h, box_size=64, ksize=3, threshold=12, avg=0.1, max_batch=batch)
    monkeypatch.setattr(_native, "MJpegEncoder", StubEncoder)
    monkeypatch.setattr(videoio, "cv2", None)
    writers = []
    real = videoio.open_writer
    if host_writer:
        monkeypatch.setattr(videoio, "open_writer", lambda p, c, fps, size, **k: writers.append(
            videoio.MjpegAviWriter(p, fps, size)) or writers[-1])
    else:
        monkeypatch.setattr(videoio, "open_writer", lambda *a, **k: writers.append(real(*a, **k)) or writers[-1])
    vm = motion.VideoMotion(filename=str(tmp_path / name), capture=videoio.SyntheticCapture(w, h, n, 0), engine=eng,
                            batch=batch, box_size=64, cache_time=cache_time, min_time=0.1, fps=30, threshold=12,
                            outdir=str(tmp_path), codec="MJPG", **kw)
    vm.find_motion()
    monkeypatch.setattr(videoio, "open_writer", real)
    files = [open(str(tmp_path / name) + f"_{i + 1}_motion.avi", "rb").read() for i in range(vm.outfiles)]
    return vm, eng, writers, files


@pytest.mark.parametrize("cleanup", [False, True])
def test_scripted_state_machine_releases_what_it_retains(tmp_path, monkeypatch, cleanup):
    host = run_dropin(tmp_path, monkeypatch, "host", ScriptedEngine, host_writer=True, cleanup=cleanup)
    vm, eng, writers, files = run_dropin(tmp_path, monkeypatch, "res", ScriptedEngine, gpu_encode=True,
                                         resident_cache=True, cleanup=cleanup)
    assert vm._resident and vm.cache_frames == 9 and eng.capacity == 9
    assert vm.written_indices == host[0].written_indices and len(vm.written_indices) > 20
    # the burst wrote nothing; the clip starts with the cached frames before its third moving frame
    assert vm.written_indices[0] == 22 + 2 + 7 + 2 - 9
    assert files == host[3] and len(files) == 1
    assert eng.retained == (0, 9) and 0 < eng.peak <= 9
    assert not vm._kept and not vm._free
    assert sum(w.host_frames for w in writers) == 0 and sum(w.fallback_frames for w in writers) == 0
    assert sum(w.device_frames for w in writers) == len(vm.written_indices)
    batches = -(-len(SCRIPT) // 4)
    assert eng.retain_calls <= batches and sum(w.encode_calls for w in writers) <= batches + len(files)
    assert max(c for w in StubEncoder.made[-1:] for c in w.calls) > 1  # a batch's frames went in one call


def test_resident_cache_off_is_todays_path(tmp_path, monkeypatch):
    host = run_dropin(tmp_path, monkeypatch, "host", ScriptedEngine, host_writer=True)
    vm, eng, writers, files = run_dropin(tmp_path, monkeypatch, "gpu", ScriptedEngine, gpu_encode=True)
    assert not vm._resident and eng.retain_calls == 0 and eng.capacity == 0
    assert files == host[3]
    assert sum(w.host_frames for w in writers) > 0  # the cached frames of older batches: the host route


@pytest.mark.parametrize("kw", [dict(cache_time=0), dict(batch=16), dict(batch=1)], ids=str)
def test_resident_cache_geometries(tmp_path, monkeypatch, kw):
    host = run_dropin(tmp_path, monkeypatch, "host", ScriptedEngine, host_writer=True, **kw)
    vm, eng, writers, files = run_dropin(tmp_path, monkeypatch, "res", ScriptedEngine, gpu_encode=True,
                                         resident_cache=True, **kw)
    assert vm.written_indices == host[0].written_indices and files == host[3]
    assert eng.retained == (0, vm.cache_frames) and eng.peak <= vm.cache_frames
    assert sum(w.host_frames + w.fallback_frames for w in writers) == 0
    assert writers[0].encoder is None  # released
    assert StubEncoder.made[-1].max_frames == min(kw.get("batch", 4) + vm.cache_frames, 64)


def test_resident_cache_needs_the_gpu_mjpg_writer(tmp_path, monkeypatch):
    for kw in (dict(), dict(gpu_encode=True, codec_override="DIB ")):
        codec = kw.pop("codec_override", None)
        w, h = 64, 48
        eng = ScriptedEngine(n_streams=1, src_w=w, src_h=h, box_size=64, ksize=3, threshold=12, avg=0.1, max_batch=4)
        vm = motion.VideoMotion(filename=str(tmp_path / "x"), capture=videoio.SyntheticCapture(w, h, 4, 0), engine=eng,
                                batch=4, box_size=64, outdir=str(tmp_path), resident_cache=True,
                                **dict(kw, **({"codec": codec} if codec else {})))
        assert vm.resident_cache and not vm._resident and eng.capacity == 0
        vm.cleanup()


def test_engine_without_retain_warns_and_writes_todays_file(tmp_path, monkeypatch, caplog):
    class Plain(ScriptedEngine):
        retain = property()  # (hasattr is False)

    today = run_dropin(tmp_path, monkeypatch, "today", ScriptedEngine, gpu_encode=True)
    with caplog.at_level(logging.WARNING, logger="find_motion_amd.VideoMotion"):
        vm, eng, writers, files = run_dropin(tmp_path, monkeypatch, "plain", Plain, gpu_encode=True, resident_cache=True)
    assert not hasattr(eng, "retain")
    assert sum("cannot retain" in r.getMessage() for r in caplog.records) == 1
    assert not vm._resident and files == today[3] and vm.written_indices == today[0].written_indices
    assert [(w.device_frames, w.host_frames) for w in writers] == [(w.device_frames, w.host_frames) for w in today[2]]


def test_flag_and_ini_key_reach_video_motion(tmp_path):
    parser = ArgumentParser()
    cli.get_args(parser)
    args = parser.parse_args(["x.avi"])
    assert args.resident_cache is False and cli._job_kwargs(args)["resident_cache"] is False
    args = parser.parse_args(["x.avi", "--gpu-encode", "--resident-cache"])
    assert args.resident_cache is True and cli._job_kwargs(args)["resident_cache"] is True
    ini = tmp_path / "c.ini"
    ini.write_text("[settings]\nresident_cache = True\ngpu_encode = True\n")
    args = cli.process_config(str(ini), parser.parse_args(["x.avi"]))
    kw = cli._job_kwargs(args)
    assert kw["resident_cache"] is True and kw["gpu_encode"] is True
    ini.write_text("[settings]\nresident_cache = yes\n")
    with pytest.raises(ValueError):
        cli.process_config(str(ini), parser.parse_args(["x.avi"]))
    eng = ScriptedEngine(n_streams=1, src_w=64, src_h=48, box_size=64, ksize=3, threshold=12, avg=0.1, max_batch=4)
    vm = motion.VideoMotion(filename=str(tmp_path / "v"), capture=videoio.SyntheticCapture(64, 48, 4, 0), engine=eng,
                            batch=4, box_size=64, outdir=str(tmp_path), fps=30, cache_time=0.5,
                            **{k: kw[k] for k in ("resident_cache", "gpu_encode")})
    assert vm._resident and eng.capacity == 15
    vm.cleanup()
