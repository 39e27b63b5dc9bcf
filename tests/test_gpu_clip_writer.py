"""The drop-in's resident pre-motion cache on the GPU (VideoMotion / StreamGroup with gpu_encode=True,
resident_cache=True): cached frames are kept in HBM past their batch, every written frame is queued on the writer by
its device address and encoded at the end of its batch, and the AVI is byte for byte the host MJPG writer's.
"""
import numpy as np
import pytest

from find_motion_amd import MotionEngine, motion, videoio
from find_motion_amd.synthetic import SyntheticVideo

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 40
GEOMETRY = dict(box_size=100, threshold=12, cache_time=0.3, min_time=0.1)  # the cache: 9 frames, three batches of 4


class Watched(MotionEngine):
    """MotionEngine that remembers the most entries its pool held and what it held when it was closed."""
    log = []

    def __init__(self, **kw):
        super().__init__(**kw)
        self.peak = 0
        self.retain_calls = 0

    def retain(self, pairs):
        out = super().retain(pairs)
        self.retain_calls += 1
        self.peak = max(self.peak, self.retained[0])
        return out

    def close(self):
        if getattr(self, "_h", None):
            Watched.log.append(dict(final=self.retained, peak=self.peak, retain_calls=self.retain_calls))
        super().close()


def run(tmp_path, monkeypatch, name, capture, host_writer=False, group=False, batch=4, **kw):
    """One drop-in run into tmp_path/name: (written indices per stream, files per stream, writers, the engine's log)."""
    out = tmp_path / name
    out.mkdir()
    writers = []
    real = videoio.open_writer
    monkeypatch.setattr(motion, "MotionEngine", Watched)
    if host_writer:  # the comparison run: Pillow on the host
        monkeypatch.setattr(videoio, "open_writer", lambda p, c, fps, size, **k: writers.append(
            videoio.MjpegAviWriter(p, fps, size)) or writers[-1])
    else:
        monkeypatch.setattr(videoio, "open_writer", lambda *a, **k: writers.append(real(*a, **k)) or writers[-1])
    Watched.log.clear()
    args = dict(GEOMETRY, outdir=str(out), codec="MJPG")
    args.update(kw)
    if group:
        names = [str(out / f"s{s}") for s in range(len(capture))]
        grp = motion.StreamGroup(names, batch=batch, captures=capture, engine=Watched, **args)
        grp.find_motion()
        vids = grp.videos
    else:
        vm = motion.VideoMotion(filename=str(out / "s0"), capture=capture, batch=batch, **args)
        vm.find_motion()
        vids = [vm]
    monkeypatch.setattr(videoio, "open_writer", real)
    files = [[open(f"{v.filename}_{i + 1}_motion.avi", "rb").read() for i in range(v.outfiles)] for v in vids]
    return [v.written_indices for v in vids], files, writers, dict(Watched.log[-1])


def check_resident(res, host, batches, cache_frames, streams=1):
    written, files, writers, eng = res
    assert written == host[0] and all(written)
    assert files == host[1]
    assert sum(w.host_frames for w in writers) == 0 and sum(w.fallback_frames for w in writers) == 0
    assert sum(w.device_frames for w in writers) == sum(len(x) for x in written)
    assert sum(w.encode_calls for w in writers) <= streams * batches + sum(len(f) for f in files)
    assert eng["final"] == (0, streams * cache_frames) and eng["peak"] <= streams * cache_frames
    assert eng["retain_calls"] <= batches  # one call per batch for the whole engine


def test_single_stream_three_ways(tmp_path, monkeypatch):
    host = run(tmp_path, monkeypatch, "host", videoio.SyntheticCapture(W, H, N, 0), host_writer=True)
    gpu = run(tmp_path, monkeypatch, "gpu", videoio.SyntheticCapture(W, H, N, 0), gpu_encode=True)
    res = run(tmp_path, monkeypatch, "res", videoio.SyntheticCapture(W, H, N, 0), gpu_encode=True, resident_cache=True)
    assert gpu[0] == host[0] and gpu[1] == host[1]
    assert sum(w.host_frames for w in gpu[2]) > 0 and gpu[3]["final"] == (0, 0)  # today's path: no pool
    check_resident(res, host, batches=N // 4, cache_frames=9)
    assert sum(w.encode_calls for w in res[2]) < len(res[0][0]) == sum(w.encode_calls for w in gpu[2])


def nv12_avi(path, n, frames=None):
    vid = SyntheticVideo(W, H, 1)
    yw = videoio.RawAviWriter(path, 30, (W, H), fourcc="NV12")
    for i in range(n):
        f = vid.frame(i) if frames is None else frames[i]
        g = f.astype(np.int32)
        y = ((g[..., 2] * 77 + g[..., 1] * 150 + g[..., 0] * 29) >> 8).astype(np.uint8)
        uv = np.stack([f[::2, ::2, 0], f[::2, ::2, 2]], -1)
        yw.write(np.concatenate([y.ravel(), uv.ravel()]))
    yw.release()
    return path


def test_nv12_source_never_converts_on_the_host(tmp_path, monkeypatch):
    path = nv12_avi(str(tmp_path / "nv12.avi"), N)
    host = run(tmp_path, monkeypatch, "host", videoio.RawAviCapture(path), host_writer=True)

    def no_host_conversion(*a, **k):
        raise AssertionError("videoio.yuv_to_bgr called")

    monkeypatch.setattr(videoio, "yuv_to_bgr", no_host_conversion)
    cap = videoio.RawAviCapture(path)
    assert cap.yuv_format == "NV12"
    res = run(tmp_path, monkeypatch, "res", cap, gpu_encode=True, resident_cache=True)
    check_resident(res, host, batches=N // 4, cache_frames=9)


def quiet_then_motion(quiet=14, moving=16, after=10):
    """The synthetic video moves in every frame, so its cache never outlives a batch.  Here: a still scene (the cache
    fills, evicts, and spans three batches of 4), a square crossing it, the still scene again."""
    yy, xx = np.mgrid[0:H, 0:W]
    still = np.stack([40 + xx // 4, 60 + yy // 4, 80 + (xx + yy) // 8], -1).astype(np.uint8)
    frames = np.repeat(still[None], quiet + moving + after, 0)
    for i in range(moving):
        frames[quiet + i, 60:120, 20 + 12 * i:80 + 12 * i] = (250, 240, 230)
    return frames


@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_cache_of_older_batches_is_written_from_hbm(tmp_path, monkeypatch, source):
    frames = quiet_then_motion()
    if source == "nv12":
        path = nv12_avi(str(tmp_path / "q.avi"), len(frames), frames)
        cap = lambda: videoio.RawAviCapture(path)  # noqa: E731
    else:
        cap = lambda: videoio.ArrayCapture(frames)  # noqa: E731
    host = run(tmp_path, monkeypatch, "host", cap(), host_writer=True)
    gpu = run(tmp_path, monkeypatch, "gpu", cap(), gpu_encode=True)
    if source == "nv12":
        monkeypatch.setattr(videoio, "yuv_to_bgr", lambda *a, **k: (_ for _ in ()).throw(AssertionError("host conversion")))
    res = run(tmp_path, monkeypatch, "res", cap(), gpu_encode=True, resident_cache=True)
    # min_movement_frames = 3 contours counted: the second or third moving frame (15 or 16) starts the clip, with the
    # nine cached frames before it
    assert host[0][0][0] in (15 - 9, 16 - 9)
    assert gpu[0] == host[0] and gpu[1] == host[1]
    check_resident(res, host, batches=len(frames) // 4, cache_frames=9)
    assert res[3]["peak"] == 9  # the full cache was resident, and the clip's first frames were encoded from it


def test_two_stream_group(tmp_path, monkeypatch):
    caps = lambda: [videoio.SyntheticCapture(W, H, N, s) for s in range(2)]  # noqa: E731
    host = run(tmp_path, monkeypatch, "host", caps(), host_writer=True, group=True)
    res = run(tmp_path, monkeypatch, "res", caps(), group=True, gpu_encode=True, resident_cache=True)
    check_resident(res, host, batches=N // 4, cache_frames=9, streams=2)
    assert len(res[0]) == 2


@pytest.mark.parametrize("kw,cache", [(dict(batch=16), 9), (dict(cache_time=0), 0)], ids=["batch16", "cache0"])
def test_other_geometries(tmp_path, monkeypatch, kw, cache):
    host = run(tmp_path, monkeypatch, "host", videoio.SyntheticCapture(W, H, N, 0), host_writer=True, **kw)
    res = run(tmp_path, monkeypatch, "res", videoio.SyntheticCapture(W, H, N, 0), gpu_encode=True, resident_cache=True,
              **kw)
    check_resident(res, host, batches=-(-N // kw.get("batch", 4)), cache_frames=cache)


def test_raw_of_a_retained_yuv_frame_comes_from_hbm(tmp_path, monkeypatch):
    """A YUV-sourced frame waiting in the cache past its batch loads raw from its retained copy (read_retained), not
    through the host conversion."""
    path = nv12_avi(str(tmp_path / "nv12.avi"), 12)
    cap = videoio.RawAviCapture(path)
    want = [videoio.yuv_to_bgr(cap._mm[off: off + cap.frame_bytes], W, H, "NV12") for off, _ in cap._offsets]
    monkeypatch.setattr(videoio, "yuv_to_bgr", lambda *a, **k: (_ for _ in ()).throw(AssertionError("host conversion")))
    vm = motion.VideoMotion(filename=str(tmp_path / "v"), capture=cap, batch=4, outdir=str(tmp_path), codec="MJPG",
                            gpu_encode=True, resident_cache=True, box_size=100, threshold=255, cache_time=0.3,
                            min_time=0.1)
    while vm.read():  # threshold 255: never any motion, every frame goes to the cache
        vm.find_diff()
        vm.step()
    old = [f for f in vm.frame_cache if f._dev is not None]
    assert len(old) >= 4 and vm._engine.retained[0] == len(old)
    for f in old:
        np.testing.assert_array_equal(f.raw, want[f.index])
    vm.cleanup()
