"""The write side on a machine without a GPU: the numpy restatement of the baseline JPEG encode
(tests/jpeg_encode_ref.py) and fm_jpeg_header against Pillow's libjpeg-turbo, byte for byte, and the writer
plumbing (videoio.open_writer / MjpegAviWriter, VideoMotion._put, --gpu-encode) with a stand-in encoder.
"""
import ctypes as C
from argparse import ArgumentParser

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_encode_ref as ref
from fake_engine import OracleEngine
from find_motion_amd import _native, cli, motion, videoio

pytestmark = pytest.mark.skipif(jc.Image is None, reason="Pillow (libjpeg-turbo) is the reference encoder")

SHAPES = [(16, 16), (37, 53), (8, 9), (61, 33), (9, 2), (5, 4), (1, 1), (17, 31)]
# (quality, subsampling, restart interval in MCUs; "row" = MCUs per row)
SETTINGS = [(95, 2, 0), (30, 2, 0), (95, 0, 0), (50, 1, 0), (100, 2, 0), (80, 2, 3), (70, 1, "row")]
CASES = [(s, c) for s in SHAPES for c in SETTINGS] + [((61, 33), (75, 2, 1))]  # 12 intervals: RST7 wraps to RST0


def restart_mcus(W, subsampling, restart):
    return -(-W // (8 * ref.SAMPLING[subsampling][0])) if restart == "row" else restart


def pillow(bgr, quality, subsampling, restart):
    kw = dict(quality=quality, subsampling=subsampling)
    if restart == "row":
        kw["restart_marker_rows"] = 1
    elif restart:
        kw["restart_marker_blocks"] = restart
    return jc.encode(bgr, **kw)


@pytest.mark.parametrize("shape,setting", CASES, ids=lambda v: "x".join(str(x) for x in v))
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_restatement_equals_pillow(shape, setting, kind):
    H, W = shape
    q, s, r = setting
    img = jc.image(H, W, kind, seed=H * 100 + W)
    got = ref.encode(img, q, s, restart_mcus(W, s, r))
    want = pillow(img, q, s, r)
    n = len(ref.header(W, H, q, s, restart_mcus(W, s, r)))
    assert got[:n] == want[:n], "header"
    assert got == want


def test_restart_case_wraps_the_marker_numbers():
    data = pillow(jc.image(61, 33, "noise"), 75, 2, 1)
    scan = data[len(ref.header(33, 61, 75, 2, 1)):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(11)]


@pytest.mark.parametrize("shape", [(37, 53), (1080, 1920)], ids=["37x53", "1080x1920"])
def test_fm_jpeg_header_equals_pillow(shape):
    H, W = shape
    img = np.zeros((H, W, 3), np.uint8)
    for s in (0, 1, 2):
        for r in (0, 3):
            for q in (1, 30, 50, 75, 95, 100):
                want = pillow(img, q, s, r)
                sos = [b for m, a, b in jc.segments(want) if m == 0xDA][0]
                got = _native.jpeg_header(W, H, q, s, r)
                assert got == want[:sos], (q, s, r)
                assert got == ref.header(W, H, q, s, r)


def test_fm_jpeg_header_rejects_bad_arguments():
    L = _native.load()
    n = C.c_size_t(7)
    buf = np.zeros(1024, np.uint8)
    for args in ((0, 8, 95, 2, 0), (8, 0, 95, 2, 0), (65536, 8, 95, 2, 0), (8, 8, 0, 2, 0), (8, 8, 101, 2, 0),
                 (8, 8, 95, 3, 0), (8, 8, 95, -1, 0), (8, 8, 95, 2, -1), (8, 8, 95, 2, 65536)):
        assert L.fm_jpeg_header(*args, buf.ctypes.data, buf.size, C.byref(n)) == _native.FM_EINVAL, args
        assert n.value == 0
        with pytest.raises(_native.FMError):
            _native.jpeg_header(*args)
    assert L.fm_jpeg_header(8, 8, 95, 2, 0, buf.ctypes.data, 10, C.byref(n)) == _native.FM_EINVAL  # too small
    assert n.value == 623  # ... but the needed size is reported
    assert L.fm_jpeg_header(8, 8, 95, 2, 0, buf.ctypes.data, buf.size, C.byref(n)) == _native.FM_OK and n.value == 623


def test_encoder_settings_rejected_before_any_device_call():
    """fm_mjpeg_enc_create validates first: no GPU is needed to be refused."""
    L = _native.load()
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling=3), dict(subsampling=-1), dict(restart_interval=-1),
               dict(width=0), dict(max_frames=0)):
        a = dict(width=16, height=16, max_frames=1, quality=95, subsampling=2, restart_interval=0)
        a.update(kw)
        h = C.c_void_p()
        rc = L.fm_mjpeg_enc_create(0, a["width"], a["height"], a["max_frames"], a["quality"], a["subsampling"],
                                   a["restart_interval"], C.byref(h))
        assert rc == _native.FM_EINVAL, kw
        assert h.value and b"bad settings" in L.fm_mjpeg_enc_last_error(h)
        L.fm_mjpeg_enc_destroy(h)
        with pytest.raises(_native.FMError):
            _native.MJpegEncoder(a["width"], a["height"], a["max_frames"], 0, a["quality"], a["subsampling"],
                                 a["restart_interval"])


# --- plumbing, with a stand-in encoder ------------------------------------------------------------------------

DEVICE = {}  # "device memory" of the stand-in engine: address -> frame


class FakeEncoder:
    """MJpegEncoder's surface with Pillow behind it."""
    quality, subsampling, restart_interval = 95, 2, 0
    made = []

    def __init__(self, width=0, height=0, max_frames=1, device=0, **kw):
        self.size, self.device, self.closed, self.refuse = (width, height), device, False, False
        FakeEncoder.made.append(self)

    def _one(self, f):
        if self.refuse:
            raise _native.FMError(_native.FM_EINVAL, "refused")
        return jc.encode(np.asarray(f), quality=95, subsampling=2)

    def encode(self, frames):
        return [self._one(f) for f in frames]

    def encode_device(self, ptrs, n=None):
        return [self._one(DEVICE[p]) for p in ptrs]

    def close(self):
        self.closed = True


class DeviceOracleEngine(OracleEngine):
    """OracleEngine that also keeps the last waited batch's frames "on the device" (frame_device_ptr)."""

    def submit(self, frames):
        super().submit(frames)
        f = np.array(frames)
        self.__dict__.setdefault("_fq", []).append(f[None] if f.ndim == 4 else f)

    def wait(self):
        super().wait()
        self._cur = self._fq.pop(0)

    def frame_device_ptr(self, t, s):
        key = 0x1000 + len(DEVICE)
        DEVICE[key] = self._cur[t, s].copy()
        return key


class Cv2Stub:
    class VideoWriter:
        def __init__(self, *a):
            self.args = a

    @staticmethod
    def VideoWriter_fourcc(*c):  # noqa: N802
        return "".join(c)


def test_open_writer_routes_gpu_encode_and_keeps_every_default(tmp_path, monkeypatch):
    p = str(tmp_path / "o.avi")
    enc = FakeEncoder()
    for stub in (None, Cv2Stub):  # without and with OpenCV
        monkeypatch.setattr(videoio, "cv2", stub)
        w = videoio.open_writer(p, "MJPG", 25, (32, 24), gpu_encode=enc)
        assert type(w) is videoio.MjpegAviWriter and w.encoder is enc and not w.own_encoder
        w.release()
        assert not enc.closed  # a caller's encoder stays open
        w = videoio.open_writer(p, "MJPG", 25, (32, 24), jpeg=True, gpu_encode=enc)  # MJPEG source: pass-through wins
        assert type(w) is videoio.MjpegAviWriter and w.encoder is None
        w.release()
        for flag in (None, False):
            w = videoio.open_writer(p, "MJPG", 25, (32, 24), jpeg=True, gpu_encode=flag)
            assert type(w) is videoio.MjpegAviWriter and w.encoder is None
            w.release()
            for codec in ("MJPG", "DIB "):
                w = videoio.open_writer(p, codec, 25, (32, 24), gpu_encode=flag)
                if stub is None:
                    assert type(w) is videoio.RawAviWriter
                    w.release()
                else:
                    assert type(w) is Cv2Stub.VideoWriter and w.args == (p, codec, 25, (32, 24))
        w = videoio.open_writer(p, "DIB ", 25, (32, 24), gpu_encode=enc)  # not MJPG: the encoder is not used
        assert type(w) is (videoio.RawAviWriter if stub is None else Cv2Stub.VideoWriter)
    monkeypatch.setattr(_native, "MJpegEncoder", FakeEncoder)
    w = videoio.open_writer(p, "MJPG", 25, (32, 24), gpu_encode=True, device=3)
    assert isinstance(w.encoder, FakeEncoder) and w.own_encoder and w.encoder.size == (32, 24) and w.encoder.device == 3
    e = w.encoder
    w.release()
    assert e.closed  # the writer's own encoder goes with it


def test_avi_written_through_an_encoder_reads_back(tmp_path):
    W, H = 53, 37
    frames = [jc.image(H, W, "smooth", s) for s in range(3)]
    enc = FakeEncoder()
    p = str(tmp_path / "g.avi")
    w = videoio.MjpegAviWriter(p, 25, (W, H), encoder=enc)
    w.write(frames[0])
    DEVICE[1] = frames[1]
    w.write_device(1)
    enc.refuse = True
    w.write(frames[2])            # refused: Pillow on the host, logged
    w.write_device(1, frames[1])  # refused, host copy supplied
    with pytest.raises(_native.FMError):
        w.write_device(1)         # refused, nothing to fall back on
    w.release()
    assert (w.host_frames, w.device_frames, w.fallback_frames) == (1, 1, 2)
    h = videoio.MjpegAviWriter(str(tmp_path / "h.avi"), 25, (W, H))  # the host writer: the same file
    for f in (frames[0], frames[1], frames[2], frames[1]):
        h.write(f)
    h.release()
    assert open(p, "rb").read() == open(str(tmp_path / "h.avi"), "rb").read()
    cap = videoio.MjpegAviCapture(p, gpu_decode=False)
    assert cap.get(videoio.CAP_PROP_FRAME_COUNT) == 4
    for f in (frames[0], frames[1], frames[2], frames[1]):
        ok, got = cap.read()
        assert ok
        np.testing.assert_array_equal(got, jc.reference_decode(jc.encode(f, quality=95, subsampling=2)))
    with pytest.raises(ValueError):
        videoio.MjpegAviWriter(str(tmp_path / "n.avi"), 25, (W, H)).write_device(1)


def test_gpu_encode_flag_reaches_video_motion_and_the_writer(tmp_path, monkeypatch):
    parser = ArgumentParser()
    cli.get_args(parser)
    assert parser.parse_args(["x.avi"]).gpu_encode is None
    args = parser.parse_args(["x.avi", "--gpu-encode"])
    assert args.gpu_encode is True and cli._job_kwargs(args)["gpu_encode"] is True
    monkeypatch.setattr(_native, "MJpegEncoder", FakeEncoder)
    monkeypatch.setattr(videoio, "cv2", None)
    W, H, n = 192, 108, 40
    out = {}
    for name, flag in (("gpu", True), ("host", None)):
        eng = DeviceOracleEngine(n_streams=1, src_w=W, src_h=H, box_size=100, ksize=5, threshold=12, avg=0.1,
                                 max_batch=4)
        vm = motion.VideoMotion(filename=str(tmp_path / name), capture=videoio.SyntheticCapture(W, H, n, 0), engine=eng,
                                batch=4, box_size=100, cache_time=0.3, min_time=0.1, fps=30, threshold=12,
                                outdir=str(tmp_path), gpu_encode=flag, codec="MJPG")
        assert vm.gpu_encode is flag
        writers = []
        real = videoio.open_writer
        if flag is None:  # the comparison run: the host MJPG writer
            monkeypatch.setattr(videoio, "open_writer", lambda p, c, fps, size, **kw: writers.append(
                videoio.MjpegAviWriter(p, fps, size)) or writers[-1])
        else:
            monkeypatch.setattr(videoio, "open_writer", lambda *a, **kw: writers.append(real(*a, **kw)) or writers[-1])
        vm.find_motion()
        monkeypatch.setattr(videoio, "open_writer", real)
        out[name] = (vm.written_indices, open(vm.outfile_name, "rb").read(), writers)
    assert out["gpu"][0] == out["host"][0] and out["gpu"][0]
    assert out["gpu"][1] == out["host"][1]
    w = out["gpu"][2][0]
    assert isinstance(w.encoder, FakeEncoder) or w.encoder is None  # released: the writer closed its own encoder
    assert w.device_frames > 0 and w.host_frames > 0 and w.fallback_frames == 0
    assert w.device_frames + w.host_frames == len(out["gpu"][0])
