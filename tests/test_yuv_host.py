"""YUV input on a machine without a GPU: the conversion's known answers, the host restatements against each
other, the host-only parts of the C ABI (fm_yuv_frame_bytes, argument validation), YUV AVI files, and the
feeder's YUV mode on the oracle-backed stand-in engine.  The GPU conversion itself is in test_gpu_yuv.py.
"""
import ctypes as C

import numpy as np
import pytest

import yuv_ref
from fake_engine import OracleEngine
from find_motion_amd import _native, videoio
from find_motion_amd._native import FM_EINVAL, FM_OK, FMYuvLayout
from find_motion_amd.feeder import BatchFeeder

FORMATS = yuv_ref.FORMATS
SIZES = [(2, 2), (6, 4), (34, 18)]


# --- the formula ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("yuv,bgr", yuv_ref.KAT)
def test_known_answers_per_pixel(yuv, bgr):
    assert yuv_ref.pixel(*yuv) == bgr


@pytest.mark.parametrize("fmt", FORMATS)
def test_known_answers_through_both_restatements(fmt):
    """Every KAT triple as a uniform 2 x 2 frame in each layout: yuv_ref and videoio.yuv_to_bgr give its BGR."""
    for (Y, U, V), bgr in yuv_ref.KAT:
        buf = np.zeros(yuv_ref.frame_bytes(2, 2, fmt), np.uint8)
        for y in range(2):
            for x in range(2):
                yuv_ref.plant(buf, 2, 2, fmt, x, y, (Y, U, V))
        want = np.broadcast_to(np.array(bgr, np.uint8), (2, 2, 3))
        np.testing.assert_array_equal(yuv_ref.yuv_ref(buf, 2, 2, fmt), want, err_msg=f"yuv_ref {fmt} {(Y, U, V)}")
        np.testing.assert_array_equal(videoio.yuv_to_bgr(buf, 2, 2, fmt), want, err_msg=f"videoio {fmt} {(Y, U, V)}")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", SIZES)
def test_vectorised_equals_per_pixel_on_random_bytes(fmt, w, h):
    rng = np.random.default_rng(w * 131 + h + FORMATS.index(fmt))
    for _ in range(3):
        buf = rng.integers(0, 256, yuv_ref.frame_bytes(w, h, fmt), dtype=np.uint8)
        np.testing.assert_array_equal(videoio.yuv_to_bgr(buf, w, h, fmt), yuv_ref.yuv_ref(buf, w, h, fmt))
        np.testing.assert_array_equal(videoio.yuv_to_bgr(buf.tobytes(), w, h, fmt), yuv_ref.yuv_ref(buf, w, h, fmt))


def test_chroma_is_replicated_not_interpolated():
    """One 2 x 2 group with its own chroma beside neutral groups: only its four pixels take the colour."""
    w, h = 6, 4
    for fmt in FORMATS:
        buf = np.full(yuv_ref.frame_bytes(w, h, fmt), 128, np.uint8)
        yuv_ref.plant(buf, w, h, fmt, 2, 2, (128, 240, 16))
        out = videoio.yuv_to_bgr(buf, w, h, fmt)
        grey = (out == 130).all(axis=2)
        rows = (2, 3) if fmt in yuv_ref.PLANAR else (2,)
        want = np.ones((h, w), bool)
        for r in rows:
            want[r, 2:4] = False
        np.testing.assert_array_equal(grey, want, err_msg=fmt)
        np.testing.assert_array_equal(out, yuv_ref.yuv_ref(buf, w, h, fmt))


def test_yuv_to_bgr_refuses_bad_input():
    with pytest.raises(ValueError):
        videoio.yuv_to_bgr(bytes(10), 3, 2, "YUY2")
    with pytest.raises(ValueError):
        videoio.yuv_to_bgr(bytes(10), 2, 3, "NV12")
    with pytest.raises(ValueError):
        videoio.yuv_to_bgr(bytes(5), 2, 2, "NV12")
    with pytest.raises(ValueError):
        videoio.yuv_to_bgr(bytes(6), 2, 2, "P010")


def test_optional_cv2_cross_check():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(5)
    w, h = 34, 18
    codes = {"NV12": cv2.COLOR_YUV2BGR_NV12, "I420": cv2.COLOR_YUV2BGR_I420, "YUY2": cv2.COLOR_YUV2BGR_YUY2,
             "UYVY": cv2.COLOR_YUV2BGR_UYVY}
    for fmt in FORMATS:
        buf = rng.integers(0, 256, yuv_ref.frame_bytes(w, h, fmt), dtype=np.uint8)
        src = buf.reshape(h * 3 // 2, w) if fmt in yuv_ref.PLANAR else buf.reshape(h, w, 2)
        np.testing.assert_array_equal(cv2.cvtColor(src, codes[fmt]), yuv_ref.yuv_ref(buf, w, h, fmt))


# --- the C ABI without a device ---------------------------------------------------------------------------

def _frame_bytes(w, h, fmt, pitch=0, coff=0, stride=0):
    L = _native.load()
    n = C.c_size_t(12345)
    lay = FMYuvLayout(fmt, pitch, coff, stride)
    return L.fm_yuv_frame_bytes(w, h, C.byref(lay), C.byref(n)), n.value


def test_library_exports_the_yuv_entry_points():
    L = _native.load()
    for name in ("fm_yuv_frame_bytes", "fm_submit_yuv", "fm_submit_yuv_list"):
        assert hasattr(L, name), name
        assert name in _native.EXPORTED
    assert L.fm_abi_version() == 1


def test_frame_bytes_tight_and_pitched():
    w, h = 34, 18
    assert _frame_bytes(w, h, _native.YUV_NV12) == (FM_OK, w * h * 3 // 2)
    assert _frame_bytes(w, h, _native.YUV_I420) == (FM_OK, w * h * 3 // 2)
    assert _frame_bytes(w, h, _native.YUV_YUY2) == (FM_OK, w * h * 2)
    assert _frame_bytes(w, h, _native.YUV_UYVY) == (FM_OK, w * h * 2)
    assert _frame_bytes(1920, 1080, _native.YUV_NV12) == (FM_OK, 3110400)
    # pitch 36, chroma 8 bytes past the luma plane: NV12 9 rows of 36, I420 two planes of 9 rows of 18
    assert _frame_bytes(w, h, _native.YUV_NV12, 36, 36 * 18 + 8) == (FM_OK, 656 + 36 * 9)
    assert _frame_bytes(w, h, _native.YUV_I420, 36, 36 * 18 + 8) == (FM_OK, 656 + 18 * 18)
    assert _frame_bytes(w, h, _native.YUV_NV12, 35) == (FM_OK, 35 * 18 + 35 * 9)  # an odd pitch is fine for NV12
    assert _frame_bytes(w, h, _native.YUV_YUY2, 72) == (FM_OK, 72 * 18)
    assert _frame_bytes(w, h, _native.YUV_UYVY, 72, 0, 5000) == (FM_OK, 72 * 18)  # the extent, not the stride
    assert _frame_bytes(w, h, _native.YUV_NV12, 0, 0, w * h * 3 // 2) == (FM_OK, w * h * 3 // 2)
    assert _frame_bytes(w, 17, _native.YUV_YUY2) == (FM_OK, w * 17 * 2)  # odd height: fine for 4:2:2
    for fmt in FORMATS:  # the wrapper, and the reference's own layout arithmetic
        for kw in (dict(), dict(pitch=40 if fmt in yuv_ref.PLANAR else 76)):
            assert _native.yuv_frame_bytes(w, h, fmt, **kw) == yuv_ref.frame_bytes(w, h, fmt, **kw)
        if fmt in yuv_ref.PLANAR:
            assert _native.yuv_frame_bytes(w, h, fmt, 36, 700) == yuv_ref.frame_bytes(w, h, fmt, 36, 700)


@pytest.mark.parametrize("args", [
    (34, 18, 4), (34, 18, -1),                              # unknown format
    (33, 18, 0), (33, 18, 1), (33, 18, 2), (33, 18, 3),     # odd width
    (34, 17, 0), (34, 17, 1),                               # odd height, 4:2:0
    (0, 18, 0), (34, 0, 2), (-2, 18, 2),                    # no frame
    (34, 18, 0, 33), (34, 18, 1, 32), (34, 18, 2, 67), (34, 18, 3, 66), (34, 18, 0, -1),   # pitch below tight
    (34, 18, 1, 35), (34, 18, 1, 37),                       # odd pitch, I420
    (34, 18, 0, 0, 34 * 18 - 1), (34, 18, 1, 36, 36 * 18 - 2), (34, 18, 0, 0, 1), (34, 18, 0, 0, -4),  # chroma in luma
    (34, 18, 0, 0, 0, 917), (34, 18, 1, 0, 0, 917), (34, 18, 2, 0, 0, 1223), (34, 18, 0, 36, 656, 979),  # stride
])
def test_frame_bytes_refuses(args):
    rc, n = _frame_bytes(*args)
    assert rc == FM_EINVAL and n == 0
    assert _native.load().fm_last_error(None)


def test_frame_bytes_null_arguments():
    L = _native.load()
    n = C.c_size_t(7)
    assert L.fm_yuv_frame_bytes(34, 18, None, C.byref(n)) == FM_EINVAL and n.value == 0
    lay = FMYuvLayout(0, 0, 0, 0)
    assert L.fm_yuv_frame_bytes(34, 18, C.byref(lay), None) == FM_EINVAL
    with pytest.raises(_native.FMError):
        _native.yuv_frame_bytes(33, 18, "NV12")
    with pytest.raises(ValueError):
        _native.yuv_frame_bytes(34, 18, "P010")


def test_submit_yuv_null_context_fails_without_a_device():
    L = _native.load()
    lay = FMYuvLayout(0, 0, 0, 0)
    buf = np.zeros(64, np.uint8)
    ptrs = (C.c_void_p * 1)(buf.ctypes.data)
    assert L.fm_submit_yuv(None, buf.ctypes.data, 1, C.byref(lay), 0) == FM_EINVAL
    assert L.fm_submit_yuv(None, None, 1, None, 1) == FM_EINVAL
    assert L.fm_submit_yuv_list(None, C.cast(ptrs, C.c_void_p), 1, C.byref(lay)) == FM_EINVAL
    assert L.fm_submit_yuv_list(None, None, 1, None) == FM_EINVAL


# --- YUV AVI files ------------------------------------------------------------------------------------------

def _write_yuv_avi(path, fmt, w, h, n, seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, yuv_ref.frame_bytes(w, h, fmt), dtype=np.uint8).tobytes() for _ in range(n)]
    wr = videoio.RawAviWriter(str(path), 25, (w, h), fourcc=fmt)
    for f in frames:
        wr.write(f)
    wr.release()
    return frames


@pytest.mark.parametrize("fmt", FORMATS)
def test_yuv_avi_round_trip(tmp_path, fmt):
    w, h, n = 34, 18, 4
    path = tmp_path / f"{fmt}.avi"
    frames = _write_yuv_avi(path, fmt, w, h, n, 11)
    cap = videoio.open_capture(str(path)) if videoio.cv2 is None else videoio.RawAviCapture(str(path))
    assert isinstance(cap, videoio.RawAviCapture) and cap.isOpened()
    assert cap.yuv_format == fmt
    assert (cap.get(videoio.CAP_PROP_FRAME_WIDTH), cap.get(videoio.CAP_PROP_FRAME_HEIGHT)) == (w, h)
    assert cap.get(videoio.CAP_PROP_FRAME_COUNT) == n and cap.get(videoio.CAP_PROP_FPS) == 25
    assert bytes(cap.peek()) == frames[0]
    for i in range(2):
        ok, fr = cap.read_yuv()
        assert ok and bytes(fr) == frames[i]
    assert bytes(cap.peek()) == frames[2]
    for i in range(2, n):  # read() goes on where read_yuv() stopped, and converts
        ok, bgr = cap.read()
        assert ok and bgr.shape == (h, w, 3) and bgr.dtype == np.uint8
        np.testing.assert_array_equal(bgr, yuv_ref.yuv_ref(frames[i], w, h, fmt))
    assert cap.peek() is None and cap.read_yuv() == (False, None) and cap.read() == (False, None)
    cap.release()


@pytest.mark.parametrize("alias,fmt", [(b"IYUV", "I420"), (b"YUYV", "YUY2")])
def test_yuv_avi_fourcc_aliases(tmp_path, alias, fmt):
    path = tmp_path / "a.avi"
    frames = _write_yuv_avi(path, fmt, 6, 4, 2, 3)
    data = path.read_bytes()
    head = data[:512].replace(fmt.encode(), alias)
    path.write_bytes(head + data[512:])
    cap = videoio.RawAviCapture(str(path))
    assert cap.isOpened() and cap.yuv_format == fmt
    ok, fr = cap.read_yuv()
    assert ok and bytes(fr) == frames[0]


def test_yuv_writer_refuses_wrong_sizes_and_fourccs(tmp_path):
    with pytest.raises(ValueError):
        videoio.RawAviWriter(str(tmp_path / "x.avi"), 25, (6, 4), fourcc="P010")
    wr = videoio.RawAviWriter(str(tmp_path / "y.avi"), 25, (6, 4), fourcc="NV12")
    with pytest.raises(ValueError):
        wr.write(bytes(35))
    wr.release()


def test_bgr_avi_reads_as_before(tmp_path):
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, (3, 9, 7, 3), dtype=np.uint8)  # 21-byte rows: padded to 24
    path = str(tmp_path / "bgr.avi")
    wr = videoio.RawAviWriter(path, 30, (7, 9))
    for f in frames:
        wr.write(f)
    wr.release()
    cap = videoio.RawAviCapture(path)
    assert cap.isOpened() and cap.yuv_format is None
    assert not hasattr(cap, "read_yuv") and not hasattr(cap, "peek")
    for f in frames:
        ok, got = cap.read()
        assert ok
        np.testing.assert_array_equal(got, f)
    assert cap.read() == (False, None)


# --- the feeder's YUV mode --------------------------------------------------------------------------------

class YuvOracleEngine(OracleEngine):
    """The oracle-backed stand-in with the engine's YUV surface: converts on the host, records what it was given."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.yuv_submits = []

    def host_buffer_yuv(self, n_frames, fmt, pitch=0, chroma_offset=0, frame_stride=0):
        H, W = self.src_shape[:2]
        return np.zeros((n_frames, self.n_streams, yuv_ref.frame_bytes(W, H, fmt)), np.uint8)

    def submit_yuv(self, frames, fmt, **kw):
        H, W = self.src_shape[:2]
        f = np.array(frames)
        self.yuv_submits.append((fmt, f))
        self.submit(np.stack([[videoio.yuv_to_bgr(f[t, s], W, H, fmt) for s in range(f.shape[1])]
                              for t in range(f.shape[0])]))


def _engine(S, W, H, T, cls=YuvOracleEngine):
    return cls(n_streams=S, src_w=W, src_h=H, box_size=W, ksize=3, threshold=12, avg=0.1, max_batch=T)


def test_feeder_selects_yuv_mode_and_pads_ended_streams(tmp_path, oracle_lib):
    w, h, T = 34, 18, 2
    a = _write_yuv_avi(tmp_path / "a.avi", "NV12", w, h, 5, 21)
    b = _write_yuv_avi(tmp_path / "b.avi", "NV12", w, h, 3, 22)
    caps = [videoio.RawAviCapture(str(tmp_path / "a.avi")), videoio.RawAviCapture(str(tmp_path / "b.avi"))]
    eng = _engine(2, w, h, T)
    feeder = BatchFeeder(eng, caps, T)
    assert feeder.yuv == "NV12" and not feeder.jpeg
    seen = [[], []]
    sizes = []
    for batch in feeder:
        assert batch.yuv == "NV12" and batch.jpegs is None
        sizes.append(batch.T)
        for s in range(2):
            seen[s] += [bytes(f) for f in batch.frames[s]]
    assert sizes == [2, 2, 1]
    assert seen == [a, b]  # every stream's own frames, in order, nothing invented
    assert eng.submits == 3 and len(eng.yuv_submits) == 3
    want = [[(a[0], b[0]), (a[1], b[1])], [(a[2], b[2]), (a[3], b[2])], [(a[4], b[2])]]  # b padded with its last
    for (fmt, got), rows in zip(eng.yuv_submits, want):
        assert fmt == "NV12" and got.shape == (len(rows), 2, yuv_ref.frame_bytes(w, h, "NV12"))
        for t, row in enumerate(rows):
            for s in range(2):
                assert got[t, s].tobytes() == row[s], (t, s)


def test_feeder_keeps_bgr_mode_for_mixed_or_plain_sources(tmp_path, oracle_lib):
    w, h, T = 34, 18, 2
    _write_yuv_avi(tmp_path / "a.avi", "NV12", w, h, 2, 1)
    _write_yuv_avi(tmp_path / "b.avi", "YUY2", w, h, 2, 2)
    # two formats: the captures convert on the host
    caps = [videoio.RawAviCapture(str(tmp_path / "a.avi")), videoio.RawAviCapture(str(tmp_path / "b.avi"))]
    eng = _engine(2, w, h, T)
    feeder = BatchFeeder(eng, caps, T)
    assert feeder.yuv is None
    assert [b.T for b in feeder] == [2] and not eng.yuv_submits and eng.submits == 1
    with pytest.raises(ValueError):
        BatchFeeder(eng, [videoio.ArrayCapture(np.zeros((1, h, w, 3), np.uint8))] * 2, T, yuv=True)
    # an engine without the YUV surface: the same file through read()
    plain = _engine(1, w, h, T, cls=OracleEngine)
    feeder = BatchFeeder(plain, [videoio.RawAviCapture(str(tmp_path / "a.avi"))], T)
    assert feeder.yuv is None
    assert [b.T for b in feeder] == [2]


def test_video_motion_reads_raw_lazily_from_a_yuv_file(tmp_path, oracle_lib):
    """The drop-in on the stand-in engine: frames of a YUV file carry their bytes, and raw -- fetched only on
    access -- is the converted frame, from the engine while the batch is current and from the host afterwards."""
    from find_motion_amd import motion

    w, h, n = 34, 18, 5
    frames = _write_yuv_avi(tmp_path / "v.avi", "UYVY", w, h, n, 9)

    class Eng(YuvOracleEngine):
        reads = 0

        def read_frame(self, t, s):
            Eng.reads += 1
            fmt, f = self.yuv_submits[-len(self._queue) - 1]
            return videoio.yuv_to_bgr(f[t, s], w, h, fmt)

    vm = motion.VideoMotion(filename=str(tmp_path / "v.avi"), outdir=str(tmp_path), box_size=w, batch=2,
                            capture=videoio.RawAviCapture(str(tmp_path / "v.avi")), engine=_engine(1, w, h, 2, cls=Eng))
    got = []
    while vm.read():
        vf = vm.current_frame
        assert vf.yuv is not None and vf._raw is None
        got.append(vf)
    assert len(got) == n
    for i, vf in enumerate(got):  # every batch but the last is gone: converted on the host
        np.testing.assert_array_equal(vf.raw, yuv_ref.yuv_ref(frames[i], w, h, "UYVY"))
    assert Eng.reads == 1  # the last batch (one frame) was still current
    vm.cleanup()
