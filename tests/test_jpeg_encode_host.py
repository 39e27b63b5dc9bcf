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


# --- the entropy coder's inputs: what the GPU tests encode, pinned and measured here ---------------------------

_COEF = {}


def case_image(name):
    fn, q, s, restarts = jc.ENTROPY_CASES[name]
    return fn(), q, s, restarts


def case_coefficients(name):
    """ref.coefficients of an entropy case, computed once (the arrays are shared: do not write to them)."""
    if name not in _COEF:
        img, q, s, _ = case_image(name)
        _COEF[name] = ref.coefficients(img, q, s)
        _COEF[name].setflags(write=False)
    return _COEF[name]


@pytest.mark.parametrize("name", list(jc.ENTROPY_CASES))
def test_restatement_equals_pillow_on_the_entropy_cases(name):
    """What licenses reading coverage off ref.coefficients: on these images too the restatement writes Pillow's
    file, at every setting the GPU encodes them with."""
    img, q, s, restarts = case_image(name)
    H, W = img.shape[:2]
    for r in restarts:
        got = ref.header(W, H, q, s, r) + ref.entropy_code(case_coefficients(name), s, r) + b"\xff\xd9"
        assert got == pillow(img, q, s, r), r


QUALITY_SWEEP = [(q, 2) for q in (1, 10, 23, 24, 25, 49, 50, 51, 99)] + [(1, 0)]  # (quality, subsampling)


@pytest.mark.parametrize("q,s", QUALITY_SWEEP)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_restatement_equals_pillow_over_the_quality_scaling(q, s, kind):
    """jpeg_set_quality's scaling, force_baseline: quality 1 (scale 5000: every entry clamps to 255), 10 (most do),
    23 / 24 / 25 (scale 217 / 208 / 200: the last quality at which an entry clamps, and the first two without),
    49 / 50 / 51 (the formula's switch), 99 (scale 2)."""
    img = jc.image(37, 53, kind, seed=7)
    assert ref.encode(img, q, s, 0) == pillow(img, q, s, 0)


def test_quality_scaling_clamps_where_the_sweep_says():
    lq = {q: ref.quant_tables(q)[0] for q in (1, 10, 23, 24)}
    assert (lq[1] == 255).all() and 0 < (lq[10] == 255).sum() < 64
    assert (lq[23] == 255).sum() == 2 and lq[24].max() == 252  # 121 and 120 * 217 / 100 clamp, 121 * 208 / 100 does not


# (H, W, subsampling, restart intervals): a frame of more than 256 blocks gives each lane of k_enc_scan a run of
# per = ceil(blocks / 256) consecutive blocks; see tests/test_gpu_jpeg_encode.py for what each shape is for
SCAN_LAYOUT = [(128, 136, 0, (1, 5)), (50, 330, 1, (1, 7)), (120, 200, 2, (1, 2, "row", 103))]


@pytest.mark.parametrize("H,W,s,restarts", SCAN_LAYOUT, ids=lambda v: str(v).replace(" ", ""))
def test_restatement_equals_pillow_on_the_scan_layout_shapes(H, W, s, restarts):
    img = jc.image(H, W, "noise", seed=H + W)
    co = ref.coefficients(img, 90, s)
    for r in restarts:
        n = restart_mcus(W, s, r)
        assert ref.header(W, H, 90, s, n) + ref.entropy_code(co, s, n) + b"\xff\xd9" == pillow(img, 90, s, r), r


ALL_AC = {(run << 4) | size for run in range(16) for size in range(1, 11)} | {0x00, 0xF0}
# the (run, size) symbols that no 4:4:4 entropy case reaches, per table: written out, so that coverage cannot shrink
# unnoticed (a construction that reaches more of them is welcome: shorten these)
MISSING_AC = [{0x58}, {0xC9, 0xE9}]


def entropy_stats(coef):
    """Of a 4:4:4 frame's scan-order coefficients, per Huffman table slot (0: Y, 1: Cb and Cr): the AC symbols,
    the most ZRLs in a block, whether a block has coefficient 63 after a run of at least 48, the AC sizes by
    sign, the DC categories by sign (no restart intervals)."""
    st = [dict(ac=set(), zrl=0, late=False, size=set(), dc=set()) for _ in range(2)]
    for comp in range(3):
        t = st[min(comp, 1)]
        blocks = coef[comp::3].astype(np.int64)
        for d, blk in zip(np.diff(blocks[:, 0], prepend=0), blocks):
            syms = list(ref._symbols(int(d), blk))
            (_, cat), _ = syms[0]
            t["dc"].add((cat, int(np.sign(d))))
            ac = [(rs, v) for (_, rs), v in syms[1:]]
            t["ac"] |= {rs for rs, _ in ac}
            t["zrl"] = max(t["zrl"], sum(rs == 0xF0 for rs, _ in ac))
            t["size"] |= {(rs & 15, int(np.sign(v))) for rs, v in ac if rs & 15}
            nz = np.nonzero(blk[1:63])[0]
            t["late"] |= bool(blk[63]) and (len(nz) == 0 or nz[-1] + 1 <= 63 - 49)
    return st


def test_entropy_cases_reach_the_whole_of_both_tables(capsys):
    """Computed from the reference alone (ref.coefficients, equal to Pillow's on these images by the test above):
    what the GPU encoder is asked to write, it is asked to write for nearly every symbol."""
    total = [dict(ac=set(), zrl=0, late=False, size=set(), dc=set()) for _ in range(2)]
    for name in jc.COVERAGE_CASES:
        for t, s in zip(total, entropy_stats(case_coefficients(name))):
            t["ac"] |= s["ac"]
            t["size"] |= s["size"]
            t["dc"] |= s["dc"]
            t["zrl"] = max(t["zrl"], s["zrl"])
            t["late"] |= s["late"]
    with capsys.disabled():
        for slot, t in enumerate(total):
            print(f"\n{'luma' if slot == 0 else 'chroma'} tables: {len(t['ac'])} of {len(ALL_AC)} AC symbols, missing "
                  f"{sorted(hex(x) for x in ALL_AC - t['ac'])}; up to {t['zrl']} ZRLs in a block; {len(t['size'])} of 20 "
                  f"signed AC sizes; {len(t['dc'])} of 23 signed DC categories", end="")
        print()
    for slot, t in enumerate(total):
        assert t["ac"] <= ALL_AC
        assert len(t["ac"]) >= 158, slot
        assert ALL_AC - t["ac"] == MISSING_AC[slot], slot
        assert t["zrl"] == 3, slot
        assert t["late"], slot
        assert t["size"] == {(n, sg) for n in range(1, 11) for sg in (1, -1)}, slot
        assert t["dc"] == {(0, 0)} | {(n, sg) for n in range(1, 12) for sg in (1, -1)}, slot


def test_three_zrls_occur_in_one_sweep_image_of_each_table():
    """... so that encoding the sweep images one by one (as the GPU tests do) meets the third round of the ZRL loop."""
    for slot, nm in ((0, "luma"), (1, "chroma")):
        assert any(entropy_stats(case_coefficients(f"sweep_{nm}_q{q}"))[slot]["zrl"] == 3 for q in jc.SWEEP_QUALITIES)


# --- the stuffing kernels' seams: conditions on Pillow's bytes ------------------------------------------------------

@pytest.mark.parametrize("seed,restart,conditions", jc.SEAM_CASES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_seam_frames_hold_their_conditions(seed, restart, conditions):
    """If the installed libjpeg ever writes other bytes for these seeds, this fails: search again (seeds 0..399 at
    restart intervals 0, 1, 2 held every condition) and replace jc.SEAM_CASES."""
    img = jc.seam_frame(seed)
    data = pillow(img, 100, 0, restart)
    scan = jc.scan_of(data)
    un, ffs = jc.unstuffed_data_ff(scan)
    assert len(un) + len(ffs) == len(scan) and un.replace(b"\xff", b"\xff\x00").count(b"\xff\x00") >= len(ffs)
    assert -(-len(un) // jc.SEAM_TILE) == 7
    assert conditions <= jc.seam_conditions(data)
    if "pair" in conditions:
        assert restart in (1, 2)
    assert ref.encode(img, 100, 0, restart) == data


def test_seam_cases_cover_every_condition():
    assert set().union(*(c for _, _, c in jc.SEAM_CASES)) == {"pair", "ones_rst", "ones_eoi", "tile_end", "tile_ffff"}


def test_short_streams_are_as_short_as_the_gpu_tests_say():
    """The streams put between long ones in one call.  A constant frame of the seam frames' size cannot be shorter
    than a lane's 16 bytes (288 blocks of at least 4 bits are 144 bytes): it is shorter than a tile's first 11
    lanes, and seven-tile frames surround it.  A constant 32 x 16 frame is shorter than one lane; the frames around
    it (black and white noise, the most bytes a block takes here) stay inside one tile."""
    H, W = jc.SEAM_SHAPE
    assert len(jc.scan_of(pillow(jc.constant(H, W), 100, 0, 0))) == 168
    H, W = jc.SHORT_SHAPE
    for r in (0, 1):
        n = len(jc.scan_of(pillow(jc.constant(H, W), 100, 0, r)))
        assert n < 16 if r == 0 else n < 16 + 7 * 2 + 8  # seven RSTn markers and their padding
    assert all(2048 < len(jc.scan_of(pillow(jc.binary_noise(H, W, s), 100, 0, 0))) < jc.SEAM_TILE for s in (0, 1))
    for f in (jc.binary_noise(H, W, 0), jc.binary_noise(H, W, 1), jc.constant(H, W)):
        assert all(ref.encode(f, 100, 0, r) == pillow(f, 100, 0, r) for r in (0, 1))


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


def test_encoder_refuses_frames_of_more_than_2_20_blocks_before_any_device_call():
    """8192 x 8192 at 4:4:4 is 3 * 2^20 blocks: a frame's bit offsets are 32-bit, so FM_ENOTSUP, with a message."""
    L = _native.load()
    h = C.c_void_p()
    assert L.fm_mjpeg_enc_create(0, 8192, 8192, 1, 95, 0, 0, C.byref(h)) == _native.FM_ENOTSUP
    assert h.value and b"more than 2^20 blocks" in L.fm_mjpeg_enc_last_error(h)
    L.fm_mjpeg_enc_destroy(h)
    with pytest.raises(_native.FMError) as e:
        _native.MJpegEncoder(8192, 8192, 1, 0, 95, 0, 0)
    assert e.value.code == _native.FM_ENOTSUP


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
