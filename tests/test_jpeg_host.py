"""Decode side, CPU: the restatement oracle/jpeg.py against Pillow's libjpeg-turbo.

libjpeg-turbo's default decode is what cv2.imdecode and OpenCV's built-in MJPEG reader (CAP_OPENCV_MJPEG) run
on MJPEG frames.  It is NOT what cv2.VideoCapture.read (fm.py:413, 497-506) runs by default: stock OpenCV builds
open AVI files with the FFmpeg backend (libavcodec IDCT, swscale), whose parity is unpinned here.
Pillow bundles libjpeg-turbo, so the restatement of jdhuff / jidctint (islow) / jdsample (fancy upsampling) / jdcolor
is pinned bit for bit here, on every sampling layout, odd sizes (partial MCUs, one-column chroma), restart
intervals and grayscale.  The committed fixtures (tests/golden/jpeg_cases.npz, tests/golden/make_golden_jpeg.py)
keep the same check on a machine whose Pillow differs."""
import os

import numpy as np
import pytest

from oracle import jpeg
from jpeg_cases import (ENCODINGS, REFUSED, RGB_REFUSED, STREAMS, SUBSAMPLINGS, Image, as_jfif, busy_noise, checkerboard, constant,
                        encode, fill_before_markers, image, luma_dc_differences, reference_decode,
                        restart_interval_lengths, segments, stream_reference, strip_dht)

pytestmark = pytest.mark.skipif(Image is None, reason="Pillow not importable")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")


def _bgr(a):
    return np.repeat(a[..., None], 3, axis=2) if a.ndim == 2 else a


@pytest.mark.parametrize("name,kw", ENCODINGS)
@pytest.mark.parametrize("H,W", [(16, 16), (37, 53), (8, 9), (24, 40), (61, 33), (9, 2), (5, 4), (3, 7), (1, 1)])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_restatement_equals_libjpeg(name, kw, H, W, kind):
    data = encode(image(H, W, kind), **kw)
    assert np.array_equal(_bgr(jpeg.decode(data)), reference_decode(data))


@pytest.mark.parametrize("H,W", [(16, 16), (37, 53)])
def test_grayscale(H, W):
    data = encode(image(H, W, "smooth")[..., 1], quality=75)
    assert np.array_equal(_bgr(jpeg.decode(data)), reference_decode(data))


def test_parse_reports_layout_and_restart_interval():
    j = jpeg.parse(encode(image(32, 48, "smooth"), quality=80, restart_marker_blocks=3))
    assert (j["frame"]["H"], j["frame"]["W"]) == (32, 48)
    assert [(c["h"], c["v"]) for c in j["frame"]["comps"]] == [(2, 2), (1, 1), (1, 1)]
    assert j["dri"] > 0
    assert set(j["ht"]) == {(0, 0), (1, 0), (0, 1), (1, 1)}


def test_progressive_is_refused():
    data = encode(image(16, 16, "smooth"), quality=75, progressive=True)
    with pytest.raises(jpeg.JpegError):
        jpeg.parse(data)


def test_golden_fixtures():
    z = np.load(GOLDEN)
    n = int(z["n"])
    for i in range(n):
        data = z[f"jpeg{i}"].tobytes()
        assert np.array_equal(_bgr(jpeg.decode(data)), z[f"bgr{i}"]), i


def test_mjpeg_avi_round_trip(tmp_path):
    """videoio.MjpegAviWriter -> MjpegAviCapture: chunk bytes, count, size and rate survive; open_capture
    picks the MJPEG reader (the GPU decode path) and open_writer(jpeg=True) the passthrough writer."""
    from find_motion_amd import videoio
    W, H = 72, 40
    jp = [encode(image(H, W, "smooth", seed=s), quality=70 + s) for s in range(5)]  # odd and even lengths
    p = str(tmp_path / "m.avi")
    w = videoio.open_writer(p, "MJPG", 25, (W, H), jpeg=True)
    assert isinstance(w, videoio.MjpegAviWriter)
    for j in jp[:4]:
        w.write_jpeg(j)
    w.write(reference_decode(jp[4]))  # a BGR frame, Pillow-encoded
    w.release()
    assert videoio.is_mjpeg_avi(p) and not videoio.is_mjpeg_avi(str(tmp_path / "none.avi"))
    cap = videoio.open_capture(p) if videoio.cv2 is None else videoio.open_capture(p, gpu_decode=True)
    assert isinstance(cap, videoio.MjpegAviCapture)
    assert (cap.get(videoio.CAP_PROP_FRAME_COUNT), cap.get(videoio.CAP_PROP_FRAME_WIDTH),
            cap.get(videoio.CAP_PROP_FRAME_HEIGHT)) == (5, W, H)
    assert abs(cap.fps - 25) < 0.01
    got = []
    while True:
        ok, j = cap.read_jpeg()
        if not ok:
            break
        got.append(j)
    assert got[:4] == jp[:4] and len(got) == 5
    assert reference_decode(got[4]).shape == (H, W, 3)
    cap.release()
    raw = str(tmp_path / "r.avi")
    videoio.RawAviWriter(raw, 25, (W, H)).release()
    assert not videoio.is_mjpeg_avi(raw)
    assert not videoio.MjpegAviCapture(raw).isOpened()  # cv2-like: a capture that failed to open


def test_mjpeg_avi_opendml_continuation(tmp_path):
    """Frames in an OpenDML 'RIFF AVIX' continuation (files past 1 GB) are read after the first RIFF's."""
    import struct

    from find_motion_amd import videoio
    W, H = 32, 16
    jp = [encode(image(H, W, "smooth", seed=s), quality=80) for s in range(5)]
    p = str(tmp_path / "big.avi")
    w = videoio.MjpegAviWriter(p, 30, (W, H))
    for j in jp[:3]:
        w.write_jpeg(j)
    w.release()
    movi = b"movi" + b"".join(b"00dc" + struct.pack("<I", len(j)) + j + (b"\0" if len(j) & 1 else b"") for j in jp[3:])
    avix = b"AVIX" + b"LIST" + struct.pack("<I", len(movi)) + movi
    with open(p, "ab") as f:
        f.write(b"RIFF" + struct.pack("<I", len(avix)) + avix)
    cap = videoio.MjpegAviCapture(p)
    got = []
    while True:
        ok, j = cap.read_jpeg()
        if not ok:
            break
        got.append(j)
    assert got == jp


def test_jpeg_layout():
    from find_motion_amd import videoio
    assert videoio.jpeg_layout(encode(image(24, 40, "smooth"), quality=75)) == (24, 40, ((2, 2), (1, 1), (1, 1)))
    assert videoio.jpeg_layout(encode(image(24, 40, "smooth"), quality=75, subsampling=1))[2] == ((2, 1), (1, 1), (1, 1))
    assert videoio.jpeg_layout(encode(image(24, 40, "smooth")[..., 0], quality=75)) == (24, 40, ((1, 1),))
    cap = videoio.JpegListCapture([encode(image(24, 40, "smooth"), quality=75)])
    assert cap.peek_jpeg() is not None and cap.read_jpeg()[0] and cap.peek_jpeg() is None


def test_standard_huffman_tables_are_the_ones_libjpeg_encodes_with():
    """oracle STD_HUFF (T.81 Annex K.3, libjpeg-turbo jstdhuff.c) == the DHT Pillow writes without optimize."""
    j = jpeg.parse(encode(image(16, 16, "noise"), quality=75))
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        bits, vals = j["ht"][key]
        assert (list(bits), list(vals)) == (list(jpeg.STD_HUFF[key][0]), list(jpeg.STD_HUFF[key][1])), key
    assert [len(jpeg.STD_HUFF[k][1]) for k in ((0, 0), (0, 1), (1, 0), (1, 1))] == [12, 12, 162, 162]


@pytest.mark.parametrize("name,kw", ENCODINGS[:5])
def test_frame_without_dht_decodes_with_the_standard_tables(name, kw):
    """AVI1 Motion-JPEG: no DHT segment; libjpeg-turbo (std_huff_tables) and the restatement supply Annex K."""
    data = encode(image(37, 53, "smooth"), **kw)
    bare = strip_dht(data)
    assert not any(m == 0xC4 for m, _, _ in segments(bare)) and len(bare) < len(data)
    want = reference_decode(data)
    assert np.array_equal(reference_decode(bare), want)  # libjpeg-turbo itself accepts the bare frame
    assert np.array_equal(_bgr(jpeg.decode(bare)), want)


@pytest.mark.parametrize("n", [1, 3])
def test_fill_bytes_before_restart_markers(n):
    """0xFF fill bytes before RSTn / EOI (T.81 B.1.1.2) are skipped, as libjpeg does."""
    data = encode(image(40, 56, "noise"), quality=80, restart_marker_blocks=2)
    filled = fill_before_markers(data, n)
    assert len(filled) > len(data)
    want = reference_decode(data)
    assert np.array_equal(reference_decode(filled), want)
    assert np.array_equal(_bgr(jpeg.decode(filled)), want)


def test_jpeg_gpu_supported_layouts():
    from find_motion_amd import videoio
    ok = [encode(image(24, 40, "smooth"), quality=75, subsampling=s) for s in (0, 1, 2)]
    ok.append(encode(image(24, 40, "smooth")[..., 0], quality=75))
    ok.append(strip_dht(ok[0]))
    assert all(videoio.jpeg_gpu_supported(j) for j in ok)
    assert not videoio.jpeg_gpu_supported(encode(image(24, 40, "smooth"), quality=75, progressive=True))
    assert not videoio.jpeg_gpu_supported(b"not a jpeg")
    # libjpeg's colour-space rule and T.81 B.2.3: RGB-coded planes and a scan out of the frame's order go to
    # the host; every other stream shape of the list is the GPU decoder's
    for name in RGB_REFUSED + ("sos_ids_swapped", "cmyk"):
        assert not videoio.jpeg_gpu_supported(REFUSED[name](24, 40)), name
    for name, make in STREAMS.items():
        assert videoio.jpeg_gpu_supported(make(24, 40)[0]), name


STREAM_SHAPES = [(37, 53), (16, 16)]


@pytest.mark.parametrize("H,W", STREAM_SHAPES)
@pytest.mark.parametrize("name", list(STREAMS))
def test_streams_pillow_does_not_write(name, H, W):
    """Table ids, merged segments, 16-bit tables, metadata, trailing bytes, a missing EOI, a gray frame's
    sampling byte: the restatement equals libjpeg, and a patch that keeps the meaning keeps libjpeg's pixels
    (a broken helper fails here as a helper)."""
    data, base = STREAMS[name](H, W)
    want = stream_reference(name, data)
    if base is not None:
        assert data != base and np.array_equal(want, reference_decode(base))
    assert np.array_equal(_bgr(jpeg.decode(data)), want)


def test_stream_patches_are_what_their_names_say():
    H, W = 37, 53
    mk = lambda name: STREAMS[name](H, W)[0]  # noqa: E731
    seg = lambda d, m: [d[a + 4:b] for k, a, b in segments(d) if k == m]  # noqa: E731
    d = mk("dqt16_sof1")
    assert seg(d, 0xC1) and not seg(d, 0xC0) and all(p[0] >> 4 == 1 and len(p) == 129 for p in seg(d, 0xDB))
    assert int(jpeg.parse(d)["qt"][1].max()) == 1000
    j = jpeg.parse(mk("three_qtables"))
    assert [c["tq"] for c in j["frame"]["comps"]] == [0, 1, 2] and not np.array_equal(j["qt"][1], j["qt"][2])
    j = jpeg.parse(mk("quant_ids_2_3"))
    assert [c["tq"] for c in j["frame"]["comps"]] == [2, 3, 3] and set(j["qt"]) == {2, 3}
    for name, ids in (("huff_ids_2_3", (2, 3)), ("huff_ids_3_2", (3, 2))):
        d = mk(name)
        assert [p[0] & 15 for p in seg(d, 0xC4)] == [ids[0], ids[0], ids[1], ids[1]]
        assert [(td, ta) for _, td, ta in jpeg.parse(d)["scan"]["sel"]] == [(ids[0],) * 2, (ids[1],) * 2, (ids[1],) * 2]
    assert len(seg(mk("merged_dht"), 0xC4)) == 1 and len(seg(STREAMS["merged_dht"](H, W)[1], 0xC4)) == 4
    std = [(list(bits), list(vals)) for bits, vals in jpeg.STD_HUFF.values()]
    for name in ("merged_dht", "huff_ids_3_2"):  # four tables of the stream's own, none of them a standard one
        own = [t for k, t in jpeg.parse(mk(name))["ht"].items() if t is not jpeg.STD_HUFF.get(k)]
        assert len(own) == 4 and all((list(bits), list(vals)) not in std for bits, vals in own)
    assert [len(p) for p in seg(mk("merged_dqt"), 0xDB)] == [130]
    assert [len(p) for p in seg(mk("merged_dqt16"), 0xDB)] == [258]
    for name, jfif in (("ids_012_jfif", True), ("ids_012_no_jfif", False)):
        d = mk(name)
        assert [c["id"] for c in jpeg.parse(d)["frame"]["comps"]] == [0, 1, 2] and bool(seg(d, 0xE0)) == jfif
    d = mk("adobe1_no_jfif")
    assert not seg(d, 0xE0) and seg(d, 0xEE)[0][:5] == b"Adobe" and seg(d, 0xEE)[0][11] == 1 and len(seg(d, 0xEE)[0]) == 12
    d = mk("jfif_and_adobe0")
    assert seg(d, 0xE0) and seg(d, 0xEE)[0][11] == 0
    assert b"\xff\xd8" in seg(mk("app1_thumbnail"), 0xE1)[0] and b"\xff\xd9" in seg(mk("app1_thumbnail"), 0xE1)[0]
    for m in (0xE2, 0xFE):
        assert all(x in seg(mk("app2_com_markers"), m)[0] for x in (b"\xff\xd8", b"\xff\xd9", b"\xff\xda"))
    d = mk("trailing_bytes")
    assert d.count(b"\xff\xd8\xff\xe0") == 2 and not d.endswith(STREAMS["trailing_bytes"](H, W)[1][-64:])
    assert b"\xff\xd9" not in mk("no_eoi")[-2:]
    for hv in (0x22, 0x21, 0x14, 0x44):
        c = jpeg.parse(mk(f"gray_{hv:#04x}"))["frame"]["comps"]
        assert len(c) == 1 and (c[0]["h"], c[0]["v"]) == (hv >> 4, hv & 15)
    # the refused ones: what makes each of them RGB, and the swapped scan
    d = REFUSED["keep_rgb"](H, W)
    assert not seg(d, 0xE0) and seg(d, 0xEE)[0][11] == 0 and [seg(d, 0xC0)[0][6 + 3 * k] for k in range(3)] == list(b"RGB")
    d = REFUSED["adobe0_no_jfif"](H, W)
    assert not seg(d, 0xE0) and seg(d, 0xEE)[0][11] == 0 and [seg(d, 0xC0)[0][6 + 3 * k] for k in range(3)] == [1, 2, 3]
    d = REFUSED["ids_RGB_bare"](H, W)
    assert not seg(d, 0xE0) and not seg(d, 0xEE) and [seg(d, 0xC0)[0][6 + 3 * k] for k in range(3)] == list(b"RGB")
    d = REFUSED["sos_ids_swapped"](H, W)
    assert [seg(d, 0xDA)[0][1 + 2 * k] for k in range(3)] == [2, 1, 3] and [seg(d, 0xDA)[0][2 + 2 * k] for k in range(3)] == [0, 0x11, 0x11]
    assert seg(REFUSED["cmyk"](H, W), 0xC0)[0][5] == 4


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_streams(name):
    """RGB-coded planes by libjpeg's colour-space rule (libjpeg returns them unconverted, which nothing here
    restates), a scan whose components are not in the frame's order (libjpeg refuses it too), CMYK."""
    data = REFUSED[name](37, 53)
    with pytest.raises(jpeg.JpegError):
        jpeg.decode(data)
    if name in RGB_REFUSED:  # libjpeg takes them, and not as YCbCr: the same planes marked JFIF decode otherwise
        ycc = jpeg.decode(as_jfif(data))
        assert not np.array_equal(reference_decode(data), ycc)
    if name == "sos_ids_swapped":
        with pytest.raises(OSError):
            reference_decode(data)


@pytest.mark.parametrize("H,W", STREAM_SHAPES)
@pytest.mark.parametrize("sub,ss", SUBSAMPLINGS)
def test_entropy_extremes(sub, ss, H, W):
    """A DC difference of category 11, blocks without an EOB, restart intervals of a few bytes: each edge is
    shown to be present in the stream, then the restatement equals libjpeg."""
    data = encode(checkerboard(H, W), quality=100, subsampling=ss)
    j = jpeg.parse(data)
    assert max(abs(v) for v in luma_dc_differences(j, jpeg.decode_coefficients(j))) == 2040
    assert np.array_equal(jpeg.decode(data), reference_decode(data))
    data = encode(busy_noise(H, W), quality=100, subsampling=ss)
    luma = jpeg.decode_coefficients(jpeg.parse(data))[0]
    assert np.all(luma[:-(-H // 8), :-(-W // 8), 63] != 0)  # every block of the image (MCU padding blocks are empty)
    assert np.array_equal(jpeg.decode(data), reference_decode(data))
    data = encode(constant(H, W), quality=75, subsampling=ss, restart_marker_blocks=1)
    lens = restart_interval_lengths(jpeg.parse(data))
    assert len(lens) == -(-H // (16 if ss == 2 else 8)) * -(-W // (8 if ss == 0 else 16)) and min(lens) <= 4
    assert np.array_equal(jpeg.decode(data), reference_decode(data))


def _marker_stream(ns, nc=3):
    """SOI, SOF0 (8-bit, 16x16, nc components at 1x1), SOS naming ns of them: the markers only."""
    sof = bytes([8, 0, 16, 0, 16, nc]) + b"".join(bytes([c + 1, 0x11, 0]) for c in range(nc))
    sos = bytes([ns]) + b"".join(bytes([c + 1, 0]) for c in range(ns)) + bytes([0, 63, 0])
    seg = lambda m, body: bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body  # noqa: E731
    return b"\xff\xd8" + seg(0xC0, sof) + seg(0xDA, sos) + b"\x00" * 8 + b"\xff\xd9"


def test_jpeg_gpu_supported_needs_one_interleaved_scan():
    """A frame whose components come in separate scans (first SOS with Ns < Nf) is refused up front, as
    parse_jpeg (fm_jpeg.hip) would refuse it (the advisor's round-3 finding)."""
    from find_motion_amd import videoio
    assert videoio.jpeg_gpu_supported(_marker_stream(3))
    assert not videoio.jpeg_gpu_supported(_marker_stream(1))
    assert not videoio.jpeg_gpu_supported(_marker_stream(2))
    assert videoio.jpeg_gpu_supported(_marker_stream(1, nc=1))


class _StubCv2:
    """Just enough of cv2 for open_capture's choice: VideoCapture records what it was opened on."""

    class VideoCapture:
        def __init__(self, src):
            self.src = src

        def isOpened(self):  # noqa: N802
            return True

    IMREAD_COLOR = 1


def _mjpeg_avi(tmp_path, **kw):
    from find_motion_amd import videoio
    p = str(tmp_path / "m.avi")
    w = videoio.MjpegAviWriter(p, 25, (40, 24))
    for s in range(3):
        w.write_jpeg(encode(image(24, 40, "smooth", seed=s), quality=75, **kw))
    w.release()
    return p


def test_open_capture_keeps_the_reference_capture_when_cv2_imports(tmp_path, monkeypatch):
    """fm.py:413: cv2.VideoCapture(filename) whenever OpenCV exists, MJPEG included; the GPU decoder only on
    opt-in (gpu_decode=True), and never for a layout it does not take."""
    from find_motion_amd import videoio
    p = _mjpeg_avi(tmp_path)
    monkeypatch.setattr(videoio, "cv2", _StubCv2)
    cap = videoio.open_capture(p)
    assert isinstance(cap, _StubCv2.VideoCapture) and cap.src == p
    assert isinstance(videoio.open_capture(p, gpu_decode=False), _StubCv2.VideoCapture)
    cap = videoio.open_capture(p, gpu_decode=True)
    assert isinstance(cap, videoio.MjpegAviCapture) and cap.gpu_decode
    q = str(tmp_path / "p.avi")
    w = videoio.MjpegAviWriter(q, 25, (40, 24))
    w.write_jpeg(encode(image(24, 40, "smooth"), quality=75, progressive=True))
    w.release()
    assert isinstance(videoio.open_capture(q, gpu_decode=True), _StubCv2.VideoCapture)
    raw = str(tmp_path / "r.avi")
    videoio.RawAviWriter(raw, 25, (40, 24)).release()
    assert isinstance(videoio.open_capture(raw), _StubCv2.VideoCapture)


def test_open_capture_without_cv2(tmp_path, monkeypatch):
    """No OpenCV: MJPEG AVIs are read here -- GPU decode for supported layouts (the default), host decode
    (Pillow, libjpeg-turbo) for the rest or on gpu_decode=False; BatchFeeder's JPEG mode only for the former."""
    from find_motion_amd import videoio
    monkeypatch.setattr(videoio, "cv2", None)
    p = _mjpeg_avi(tmp_path)
    cap = videoio.open_capture(p)
    assert isinstance(cap, videoio.MjpegAviCapture) and cap.gpu_decode
    cap = videoio.open_capture(p, gpu_decode=False)
    assert isinstance(cap, videoio.MjpegAviCapture) and not cap.gpu_decode
    ok, fr = cap.read()
    assert ok and np.array_equal(fr, reference_decode(encode(image(24, 40, "smooth", seed=0), quality=75)))
    q = str(tmp_path / "p.avi")
    w = videoio.MjpegAviWriter(q, 25, (40, 24))
    pj = encode(image(24, 40, "smooth"), quality=75, progressive=True)
    w.write_jpeg(pj)
    w.release()
    cap = videoio.open_capture(q, gpu_decode=True)
    assert isinstance(cap, videoio.MjpegAviCapture) and not cap.gpu_decode
    ok, fr = cap.read()
    assert ok and np.array_equal(fr, reference_decode(pj))
