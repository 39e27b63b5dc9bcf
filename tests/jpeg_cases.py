"""JPEG test inputs for the decode side (§8(f)-3): frames encoded by Pillow (libjpeg-turbo), decoded by Pillow
as the reference decode.  That is libjpeg-turbo's default decode, i.e. cv2.imdecode and OpenCV's built-in
MJPEG reader (CAP_OPENCV_MJPEG); cv2.VideoCapture's default FFmpeg backend decodes with libavcodec + swscale
instead, which nothing here can pin (neither is in the image)."""
from __future__ import annotations

import io

import numpy as np

import jpeg_encode_ref as ref

try:
    from PIL import Image
except ImportError:  # pragma: no cover - Pillow is in the image; the tests skip without it
    Image = None

# (name, encoder keyword arguments): 4:2:0 / 4:2:2 / 4:4:4, qualities, restart intervals
ENCODINGS = [
    ("420_q75", dict(quality=75)),
    ("420_q30", dict(quality=30)),
    ("444_q95", dict(quality=95, subsampling=0)),
    ("422_q50", dict(quality=50, subsampling=1)),
    ("420_rst3", dict(quality=80, restart_marker_blocks=3)),
    ("422_rstrow", dict(quality=70, subsampling=1, restart_marker_rows=1)),
]


def image(H: int, W: int, kind: str, seed: int = 1) -> np.ndarray:
    """BGR u8 test image: noise (every coefficient busy) or a noisy gradient (typical video)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y) * 7) % 256], -1)
    return (img + rng.integers(-20, 21, img.shape)).clip(0, 255).astype(np.uint8)


def encode(bgr: np.ndarray, **kw) -> bytes:
    """BGR (or gray) u8 -> JPEG bytes (Pillow, libjpeg-turbo)."""
    arr = bgr[..., ::-1] if bgr.ndim == 3 else bgr
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(b, "JPEG", **kw)
    return b.getvalue()


def reference_decode(data: bytes) -> np.ndarray:
    """Pillow's libjpeg-turbo decode -> BGR u8 (gray replicated to three channels, as cap.read returns)."""
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    if a.ndim == 2:
        return np.repeat(a[..., None], 3, axis=2)
    return np.ascontiguousarray(a[..., ::-1])


def segments(data: bytes):
    """(marker, start, end) of every marker segment before the scan data (SOI excluded)."""
    out, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m = data[i + 1]
        ln = (data[i + 2] << 8) | data[i + 3]
        out.append((m, i, i + 2 + ln))
        if m == 0xDA:
            break
        i += 2 + ln
    return out


def strip_dht(data: bytes) -> bytes:
    """The same JPEG without its DHT segments (the AVI1 Motion-JPEG form many cameras write: the decoder
    supplies the T.81 Annex K tables, which are exactly what libjpeg-turbo encodes with by default)."""
    out, last = bytearray(data[:2]), 2
    for m, a, b in segments(data):
        out += data[last:a]
        if m != 0xC4:
            out += data[a:b]
        last = b
    return bytes(out + data[last:])


def segment(marker: int, payload: bytes) -> bytes:
    """One marker segment: FF, the marker, the two length bytes, the payload."""
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _rewrite(data: bytes, fn) -> bytes:
    """The same JPEG with its header segments (SOI excluded, SOS included) replaced by what fn returns for
    the list of [marker, payload] pairs; the entropy-coded data and what follows it are kept."""
    segs = segments(data)
    assert segs and segs[-1][0] == 0xDA, "no SOS"
    out = fn([[m, data[a + 4:b]] for m, a, b in segs])
    return data[:2] + b"".join(segment(m, p) for m, p in out) + data[segs[-1][2]:]


def drop_segments(data: bytes, marker: int) -> bytes:
    """The same JPEG without its segments of this marker."""
    return _rewrite(data, lambda segs: [s for s in segs if s[0] != marker])


def insert_after_soi(data: bytes, *segs: bytes) -> bytes:
    """The same JPEG with whole segments (see segment()) put right after the SOI."""
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"".join(segs) + data[2:]


def merge_segments(data: bytes, marker: int) -> bytes:
    """Every segment of this marker (DQT or DHT: a payload is a list of tables) merged into one, at the place
    of the first."""
    def fn(segs):
        body = b"".join(p for m, p in segs if m == marker)
        out, done = [], False
        for m, p in segs:
            if m != marker:
                out.append([m, p])
            elif not done:
                out.append([m, body])
                done = True
        return out
    return _rewrite(data, fn)


def _is_sof(m: int) -> bool:
    return 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)


def renumber_components(data: bytes, ids) -> bytes:
    """Component k of the frame gets id ids[k], in the SOF and in the SOS selectors together."""
    def fn(segs):
        old = {}
        for s in segs:
            p = bytearray(s[1])
            if _is_sof(s[0]):
                for k in range(p[5]):
                    old[p[6 + 3 * k]] = ids[k]
                    p[6 + 3 * k] = ids[k]
            elif s[0] == 0xDA:
                for k in range(p[0]):
                    p[1 + 2 * k] = old[p[1 + 2 * k]]
            s[1] = bytes(p)
        return segs
    return _rewrite(data, fn)


def renumber_huffman(data: bytes, ids: dict) -> bytes:
    """Huffman table id t becomes ids[t] (both classes), in every DHT and in the SOS selectors."""
    def fn(segs):
        for s in segs:
            p = bytearray(s[1])
            if s[0] == 0xC4:
                q = 0
                while q < len(p):
                    p[q] = (p[q] & 0xF0) | ids.get(p[q] & 15, p[q] & 15)
                    q += 17 + sum(p[q + 1:q + 17])
            elif s[0] == 0xDA:
                for k in range(p[0]):
                    b = p[2 + 2 * k]
                    p[2 + 2 * k] = (ids.get(b >> 4, b >> 4) << 4) | ids.get(b & 15, b & 15)
            s[1] = bytes(p)
        return segs
    return _rewrite(data, fn)


def renumber_quant(data: bytes, ids: dict) -> bytes:
    """Quantization table id t becomes ids[t], in every DQT and in the SOF's component entries."""
    def fn(segs):
        for s in segs:
            p = bytearray(s[1])
            if s[0] == 0xDB:
                q = 0
                while q < len(p):
                    step = 129 if p[q] >> 4 else 65
                    p[q] = (p[q] & 0xF0) | ids.get(p[q] & 15, p[q] & 15)
                    q += step
            elif _is_sof(s[0]):
                for k in range(p[5]):
                    p[8 + 3 * k] = ids.get(p[8 + 3 * k], p[8 + 3 * k])
            s[1] = bytes(p)
        return segs
    return _rewrite(data, fn)


def set_gray_sampling(data: bytes, hv: int) -> bytes:
    """A one-component frame with its SOF sampling byte set to hv (a single component's factors change
    nothing: its scan is not interleaved, T.81 A.2.2)."""
    def fn(segs):
        for s in segs:
            if _is_sof(s[0]):
                assert s[1][5] == 1, "not a one-component frame"
                s[1] = s[1][:7] + bytes([hv]) + s[1][8:]
        return segs
    return _rewrite(data, fn)


def append_after_eoi(data: bytes, extra: bytes) -> bytes:
    assert data[-2:] == b"\xff\xd9"
    return data + extra


def drop_eoi(data: bytes) -> bytes:
    assert data[-2:] == b"\xff\xd9"
    return data[:-2]


def swap_sos_ids(data: bytes, a: int = 0, b: int = 1) -> bytes:
    """The component selectors of scan entries a and b exchanged (their table selectors stay): a scan whose
    component order differs from the frame's, which T.81 B.2.3 forbids and libjpeg refuses."""
    def fn(segs):
        p = bytearray(segs[-1][1])
        p[1 + 2 * a], p[1 + 2 * b] = p[1 + 2 * b], p[1 + 2 * a]
        segs[-1][1] = bytes(p)
        return segs
    return _rewrite(data, fn)


def adobe_app14(transform: int) -> bytes:
    """An Adobe APP14 segment: 'Adobe', version 100, flags0, flags1, the colour transform byte."""
    return segment(0xEE, b"Adobe" + (100).to_bytes(2, "big") + b"\0\0\0\0" + bytes([transform]))


def fill_before_markers(data: bytes, n: int = 2) -> bytes:
    """Insert n 0xFF fill bytes before every RSTn marker and the EOI of the scan (T.81 B.1.1.2 allows any
    number; libjpeg skips them)."""
    sos = [s for s in segments(data) if s[0] == 0xDA][0]
    head, scan = data[:sos[2]], data[sos[2]:]
    out, k = bytearray(), 0
    while k < len(scan):
        c = scan[k]
        if c == 0xFF and k + 1 < len(scan) and (0xD0 <= scan[k + 1] <= 0xD7 or scan[k + 1] == 0xD9):
            out += b"\xff" * n
        out.append(c)
        k += 1
    return bytes(head + out)


# ---- streams Pillow's default encoder never writes (tests/test_gpu_jpeg_streams.py, tests/test_jpeg_host.py)

def _after_jfif(data: bytes, *segs: bytes) -> bytes:
    """Segments put right after the JFIF APP0 (which stays first, as JFIF asks)."""
    m, a, b = segments(data)[0]
    assert m == 0xE0
    return insert_after_soi(drop_segments(data, 0xE0), data[a:b], *segs)


def _base(H: int, W: int, seed: int = 3, **kw) -> bytes:
    """4:2:0 unless told otherwise; quality 85 unless the tables are given (Pillow would scale them by it)."""
    return encode(image(H, W, "smooth", seed=seed), **{**({} if "qtables" in kw else {"quality": 85}), **kw})


def _opt(H: int, W: int, seed: int = 3) -> bytes:
    return _base(H, W, seed, optimize=True)


def _gray(H: int, W: int, seed: int = 3) -> bytes:
    return encode(image(H, W, "smooth", seed=seed)[..., 1], quality=85)


_QT3 = [[1 + (k * 7) % 23 for k in range(64)], [2 + (k * 5) % 61 for k in range(64)], [3 + (k * 11) % 97 for k in range(64)]]
_MARKERS = b"x\xff\xd8y\xff\xd9z\xff\xda\x00\x0c\x03\x01\x00\xff\xc4\xff\xd9"


def _thumbnail() -> bytes:
    return encode(image(8, 8, "noise", seed=9), quality=50)


def _keep_rgb(H: int, W: int) -> bytes:
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(image(H, W, "smooth", seed=3)[..., ::-1])).save(b, "JPEG", quality=85, keep_rgb=True)
    return b.getvalue()


def _cmyk(H: int, W: int) -> bytes:
    b = io.BytesIO()
    Image.fromarray(image(H, W, "smooth", seed=3)[..., [0, 1, 2, 0]].copy(), "CMYK").save(b, "JPEG", quality=85)
    return b.getvalue()


# name -> (H, W, image seed = 3) -> (stream, the unpatched stream it must decode like or None).
# The decoder takes all of these.
STREAMS = {
    "dqt16_sof1": lambda H, W, s=3: (_base(H, W, s, qtables=[[300] * 64, [1000] * 64]), None),
    "three_qtables": lambda H, W, s=3: (_base(H, W, s, qtables=_QT3), None),
    "quant_ids_2_3": lambda H, W, s=3: (renumber_quant(_base(H, W, s), {0: 2, 1: 3}), _base(H, W, s)),
    "huff_ids_2_3": lambda H, W, s=3: (renumber_huffman(_base(H, W, s), {0: 2, 1: 3}), _base(H, W, s)),
    # the stream's own (optimized) tables: a table taken from the wrong slot is then not the standard one either
    "huff_ids_3_2": lambda H, W, s=3: (renumber_huffman(_opt(H, W, s), {0: 3, 1: 2}), _opt(H, W, s)),
    "merged_dht": lambda H, W, s=3: (merge_segments(_opt(H, W, s), 0xC4), _opt(H, W, s)),
    "merged_dqt": lambda H, W, s=3: (merge_segments(_base(H, W, s), 0xDB), _base(H, W, s)),
    "merged_dqt16": lambda H, W, s=3: (merge_segments(_base(H, W, s, qtables=[[300] * 64, [1000] * 64]), 0xDB),
                                  _base(H, W, s, qtables=[[300] * 64, [1000] * 64])),
    "ids_012_jfif": lambda H, W, s=3: (renumber_components(_base(H, W, s), [0, 1, 2]), _base(H, W, s)),
    "ids_012_no_jfif": lambda H, W, s=3: (drop_segments(renumber_components(_base(H, W, s), [0, 1, 2]), 0xE0), _base(H, W, s)),
    "adobe1_no_jfif": lambda H, W, s=3: (insert_after_soi(drop_segments(_base(H, W, s), 0xE0), adobe_app14(1)), _base(H, W, s)),
    "jfif_and_adobe0": lambda H, W, s=3: (_after_jfif(_base(H, W, s), adobe_app14(0)), _base(H, W, s)),
    "app1_thumbnail": lambda H, W, s=3: (_after_jfif(_base(H, W, s), segment(0xE1, b"Exif\0\0" + _thumbnail())), _base(H, W, s)),
    "app2_com_markers": lambda H, W, s=3: (_after_jfif(_base(H, W, s), segment(0xE2, _MARKERS), segment(0xFE, _MARKERS)),
                                      _base(H, W, s)),
    "trailing_bytes": lambda H, W, s=3: (append_after_eoi(_base(H, W, s), b"\0junk\xff\xff" + _base(H, W, s, quality=40)),
                                    _base(H, W, s)),
    "no_eoi": lambda H, W, s=3: (drop_eoi(_base(H, W, s)), _base(H, W, s)),
    "gray_0x22": lambda H, W, s=3: (set_gray_sampling(_gray(H, W, s), 0x22), _gray(H, W, s)),
    "gray_0x21": lambda H, W, s=3: (set_gray_sampling(_gray(H, W, s), 0x21), _gray(H, W, s)),
    "gray_0x14": lambda H, W, s=3: (set_gray_sampling(_gray(H, W, s), 0x14), _gray(H, W, s)),
    "gray_0x44": lambda H, W, s=3: (set_gray_sampling(_gray(H, W, s), 0x44), _gray(H, W, s)),
}

# name -> (H, W) -> stream.  The decoder refuses these: RGB-coded planes (libjpeg's colour-space rule), a scan
# whose components are not in the frame's order, four components.
REFUSED = {
    "keep_rgb": _keep_rgb,
    "adobe0_no_jfif": lambda H, W, s=3: insert_after_soi(drop_segments(_base(H, W, s, subsampling=0), 0xE0), adobe_app14(0)),
    "ids_RGB_bare": lambda H, W, s=3: drop_segments(renumber_components(_base(H, W, s, subsampling=0), [0x52, 0x47, 0x42]), 0xE0),
    "sos_ids_swapped": lambda H, W, s=3: swap_sos_ids(_base(H, W, s, subsampling=0), 0, 1),
    "cmyk": _cmyk,
}
RGB_REFUSED = ("keep_rgb", "adobe0_no_jfif", "ids_RGB_bare")


def as_jfif(data: bytes) -> bytes:
    """The stream with component ids 1, 2, 3, no Adobe segment and a JFIF APP0: YCbCr by libjpeg's rule."""
    d = drop_segments(drop_segments(renumber_components(data, [1, 2, 3]), 0xEE), 0xE0)
    return insert_after_soi(d, segment(0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0"))


def reference_decode_truncated(data: bytes) -> np.ndarray:
    """reference_decode of a stream without EOI: libjpeg supplies the EOI, Pillow must be told to accept it."""
    from PIL import ImageFile
    old = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    try:
        return reference_decode(data)
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = old


def stream_reference(name: str, data: bytes) -> np.ndarray:
    return reference_decode_truncated(data) if name == "no_eoi" else reference_decode(data)


# ---- entropy extremes

SUBSAMPLINGS = [("444", 0), ("422", 1), ("420", 2)]


def checkerboard(H: int, W: int) -> np.ndarray:
    """8 x 8 blocks, black and white in turn: at quality 100 the luma DC goes from -1024 to 1016 and back."""
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(((((y >> 3) + (x >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def busy_noise(H: int, W: int, seed: int = 5) -> np.ndarray:
    """Noise over a pixel checkerboard (the sign pattern of the DCT's basis function 7,7): at quality 100
    coefficient 63 of every luma block is far from zero, so no block of the image ends in an EOB."""
    y, x = np.mgrid[0:H, 0:W]
    carrier = 128 + 60 * (1 - 2 * ((x + y) & 1))
    rng = np.random.default_rng(seed)
    return (carrier[..., None] + rng.integers(-50, 51, (H, W, 3))).astype(np.uint8)


def constant(H: int, W: int) -> np.ndarray:
    return np.full((H, W, 3), 128, np.uint8)


def chroma_checkerboard(H: int, W: int, cell: int = 8) -> np.ndarray:
    """cell x cell squares, blue (Cb 255) and yellow (Cb 0) in turn, Y and Cr nearly level: at quality 100 the Cb
    DC goes from 1016 to -1024 and back, a difference of category 11 with both signs.  cell = 16 keeps that
    through 4:2:0's 2 x 2 averaging."""
    y, x = np.mgrid[0:H, 0:W]
    blue = (((y // cell) + (x // cell)) & 1) == 0
    return np.where(blue[..., None], np.array([255, 0, 0], np.uint8), np.array([0, 255, 255], np.uint8))


def dc_ladder(slot: int) -> np.ndarray:
    """17 level 8 x 8 blocks in a row, 127 and 127 + 2^k in turn for k = 0..7: at quality 100 and 4:4:4 the DC
    differences of the component are -8, then +8 * 2^k and -8 * 2^k, categories 4 to 11 with both signs (1 to 3
    come with symbol_sweep).  Slot 0: gray levels.  Slot 1: B = L, G = R = 255 - L, whose Cb is L exactly."""
    levels = [127]
    for k in range(8):
        levels += [127 + (1 << k), 127]
    p = np.repeat(np.repeat(np.array(levels)[None, :], 8, 0), 8, 1)
    return np.stack([p, p, p] if slot == 0 else [p, 255 - p, 255 - p], -1).astype(np.uint8)


# ---- the write side's entropy coder: every (run, size) symbol, ZRL chains, the stuffing kernels' seams

SWEEP_QUALITIES = (10, 25, 50, 75, 90, 100)
SWEEP_LONE = (17, 18, 33, 34, 49, 50, 63)  # zigzag positions: 1, 2, 3 ZRLs before the value; 63 leaves no EOB
SWEEP_COLS = 20                            # blocks per image row


def _dct_basis() -> np.ndarray:
    """[u][x]: the orthonormal 8-point DCT-II matrix."""
    x = np.arange(8)
    m = np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    return m


def sweep_planes(slot: int, quality: int) -> np.ndarray:
    """The 8 x 8 sample blocks of symbol_sweep, u8 [n][8][8], aimed at the quantization table of `slot` at this
    quality (jpeg_set_quality's scaling, force_baseline):
      - for each run 0..15, size 1..10 and sign, the float IDCT of one coefficient at zigzag position 1 + run
        (2^size - 1, or -2^(size - 1)) times its quantizer, plus 128, rounded and clipped;
      - the same with a lone +-1 at each of SWEEP_LONE;
      - for each AC basis function, its sign pattern in 0 / 255 (at quality 100: the size 9 and 10 values).
    What a block really codes to is for the encoder under test and the reference to agree on: clipping bends
    the large targets, and rounding adds +-1 coefficients at quality 100."""
    q = ref.quant_tables(quality)[slot]
    m = _dct_basis()
    targets = [(1 + run, v) for run in range(16) for size in range(1, 11) for v in ((1 << size) - 1, -(1 << (size - 1)))]
    targets += [(k, v) for k in SWEEP_LONE for v in (1, -1)]
    blocks = []
    for k, v in targets:
        c = np.zeros(64)
        c[ref.ZIGZAG[k]] = v * q[ref.ZIGZAG[k]]
        blocks.append(np.rint(m.T @ c.reshape(8, 8) @ m + 128).clip(0, 255))
    for k in range(1, 64):
        c = np.zeros(64)
        c[ref.ZIGZAG[k]] = 1
        blocks.append(np.where(m.T @ c.reshape(8, 8) @ m > 0, 255, 0))
    return np.array(blocks).astype(np.uint8)


def symbol_sweep(slot: int, quality: int) -> np.ndarray:
    """BGR u8 image, to be encoded 4:4:4, whose blocks are sweep_planes(slot, quality), SWEEP_COLS to a row (the
    last row filled with level 128).  Slot 0 (luma tables): a gray image.  Slot 1 (chroma tables): the blocks
    are the Cb plane under Y = Cr = 128, converted to BGR by the JFIF equations, rounded and clipped."""
    b = sweep_planes(slot, quality)
    rows = -(-len(b) // SWEEP_COLS)
    b = np.concatenate([b, np.full((rows * SWEEP_COLS - len(b), 8, 8), 128, np.uint8)])
    p = b.reshape(rows, SWEEP_COLS, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, SWEEP_COLS * 8)
    if slot == 0:
        return np.repeat(p[..., None], 3, axis=2)
    cb = p.astype(np.float64) - 128
    bgr = np.stack([128 + 1.772 * cb, 128 - 0.344136 * cb, np.full_like(cb, 128)], -1)
    return np.rint(bgr).clip(0, 255).astype(np.uint8)


SEAM_SHAPE = (64, 96)  # H, W: at 4:4:4 and quality 100 a noise frame's scan is about 25 KB, seven 4 KiB tiles
SEAM_TILE = 4096       # bytes of unstuffed stream per workgroup of the stuffing kernels (kTile, fm_jpeg_enc.hip)

# (image seed, restart interval in MCUs, conditions): seeded noise frames in whose Pillow file the conditions
# hold -- found by a search over seeds 0..399 at intervals 0, 1 and 2, and asserted by
# tests/test_jpeg_encode_host.py, so that the GPU tests on them cannot pass vacuously.
#   pair        FF 00 D0..D7 in the scan with restart markers on: a data pair that looks like an RSTn marker
#   ones_rst    FF 00 FF Dn: an all-ones padded byte before an RSTn marker
#   ones_eoi    the scan ends in FF 00: an all-ones byte before the EOI
#   tile_end    a data FF on the last byte of a tile of the unstuffed stream
#   tile_ffff   FF FF across such a tile seam
SEAM_CASES = [
    (0, 1, {"pair", "ones_rst"}),
    (1, 2, {"pair", "ones_rst"}),
    (3, 0, {"ones_eoi"}),
    (3, 1, {"ones_eoi", "ones_rst"}),
    (4, 1, {"tile_end"}),
    (13, 0, {"tile_end", "ones_eoi"}),
    (27, 2, {"tile_end"}),
    (399, 1, {"tile_end", "tile_ffff"}),
]


SHORT_SHAPE = (16, 32)  # H, W: eight 4:4:4 MCUs; a constant frame's scan is 14 bytes, less than a lane's 16


def seam_frame(seed: int) -> np.ndarray:
    return image(*SEAM_SHAPE, "noise", seed=seed)


def binary_noise(H: int, W: int, seed: int) -> np.ndarray:
    """Every sample 0 or 255: about 100 bytes a block at quality 100."""
    return (np.random.default_rng(seed).integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)


def scan_of(data: bytes) -> bytes:
    """The entropy-coded segment of a baseline file as written: after the SOS, without the EOI."""
    sos = [b for m, a, b in segments(data) if m == 0xDA][0]
    assert data[-2:] == b"\xff\xd9"
    return data[sos:-2]


def unstuffed_data_ff(scan: bytes):
    """(the scan with every FF 00 turned into FF, the offsets in it of those data FFs)."""
    out, ffs, k = bytearray(), [], 0
    while k < len(scan):
        out.append(scan[k])
        if scan[k] == 0xFF and k + 1 < len(scan) and scan[k + 1] == 0:
            ffs.append(len(out) - 1)
            k += 1
        k += 1
    return bytes(out), ffs


def seam_conditions(data: bytes) -> set:
    """Which of SEAM_CASES' conditions hold in this file (Pillow's)."""
    scan = scan_of(data)
    un, ffs = unstuffed_data_ff(scan)
    got = set()
    for k in range(len(scan) - 2):
        if scan[k] == 0xFF and scan[k + 1] == 0:
            if 0xD0 <= scan[k + 2] <= 0xD7:
                got.add("pair")
            if k + 3 < len(scan) and scan[k + 2] == 0xFF and 0xD0 <= scan[k + 3] <= 0xD7:
                got.add("ones_rst")
    if scan[-2:] == b"\xff\x00":
        got.add("ones_eoi")
    for p in ffs:
        if p % SEAM_TILE == SEAM_TILE - 1 and p + 1 < len(un):
            got.add("tile_end")
            if un[p + 1] == 0xFF:
                got.add("tile_ffff")
    return got


def _entropy_cases() -> dict:
    """name -> (image function, quality, subsampling, restart intervals in MCUs): the inputs on which the encoder's
    entropy coder is pinned (tests/test_gpu_jpeg_encode.py) and, through Pillow's files, the decoder's."""
    out = {}
    for slot, nm in ((0, "luma"), (1, "chroma")):
        for q in SWEEP_QUALITIES:
            out[f"sweep_{nm}_q{q}"] = (lambda slot=slot, q=q: symbol_sweep(slot, q), q, 0, (0, 1))
        out[f"ladder_{nm}"] = (lambda slot=slot: dc_ladder(slot), 100, 0, (0,))
    for sub, ss in SUBSAMPLINGS[::2]:
        out[f"checker_luma_{sub}"] = (lambda: checkerboard(24, 40), 100, ss, (0,))
        out[f"checker_chroma_{sub}"] = (lambda ss=ss: chroma_checkerboard(32, 48, 16 if ss else 8), 100, ss, (0,))
        out[f"busy_noise_{sub}"] = (lambda: busy_noise(37, 53), 100, ss, (0, 1))
    out["constant"] = (lambda: constant(16, 16), 75, 2, (0, 1))
    return out


ENTROPY_CASES = _entropy_cases()
# the 4:4:4 ones: Cb and Cr blocks are then whole blocks of the image, and the scan is Y, Cb, Cr in turn
COVERAGE_CASES = [n for n, c in ENTROPY_CASES.items() if c[2] == 0]


def luma_dc_differences(j: dict, coefs) -> list:
    """The DC differences of component 0 in scan order (no restart intervals), from oracle.jpeg.parse and
    decode_coefficients: dequantized DC / its quantizer, block after block as the MCUs interleave them."""
    assert j["dri"] == 0
    c = j["frame"]["comps"][0]
    dc = coefs[0][..., 0] // j["qt"][c["tq"]][0]
    bh, bw = dc.shape
    if len(j["frame"]["comps"]) == 1:
        W, H = j["frame"]["W"], j["frame"]["H"]
        seq = [dc[by, bx] for by in range(-(-H // 8)) for bx in range(-(-W // 8))]
    else:
        seq = [dc[my * c["v"] + v, mx * c["h"] + h] for my in range(bh // c["v"]) for mx in range(bw // c["h"])
               for v in range(c["v"]) for h in range(c["h"])]
    return [int(b) - int(a) for a, b in zip([0] + seq[:-1], seq)]


def restart_interval_lengths(j: dict) -> list:
    """Byte lengths of the restart intervals of oracle.jpeg.parse's entropy-coded segment."""
    out, n, d, k = [], 0, j["scan"]["data"], 0
    while k < len(d):
        if d[k] == 0xFF and k + 1 < len(d) and 0xD0 <= d[k + 1] <= 0xD7:
            out.append(n)
            n = 0
            k += 2
        else:
            n += 1
            k += 1
    return out + [n]
