"""numpy restatement of the baseline JPEG encode the GPU MJPG writer reproduces (find_motion_amd/csrc/fm_jpeg_enc.hip)
-- TEST INFRASTRUCTURE, stage by stage so that a GPU mismatch can be traced to colour, DCT or entropy coding.

The target is libjpeg-turbo as Pillow calls it: Image.save(..., "JPEG", quality=q, subsampling=s), i.e.
jpeg_set_quality(q, force_baseline), JDCT_ISLOW, the T.81 Annex K Huffman tables (not optimized).  Stages, by the
libjpeg file whose arithmetic they follow: jccolor.c (16-bit fixed-point YCbCr), jcprepct.c / jcsample.c (edge
replication, h2v1 / h2v2 downsampling with alternating bias), jfdctint.c (CONST_BITS 13, PASS1_BITS 2),
jcdctmgr.c (quantization by plain division), jccoefct.c (dummy blocks), jchuff.c (Huffman coding, byte stuffing,
restart markers), jcmarker.c (segment order).

    encode(bgr, quality, subsampling, restart_interval) -> bytes       the whole file
    coefficients(bgr, quality, subsampling) -> int16 [blocks][64]      scan (MCU-interleaved) order, zigzag
    header(width, height, quality, subsampling, restart_interval)      SOI .. SOS
"""
from __future__ import annotations

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
                   31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)  # zigzag index -> natural index

# T.81 Annex K.1 quantization tables (natural order), scaled by jpeg_set_quality
STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
              47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# T.81 Annex K.3 Huffman tables: (code counts per length 1..16, symbols)
_AC0 = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
        0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
        0x82, 0x09, 0x0a, 0x16]
_AC1 = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
        0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
        0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1]


def _ac(head):
    return head + [rs for rs in range(256) if 1 <= (rs & 15) <= 10 and rs not in head]


HUFF = {  # (class, slot)
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], _ac(_AC0)),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _ac(_AC1)),
}
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}  # Pillow's subsampling value -> Y's (h, v); Cb, Cr are 1x1


def quant_tables(quality: int):
    """jpeg_set_quality(quality, force_baseline): (luma, chroma) in natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((np.array(t, np.int64) * scale + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA)]


def _codes(bits, vals):
    """{symbol: (code, length)} of a canonical Huffman table."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def header(width: int, height: int, quality: int, subsampling: int, restart_interval: int = 0) -> bytes:
    """SOI, APP0 (JFIF 1.01, density 1x1 without units), DQT x2, SOF0, DHT x4, [DRI], SOS."""
    h, v = SAMPLING[subsampling]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate(quant_tables(quality)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(x) for x in q[ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + bytes([height >> 8, height & 255, width >> 8, width & 255, 3,
                                             1, (h << 4) | v, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls, slot in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = HUFF[(cls, slot)]
        ln = 2 + 1 + 16 + len(vals)
        out += b"\xff\xc4" + bytes([ln >> 8, ln & 255, (cls << 4) | slot]) + bytes(bits) + bytes(vals)
    if restart_interval:
        out += b"\xff\xdd\x00\x04" + bytes([restart_interval >> 8, restart_interval & 255])
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def ycc(bgr: np.ndarray):
    """jccolor.c rgb_ycc_convert: three int planes."""
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_cols(p, n):
    return p if p.shape[1] >= n else np.concatenate([p, np.repeat(p[:, -1:], n - p.shape[1], 1)], 1)


def _pad_rows(p, n):
    return p if p.shape[0] >= n else np.concatenate([p, np.repeat(p[-1:], n - p.shape[0], 0)], 0)


def component_planes(bgr: np.ndarray, subsampling: int):
    """The three sample planes as the DCT sees them, each padded to its own block grid: columns are replicated
    on the full-resolution plane, rows only up to a multiple of v before downsampling and the downsampled rows
    after it."""
    H, W = bgr.shape[:2]
    h, v = SAMPLING[subsampling]
    planes = []
    for ci, p in enumerate(ycc(bgr)):
        ch, cv = (h, v) if ci == 0 else (1, 1)
        cw, chh = -(-W * ch // h), -(-H * cv // v)          # component size in samples
        bw, bh = -(-cw // 8), -(-chh // 8)                  # its own block grid
        fx, fy = h // ch, v // cv                            # downsampling factors
        p = _pad_rows(_pad_cols(p, bw * 8 * fx), -(-H // v) * v)
        if fx == 2 and fy == 2:
            bias = np.tile([1, 2], p.shape[1] // 2)[: p.shape[1] // 2]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif fx == 2:
            bias = np.tile([0, 1], p.shape[1] // 2)[: p.shape[1] // 2]
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        planes.append(_pad_rows(p, bh * 8)[: bh * 8, : bw * 8])
    return planes


def _fdct_1d(d, first: bool):
    """One pass of jfdctint.c over the last axis (8 samples)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15

    def ds(x, n):
        return (x + (1 << (n - 1))) >> n

    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = ds(t10 + t11, 2), ds(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = ds(z1 + t13 * 6270, sh), ds(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, sh), ds(t5 + z2 + z4, sh), ds(t6 + z2 + z3, sh), ds(t7 + z1 + z4, sh)
    return np.stack(o, -1)


def fdct_quant(block: np.ndarray, q: np.ndarray) -> np.ndarray:
    """8x8 samples -> 64 quantized coefficients, natural order."""
    w = _fdct_1d(block.astype(np.int64) - 128, True)                 # rows
    w = _fdct_1d(w.T, False).T                                        # columns
    c = w.reshape(64)
    q8 = q * 8
    return np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)


def coefficients(bgr: np.ndarray, quality: int, subsampling: int) -> np.ndarray:
    """int16 [MCUs * blocks per MCU][64]: scan order, zigzag, dummy blocks included (jccoefct.c: a block of an
    MCU beyond its component's own grid has zero AC and the DC of the block before it in the MCU)."""
    H, W = bgr.shape[:2]
    h, v = SAMPLING[subsampling]
    planes = component_planes(bgr, subsampling)
    qt = quant_tables(quality)
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    out = []
    for m in range(mx * my):
        mr, mc = divmod(m, mx)
        for ci, (ch, cv) in enumerate(((h, v), (1, 1), (1, 1))):
            p = planes[ci]
            for by in range(cv):
                for bx in range(ch):
                    r, c = (mr * cv + by) * 8, (mc * ch + bx) * 8
                    if r < p.shape[0] and c < p.shape[1]:
                        out.append(fdct_quant(p[r:r + 8, c:c + 8], qt[min(ci, 1)])[ZIGZAG])
                    else:
                        d = np.zeros(64, np.int64)
                        d[0] = out[-1][0]
                        out.append(d)
    return np.array(out, np.int16)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def entropy_code(coef: np.ndarray, subsampling: int, restart_interval: int = 0) -> bytes:
    """Scan-order zigzag coefficients -> the stuffed entropy-coded segment with RSTn markers (jchuff.c)."""
    h, v = SAMPLING[subsampling]
    bpm = h * v + 2
    comp_of = [0] * (h * v) + [1, 2]
    tabs = {k: _codes(*t) for k, t in HUFF.items()}
    w, pred = _Bits(), [0, 0, 0]
    nm = len(coef) // bpm
    for m in range(nm):
        if restart_interval and m and m % restart_interval == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + ((m // restart_interval - 1) & 7)])
            pred = [0, 0, 0]
        for k in range(bpm):
            blk = coef[m * bpm + k].astype(np.int64)
            ci = comp_of[k]
            slot = min(ci, 1)
            d = int(blk[0]) - pred[ci]
            pred[ci] = int(blk[0])
            for run_sym, val in _symbols(d, blk):
                code, ln = tabs[(0 if run_sym[0] == "dc" else 1, slot)][run_sym[1]]
                w.put(code, ln)
                s = run_sym[1] & 15
                if s:
                    w.put((val if val >= 0 else val - 1) & ((1 << s) - 1), s)
    w.flush()
    return bytes(w.out)


def _symbols(dc_diff: int, blk):
    yield ("dc", abs(dc_diff).bit_length()), dc_diff
    run = 0
    nz = np.nonzero(blk[1:])[0]
    last = int(nz[-1]) + 1 if len(nz) else 0
    for k in range(1, last + 1):
        a = int(blk[k])
        if a == 0:
            run += 1
            continue
        while run > 15:
            yield ("ac", 0xF0), 0
            run -= 16
        yield ("ac", (run << 4) | abs(a).bit_length()), a
        run = 0
    if last < 63:
        yield ("ac", 0x00), 0


def encode(bgr: np.ndarray, quality: int = 95, subsampling: int = 2, restart_interval: int = 0) -> bytes:
    """BGR u8 [H][W][3] -> the JPEG file Pillow writes for the same pixels and settings."""
    H, W = bgr.shape[:2]
    coef = coefficients(bgr, quality, subsampling)
    return header(W, H, quality, subsampling, restart_interval) + \
        entropy_code(coef, subsampling, restart_interval) + b"\xff\xd9"
