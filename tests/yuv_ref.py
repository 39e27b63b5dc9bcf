"""TEST ONLY: a deliberately plain, per-pixel restatement of the YUV -> BGR conversion the engine runs on the GPU
(fm_submit_yuv) and videoio.yuv_to_bgr vectorises: cv2.cvtColor(yuv, COLOR_YUV2BGR_{NV12,I420,YUY2,UYVY}) as
OpenCV 4.x computes it -- BT.601 limited range, integer, the chroma pair of a 2x1 (YUY2 / UYVY) or 2x2 (NV12 /
I420) group replicated.  Independent of both: Python integers, one pixel at a time, the four layouts with their
pitch and chroma offset spelled out.
"""
import numpy as np

FORMATS = ("NV12", "I420", "YUY2", "UYVY")
PLANAR = ("NV12", "I420")

# (Y, U, V) -> (B, G, R), worked out by hand from the formula
KAT = [
    ((16, 128, 128), (0, 0, 0)),
    ((235, 128, 128), (255, 255, 255)),
    ((255, 128, 128), (255, 255, 255)),  # 278 before the clamp
    ((0, 128, 128), (0, 0, 0)),          # Y below 16
    ((128, 128, 128), (130, 130, 130)),
    ((126, 128, 129), (128, 127, 130)),
    ((81, 90, 240), (0, 0, 254)),        # B and G are -1 before the clamp: the shift floors
    ((145, 54, 34), (1, 255, 0)),
    ((41, 240, 110), (255, 0, 0)),
    ((255, 255, 255), (255, 125, 255)),
    ((0, 0, 0), (0, 154, 0)),
    ((235, 16, 16), (29, 255, 76)),
]


def sat_u8(v):
    return 0 if v < 0 else 255 if v > 255 else v


def pixel(Y, U, V):
    """(B, G, R) of one pixel; Python's >> on a negative int floors, as an arithmetic shift does."""
    uu, vv = int(U) - 128, int(V) - 128
    y = max(0, int(Y) - 16) * 1220542
    r = sat_u8((y + 524288 + 1673527 * vv) >> 20)
    g = sat_u8((y + 524288 - 852492 * vv - 409993 * uu) >> 20)
    b = sat_u8((y + 524288 + 2116026 * uu) >> 20)
    return b, g, r


def resolve(w, h, fmt, pitch=0, chroma_offset=0):
    """(pitch, chroma offset, bytes of one frame) with the zeros replaced by the tight values."""
    assert fmt in FORMATS and w % 2 == 0 and (fmt not in PLANAR or h % 2 == 0)
    if fmt in PLANAR:
        pitch = pitch or w
        coff = chroma_offset or pitch * h
        size = coff + (pitch * (h // 2) if fmt == "NV12" else (pitch // 2) * h)
        return pitch, coff, size
    pitch = pitch or 2 * w
    return pitch, 0, pitch * h


def frame_bytes(w, h, fmt, pitch=0, chroma_offset=0):
    return resolve(w, h, fmt, pitch, chroma_offset)[2]


def offsets(w, h, fmt, x, y, pitch=0, chroma_offset=0):
    """Byte offsets (of Y, of U, of V) of pixel (x, y) within one frame."""
    pitch, coff, _ = resolve(w, h, fmt, pitch, chroma_offset)
    if fmt == "NV12":
        c = coff + (y // 2) * pitch + (x // 2) * 2
        return y * pitch + x, c, c + 1
    if fmt == "I420":
        cp = pitch // 2
        u = coff + (y // 2) * cp + x // 2
        return y * pitch + x, u, u + cp * (h // 2)
    pair = y * pitch + (x // 2) * 4
    if fmt == "YUY2":  # Y0 U Y1 V
        return pair + 2 * (x & 1), pair + 1, pair + 3
    return pair + 1 + 2 * (x & 1), pair, pair + 2  # UYVY: U Y0 V Y1


def yuv_ref(buf, w, h, fmt, pitch=0, chroma_offset=0):
    """One frame (bytes-like, at least frame_bytes long) -> BGR u8 (h, w, 3), pixel by pixel."""
    buf = bytes(buf)
    out = np.empty((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            iy, iu, iv = offsets(w, h, fmt, x, y, pitch, chroma_offset)
            out[y, x] = pixel(buf[iy], buf[iu], buf[iv])
    return out


def plant(buf, w, h, fmt, x, y, yuv, pitch=0, chroma_offset=0):
    """Write the (Y, U, V) triple at pixel (x, y) of the frame in the uint8 array buf (the chroma pair is shared
    by the pixel's group, whose other pixels keep their own luma)."""
    iy, iu, iv = offsets(w, h, fmt, x, y, pitch, chroma_offset)
    buf[iy], buf[iu], buf[iv] = yuv


def random_frames(rng, n, w, h, fmt, pitch=0, chroma_offset=0, frame_stride=0):
    """n frames of random full-range bytes (the padding random too: nothing may read it) in one uint8 array,
    frame_stride (0: tight) apart, with the KAT triples planted one per pixel group as far as they fit."""
    size = frame_bytes(w, h, fmt, pitch, chroma_offset)
    stride = frame_stride or size
    buf = rng.integers(0, 256, (n - 1) * stride + size, dtype=np.uint8)
    gy = 2 if fmt in PLANAR else 1
    groups = [(x, y) for y in range(0, h, gy) for x in range(0, w, 2)]
    for f in range(n):
        fr = buf[f * stride: f * stride + size]
        for k, (yuv, _) in enumerate(KAT):
            if k >= len(groups):
                break
            gx, gyy = groups[(k * 7 + f) % len(groups)] if len(groups) > len(KAT) * 7 else groups[k]
            plant(fr, w, h, fmt, gx, gyy, yuv, pitch, chroma_offset)
    return buf
