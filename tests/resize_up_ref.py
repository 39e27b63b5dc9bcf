"""cv2.resize(..., INTER_AREA) with a destination larger than the source, restated in numpy.

OpenCV takes the area paths only when both scales are >= 1; otherwise INTER_AREA runs the 8-bit bilinear
resizer with "area mode" taps.  Only the tap rule differs from INTER_LINEAR (yolo_ref.linear_taps); the
fixed-point stages are those of yolo_ref.resize_linear_u8.  A restatement from knowledge of resize.cpp:
parity to cv2 itself is not pinned by any test here."""
from __future__ import annotations

import math

import numpy as np


def area_up_taps(ssize: int, dsize: int):
    """One axis: first tap, second tap (clamped), the two short coefficients (a0 + a1 == 2048)."""
    s0, s1, a0, a1 = [], [], [], []
    inv = float(dsize) / float(ssize)
    scale = 1.0 / inv
    for d in range(dsize):
        sx = int(math.floor(d * scale))
        fx = np.float32((d + 1) - (sx + 1) * inv)
        fx = np.float32(0) if fx <= 0 else np.float32(fx - np.floor(fx))
        if sx < 0:
            sx, fx = 0, np.float32(0)
        if sx >= ssize - 1:
            sx, fx = ssize - 1, np.float32(0)
        s0.append(sx)
        s1.append(min(sx + 1, ssize - 1))
        a0.append(int(np.rint(np.float32(np.float32(1) - fx) * np.float32(2048))))
        a1.append(int(np.rint(fx * np.float32(2048))))
    return np.array(s0), np.array(s1), np.array(a0, np.int64), np.array(a1, np.int64)


def up_height(H: int, W: int, box: int) -> int:
    """imutils.resize(frame, width=box): the height it asks cv2.resize for."""
    return int(H * (box / float(W)))


def resize_area_up_u8(img: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """cv2.resize(img, (dw, dh), interpolation=INTER_AREA) for uint8 [H, W, C] with dw > W or dh > H."""
    H, W = img.shape[:2]
    if (H, W) == (dh, dw):
        return img.copy()
    x0, x1, a0, a1 = area_up_taps(W, dw)
    y0, y1, b0, b1 = area_up_taps(H, dh)
    S = img.astype(np.int64)
    D = S[:, x0] * a0[None, :, None] + S[:, x1] * a1[None, :, None]  # [H, dw, C]
    D0, D1 = D[y0], D[y1]
    v = (((b0[:, None, None] * (D0 >> 4)) >> 16) + ((b1[:, None, None] * (D1 >> 4)) >> 16) + 2) >> 2
    return v.astype(np.uint8)
