"""Shapes and frames for the INTER_AREA resize variants (test_gpu_resize_content.py; proven in
test_pixel_content_host.py).

launch_resize_area picks k_resize_area_nt<NT> from the x table's maximal tap count: NT = (taps + 1) & ~1 up to 32,
so an odd count runs its instantiation with one zero-padded weight.  NT_CASES holds, for every NT = 2 .. 32 and
both tap counts NT - 1 and NT, a source width that gives that count at a destination BOX px wide, found by
counting computeResizeAreaTab's entries for every width; the tests assert the count from oracle_np.area_tab.
"""
import math

import numpy as np

import oracle
from oracle import oracle_np
import pixel_content as pc

BOX = 40       # destination width: a row of threads meets every byte misalignment and the window past the frame
ROWS = 3       # destination rows of the NT cases (a ragged last row pair)
S, T, NB = 2, 2, 2


def area_mode(W, H, box):
    """cv::resize(INTER_AREA)'s choice for imutils.resize(width=box): ("identity",), ("fast", isx, isy) for an
    integer scale on both axes, or ("general", the x table's maximal tap count)."""
    h = oracle.work_height(H, W, box)
    if (h, box) == (H, W):
        return ("identity",)
    sx, sy = 1.0 / (box / W), 1.0 / (h / H)
    assert sx >= 1 and sy >= 1
    isx, isy = int(round(sx)), int(round(sy))
    eps = np.finfo(float).eps
    if abs(sx - isx) < eps and abs(sy - isy) < eps:
        return ("fast", isx, isy)
    return ("general", max(len(e) for e in oracle_np.area_tab(W, box)))


def _tap_profile(W, box):
    """(the maximal entry count of computeResizeAreaTab(W -> box), the widest narrower end tap, in source px, of
    a column with that count), without building the table."""
    scale = 1.0 / (box / W)
    best, end = 0, 0.0
    for dx in range(box):
        f1 = dx * scale
        f2 = f1 + scale
        s2 = min(math.floor(f2), W - 1)
        s1 = min(math.ceil(f1), s2)
        lo, hi = s1 - f1, f2 - s2
        n = (lo > 1e-3) + (s2 - s1) + (hi > 1e-3)
        e = min(lo if lo > 1e-3 else 1.0, hi if hi > 1e-3 else 1.0)
        if n > best:
            best, end = n, e
        elif n == best:
            end = max(end, e)
    return best, end


def _source_height(W, box, rows):
    """The smallest H whose work height is `rows`."""
    H = rows * W // box
    while oracle.work_height(H, W, box) < rows:
        H += 1
    return H


def _nt_cases():
    """For every tap count 2 .. 32 the odd source width whose end taps weigh most (the narrowest of equals).  The first
    width with a count has it on two columns whose end taps cover 0.025 px, 0.1 % of the sum: a wrong byte in the
    last tap -- all that the tail load of k_resize_area_nt holds -- would seldom change an output there."""
    found = {}
    for W in range(BOX + 1, 33 * BOX, 2):  # odd widths: 3 W is odd, so the rows start at every byte alignment
        if W % BOX:
            t, end = _tap_profile(W, BOX)
            if t not in found or end > found[t][0]:
                found[t] = (end, W)
    return [(found[t][1], _source_height(found[t][1], BOX, ROWS), BOX, (t + 1) & ~1, t) for t in range(2, 33)]


NT_CASES = _nt_cases()   # (W, H, box, NT, taps)
# past 32 taps: the LDS-staged kernel (3 W % 16 == 0) and the plain one
ROWS_CASE = (1376, _source_height(1376, BOX, ROWS), BOX)
PLAIN_CASE = (1370, _source_height(1370, BOX, ROWS), BOX)
# k_resize_area_fast: (W, H, box, sx, sy).  3 x 3 and 5 x 5 take the float branch, 200 x 3 -> 100 x 1 is 2 x 3
# (h = int(3 * 0.5) = 1; not the (sum + 2) >> 2 of 2 x 2), 4 x 4 on noise has exact .5 ties
TIE_CASE = (160, 120, 40)
FAST_CASES = [(150, 45, 50, 3, 3), (250, 50, 50, 5, 5), (200, 3, 100, 2, 3), TIE_CASE + (4, 4)]


def case_id(c):
    return "x".join(str(v) for v in c[:2]) + f"-box{c[2]}" + (f"-nt{c[3]}-taps{c[4]}" if len(c) > 3 else "")


def frames(W, H, b):
    """Batch b of [T][S][H][W][3]: noise, the 1-px checkerboard and the dotted white / black frames of
    pixel_content.white, in a different order on each stream."""
    rng = np.random.default_rng([W, H, b])
    check = np.repeat(pc.checkerboard(H, W)[..., None], 3, -1)
    dotted = pc.white(W, H, 1, 6)[:, 0]  # kinds: black, white, white + dots, black, black + dots, white
    kinds = [["noise", "check"], ["check", "noise"]] if b == 0 else [["white_dots", "noise"], ["noise", "black_dots"]]
    out = np.empty((T, S, H, W, 3), np.uint8)
    for s in range(S):
        for t in range(T):
            kind = kinds[s][t]
            out[t, s] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if kind == "noise" else \
                check if kind == "check" else dotted[2] if kind == "white_dots" else dotted[4]
    return out


def tie_count(frame, n):
    """Outputs of the n x n integer-scale resize of `frame` whose mean is an exact .5 tie."""
    H, W, _ = frame.shape
    sums = frame[:H // n * n, :W // n * n].reshape(H // n, n, W // n, n, 3).astype(np.int64).sum(axis=(1, 3))
    return int((2 * sums % (n * n) == 0).sum() - (sums % (n * n) == 0).sum())
