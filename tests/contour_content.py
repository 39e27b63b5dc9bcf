"""Masks for the contour pass (fm_ccl.hip), painted exactly on any pixel path, with the conditions that prove them.

The adversarial masks of the other modules are painted with ksize 1, which past 16,384 pixels is the "fused" path:
k_fused dilates itself and the contour chain runs k_tile_ccl<false>.  The product chain -- k_pix5, k_tile_flags,
k_regions<true>, k_tile_ccl<true> with dilate_tile's eight halo reads, k_tile_heavy, k_merge, k_fold, k_emit,
k_counts -- saw smooth pictures only.  Here a mask is painted through the keep-mask instead of through the
frame, which works behind a Gaussian of any size.

  painter       A black frame, then white ones, threshold 0, avg 0.0 and a keep-mask equal to the pattern: the
                masked blur is 255 on the pattern and 0 elsewhere, the background stays 0, so the stored
                threshold bits are the pattern and the mask is dilate5(pattern).  paint_frames() makes the
                frames and keep-masks of one batch, tile_bits() the engine's threshold_bits layout.
  class model   tile_classes(dilated mask): for every 64 x 64 tile the way tile_ccl handles it -- empty, full,
                simple, compact, light, heavy -- with the run counts the decision is taken on.  Restated from
                tile_ccl, simple_tile and compact_tile of fm_ccl.hip as they stand (test code about this
                project's own kernel).  The only observable of it on an engine is ccl_stats()["heavy_tiles"],
                which every GPU case compares with the model's count.
  boundary      tiles at the class boundaries (64 | 65 compact runs, 256 | 257 runs, a heavy tile with distinct
                rows, simple_tile's variants and near-misses), built inside one tile by construction and a
                search over one parameter; the counts always come from tile_classes on oracle.dilate5.
  seams         contacts, rings, serpentines and regions laid across the tile edges at 64 and 128.
  ccl           masks aimed at the pixel-level labelling of fm_kernels.hip (k_ccl_*): diagonal contacts across the
                corners of its 32 x 32 blocks that are no tile corners, a frame on the image border whose hole
                reaches the border through a 1-px channel (4-connected background, k_ccl_outer's four segments,
                k_ccl_roots' left-neighbour test), islands inside holes.
  overlay       a pattern on a dot lattice of pitch 6, the dots within 6 px of the pattern left out: the frames that
                exhaust the tile pass's union-find nodes, so that relabel_frame labels adversarial pictures.

test_contour_content_host.py and test_pixel_ccl_host.py assert every stated class, count and contour outcome on the oracle alone;
test_gpu_contour_content.py and test_gpu_pixel_ccl.py run the same sets through engines and compare bit for bit.
"""
import functools
import pathlib
import re

import numpy as np

import oracle
from test_gpu_contour_points import spiral
from test_gpu_tile_flags import _bits_from_mask

TS = 64
COMPACT_MAX, LIGHT_MAX, HEAVY_MAX = 64, 256, 1600  # compact_tile's lanes, LIGHT, kTileMaxRuns
CLASSES = ("empty", "full", "simple", "compact", "light", "heavy")

# W, H of the GPU module's cases.  CHAIN: 6 x 5 = 30 tiles with a 4-px last tile column and row (the kernel
# chain); FRAME: 4 x 3 = 12 tiles (k_frame_contours); SMALL: 12,288 pixels (the small-image path); the CUT shapes
# have w % 64 and h % 64 in {1, 2, 63} and 30 tiles.
CHAIN, FRAME, SMALL = (324, 260), (200, 136), (128, 96)
CUTS = ((321, 258), (322, 319), (383, 257))
FOUR_WAVE = (1024, 512)


# ------------------------------------------------------------------------------------------------------------
# painter

def paint_frames(patterns):
    """patterns: S bool / 0-1 arrays [H][W] -> (frames uint8 [2][S][H][W][3]: black, then white; the S keep-masks).
    On an engine (or oracle stream) with threshold 0 and avg 0.0 whose stream s has keep-mask s, frame 1's mask is
    dilate5(patterns[s]) whatever the Gaussian size; frame 0's is empty (it initialises the background to 0, or
    meets the 0 an earlier batch left)."""
    H, W = patterns[0].shape
    fr = np.zeros((2, len(patterns), H, W, 3), np.uint8)
    fr[1] = 255
    return fr, [np.ascontiguousarray(p, dtype=np.uint8) for p in patterns]


def tile_bits(pattern):
    """uint64 [ntiles][64]: the engine's threshold_bits of a frame whose threshold mask is `pattern`."""
    return _bits_from_mask(np.asarray(pattern, bool))


def dilated(pattern):
    """The oracle's 5 x 5 dilation of a 0 / 1 pattern, as the 0 / 255 mask the engine returns."""
    return oracle.dilate5((np.asarray(pattern) != 0).astype(np.uint8) * 255)


# ------------------------------------------------------------------------------------------------------------
# class model

def _tiles(mask):
    """(ty, tx) -> bool [64][64] of every tile of a mask; pixels past the image are zero."""
    h, w = mask.shape
    nty, ntx = -(-h // TS), -(-w // TS)
    pad = np.zeros((nty * TS, ntx * TS), bool)
    pad[:h, :w] = mask != 0
    return {(ty, tx): pad[ty * TS:(ty + 1) * TS, tx * TS:(tx + 1) * TS] for ty in range(nty) for tx in range(ntx)}


def row_runs(t):
    """Runs of every row, foreground and background: bit 0 always starts one."""
    return 1 + (t[:, 1:] != t[:, :-1]).sum(1)


def run_counts(t):
    """(compact runs, total runs): compact_tile counts the runs of the rows that differ from the row above (row 0
    always counts), tile_ccl the runs of every row."""
    runs = row_runs(t)
    distinct = np.ones(TS, bool)
    distinct[1:] = (t[1:] != t[:-1]).any(1)
    return int(runs[distinct].sum()), int(runs.sum())


def pair_count(t):
    """tile_ccl's `np`: over the runs B of every row below the first, the same-colour runs of the row above that B
    touches -- the window [b0 - 1, b1 + 1] for foreground (8-connected), [b0, b1] for background.  The labelling
    refuses a tile at np > 2 * CAP as it does at total > CAP."""
    n = 0
    for r in range(1, TS):
        up, row = t[r - 1], t[r]
        starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
        ends = np.r_[starts[1:] - 1, TS - 1]
        upid = np.cumsum(np.r_[True, up[1:] != up[:-1]]) - 1  # run index of every pixel of the row above
        for b0, b1 in zip(starts, ends):
            fg = bool(row[b0])
            w0, w1 = (max(b0 - 1, 0), min(b1 + 1, TS - 1)) if fg else (b0, b1)
            hits = np.flatnonzero(up[w0:w1 + 1] == fg)
            if len(hits):
                n += (int(upid[w0 + hits[-1]]) - int(upid[w0 + hits[0]])) // 2 + 1
    return n


def simple_roots(t):
    """simple_tile's root count of a tile, or None where one of its conditions fails before the count: at most one
    foreground run per row, the rows that have one consecutive (r0..r1), each run touching the one above 8-wise.
    The count: the chains of background runs left (x 0 .. xs - 1) and right (xe + 1 .. 63) of the foreground start
    a root each, but for the chains through row r0 (the top region's, whose root is row 0's run) and through row
    r1 (the bottom region's, rooted at its earliest run -- or the top region's, where a chain spans the band)."""
    prev = np.zeros_like(t)
    prev[:, 1:] = t[:, :-1]
    nfg = (t & ~prev).sum(1)
    if (nfg > 1).any() or not (nfg == 1).any():
        return None
    rows = np.flatnonzero(nfg == 1)
    r0, r1 = int(rows[0]), int(rows[-1])
    if len(rows) != r1 - r0 + 1:
        return None
    xs = {r: int(np.argmax(t[r])) for r in rows}
    xe = {r: TS - 1 - int(np.argmax(t[r][::-1])) for r in rows}
    for r in range(r0 + 1, r1 + 1):
        if not (xs[r] <= xe[r - 1] + 1 and xe[r] >= xs[r - 1] - 1):
            return None
    Lm = [r0 <= r <= r1 and xs[r] > 0 for r in range(TS)]
    Rm = [r0 <= r <= r1 and xe[r] < TS - 1 for r in range(TS)]
    Ls = [Lm[r] and not (r > 0 and Lm[r - 1]) for r in range(TS)]
    Rs = [Rm[r] and not (r > 0 and Rm[r - 1]) for r in range(TS)]
    top, bot = r0 > 0, r1 < TS - 1
    merge = top and bot and (all(Lm[r0:r1 + 1]) or all(Rm[r0:r1 + 1]))
    L1, R1 = Lm[r1], Rm[r1]
    sL1 = max(r for r in range(r1 + 1) if Ls[r]) if L1 else 0
    sR1 = max(r for r in range(r1 + 1) if Rs[r]) if R1 else 0
    RL = {r for r in range(TS) if Ls[r]}
    RR = {r for r in range(TS) if Rs[r]}
    if top:
        RL.discard(r0)
        RR.discard(r0)
        RL.add(0)
    if bot:
        if L1:
            RL.discard(sL1)
        if R1:
            RR.discard(sR1)
    if bot and not merge:
        lt, rt = L1 and not (top and sL1 == r0), R1 and not (top and sR1 == r0)
        brow, bright = r1 + 1, False
        if rt and sR1 < brow:
            brow, bright = sR1, True
        if lt and sL1 <= brow:
            brow, bright = sL1, False
        (RR if bright else RL).add(brow)
    return len(RL) + len(RR) + 1


def tile_class(t):
    """(class, compact runs, total runs) of one tile, in tile_ccl's order.  "over" is a tile no pass labels (the
    frame would fall back to the pixel-level labelling); no mask of this module may hold one."""
    if not t.any():
        return "empty", 1, TS
    if t.all():
        return "full", 1, TS
    compact, total = run_counts(t)
    n = simple_roots(t)
    if n is not None and n <= 64:
        return "simple", compact, total
    if compact <= COMPACT_MAX:
        return "compact", compact, total
    pairs = pair_count(t)
    if total <= LIGHT_MAX and pairs <= 2 * LIGHT_MAX:
        return "light", compact, total
    if total <= HEAVY_MAX and pairs <= 2 * HEAVY_MAX:
        return "heavy", compact, total
    return "over", compact, total


def tile_classes(dilated_mask):
    """(ty, tx) -> (class, compact runs, total runs) for every 64 x 64 tile of a dilated mask."""
    return {k: tile_class(t) for k, t in _tiles(dilated_mask).items()}


def histogram(classes):
    return {c: sum(1 for v in classes.values() if v[0] == c) for c in CLASSES + ("over",)}


# ------------------------------------------------------------------------------------------------------------
# patterns: points relative to a tile's origin, clipped to the image

def _canvas(shape):
    W, H = shape
    return np.zeros((H, W), np.uint8)


def _put(p, ty, tx, pts):
    H, W = p.shape
    for r, c in pts:
        y, x = ty * TS + r, tx * TS + c
        if 0 <= y < H and 0 <= x < W:
            p[y, x] = 1
    return p


def _diag(r0, n, c0):
    """n pixels going down and right from (r0, c0): dilated, every row it covers differs from the one above"""
    return [(r0 + i, c0 + i) for i in range(n)]


def _vline(c, r0=-2, r1=TS + 2):
    return [(r, c) for r in range(r0, r1)]


def t_compact(c0):
    """One diagonal of 18 pixels -- 22 distinct rows of 3 runs, less one run for every row that reaches column 63
    -- and a dot below it, so that the rows with a foreground run are not consecutive (not simple)"""
    return _diag(20, 18, c0) + [(52, 10)]


def t_total(c0):
    """A diagonal across the whole tile and a second one of 36 pixels right of it, starting at column c0: two runs
    more on each of its 40 rows, less one for every row that reaches column 63 (five rows at once, then one
    more for each column further right)"""
    return _diag(-2, TS + 4, 1) + _diag(10, 36, c0)


def t_heavy(phase):
    """Dots at x-pitch 6 on rows at pitch 5, each row of dots shifted by 1: 5-px squares stacked without a gap,
    every row of the tile different from the one above"""
    return [(r, c) for r in range(-5, TS + 5) if r % 5 == 0 for c in range(-6, TS + 6) if (c - r // 5 + phase) % 6 == 0]


def t_teeth():
    """A filled body with 5-px teeth on column 0 every 6 rows and on column 63 likewise, 3 rows lower: every tooth
    gap starts a background chain of one row, the most roots a dilated tile gives simple_tile"""
    body = [(r, c) for r in range(-2, TS + 2) for c in range(5, 59)]
    return body + [(3 + 6 * j, 0) for j in range(11)] + [(6 + 6 * j, TS - 1) for j in range(10)]


def t_slope():
    """A thick line from the tile's left edge down to its right edge: top and bottom regions that no chain joins"""
    return [(10 + (c + 2) * 40 // 68, c) for c in range(-2, TS + 3)]


# name -> (tile points, stated class, compact runs, total runs); None where the count is not the point
BOUNDARY = {
    "full":             ([(r, c) for r in range(-2, TS + 2) for c in range(-2, TS + 2)], "full", None, None),
    "simple_all_rows":  (_vline(30), "simple", None, None),                 # r0 = 0, r1 = 63: no top, no bottom
    "simple_from_top":  (_vline(30, -2, 31), "simple", None, None),         # r0 = 0 with a bottom region
    "simple_to_bottom": (_vline(30, 30), "simple", None, None),             # r1 = 63 with a top region
    "simple_diagonal":  ([(20, 20), (25, 25)], "simple", None, None),       # xs == xe_above + 1
    "simple_near_miss": ([(20, 20), (25, 26)], "compact", None, None),      # xs == xe_above + 2: two components
    "simple_diag_left": ([(20, 25), (25, 20)], "simple", None, None),       # xe == xs_above - 1
    "simple_miss_left": ([(20, 26), (25, 20)], "compact", None, None),
    "simple_left_chain": ([(30, 61)], "simple", None, None),                # xe = 63: the left chain spans the band
    "simple_right_chain": ([(30, 2)], "simple", None, None),                # xs = 0: the right chain does
    "simple_both_chains": ([(30, 30)], "simple", None, None),
    "simple_slope":     (t_slope(), "simple", None, None),                  # top and bottom regions stay apart
    "simple_slope_up":  ([(r, TS - 1 - c) for r, c in t_slope()], "simple", None, None),  # mirrored: a right-run root
    "simple_teeth":     (t_teeth(), "simple", None, None),
    "simple_col63":     ([(30, TS + 1)], "simple", None, None),             # a foreground run on column 63 only
    "simple_col0":      ([(30, -2)], "simple", None, None),                 # ... on column 0 only
}
TEETH_ROOTS = 23          # simple_teeth's root count: 11 left chains, 11 right chains and the foreground
# The `nroots > 64` exit of simple_tile is out of a dilated mask's reach: a background run on column 0 between two
# rows whose foreground starts at column 0 needs 5 rows of foreground on either side (a 5 x 5 square each), so the
# left chains start at least 6 rows apart, the right ones too: at most 11 + 11 + 1 roots.


def _home_counts(points):
    """(class, compact runs, total runs) of tile (1, 1) of a 3 x 3-tile image that holds `points`"""
    return tile_classes(dilated(_put(_canvas((3 * TS, 3 * TS)), 1, 1, points)))[(1, 1)]


def _search(make, target, values, which):
    """The first parameter whose tile has `target` compact (which = 1) or total (2) runs by tile_classes on the
    oracle's dilation."""
    for v in values:
        if _home_counts(make(v))[which] == target:
            return v
    raise AssertionError(f"no parameter reaches {target}")


HEAVY_ROWS_RUNS = 1412    # the runs heavy_rows reaches in an interior tile (fm_internal.h's bound is 24 x 64 = 1,536)


@functools.lru_cache(None)
def searched():
    """name -> (tile points, stated class, compact runs, total runs) of the tiles found by search"""
    out = {}
    for n, cls in ((64, "compact"), (65, "light")):
        out[f"compact_{n}"] = (t_compact(_search(t_compact, n, range(30, 60), 1)), cls, n, None)
    for n, cls in ((256, "light"), (257, "heavy")):
        out[f"total_{n}"] = (t_total(_search(t_total, n, range(20, 60), 2)), cls, None, n)
    phase = max(range(30), key=lambda ph: _home_counts(t_heavy(ph))[2])
    out["heavy_rows"] = (t_heavy(phase), "heavy", None, HEAVY_ROWS_RUNS)
    return out


def boundary_table():
    return {**BOUNDARY, **searched()}


def home_tile(shape):
    """The tile the boundary tiles are built in: (1, 1), or (0, 0) where that tile is cut by the image"""
    W, H = shape
    return (1, 1) if W >= 2 * TS and H >= 2 * TS else (0, 0)


# the boundary tiles whose stated class and counts survive at tile (0, 0) of SMALL (no rows above, no columns left)
SMALL_NAMES = ("full", "simple_from_top", "simple_to_bottom", "simple_diagonal", "simple_near_miss",
               "simple_diag_left", "simple_miss_left", "simple_left_chain", "simple_both_chains", "simple_col63",
               "compact_64", "compact_65", "heavy_rows")


def boundary_set(shape):
    """[(name, pattern, (ty, tx), class, compact, total)]: every boundary tile alone in its home tile"""
    ty, tx = home_tile(shape)
    tab = boundary_table()
    names = SMALL_NAMES if shape == SMALL else list(tab)
    out = [(n, _put(_canvas(shape), ty, tx, tab[n][0]), (ty, tx)) + tab[n][1:] for n in names]
    if shape == SMALL:  # (on the image's corner heavy_rows has fewer runs: the class is stated, not the count)
        out = [c[:5] + (None,) if c[0] == "heavy_rows" else c for c in out]
    return out


def cut_set(shape):
    """[(name, pattern, (ty, tx), class or None)]: simple_tile's variants in the tiles the image cuts -- the last
    tile column (w % 64 columns wide), the last tile row (h % 64 rows), the corner tile -- a run on column 63 only
    in the tile left of the last column, the heavy lattice in cut tiles (heavy at 63 rows or columns), and the
    mixed frame, which gives the set every class"""
    W, H = shape
    lx, ly = (W - 1) // TS, (H - 1) // TS
    vw, vh = W - lx * TS, H - ly * TS
    out = []

    def add(name, ty, tx, pts, cls="simple"):
        out.append((name, _put(_canvas(shape), ty, tx, pts), (ty, tx), cls))

    add("cut_right_row", 1, lx, [(30, c) for c in range(-2, vw)])            # a horizontal bar into the last column
    add("cut_right_all_rows", 1, lx, _vline(0))                              # r0 = 0, r1 = 63 on its column 0
    add("cut_bottom_all_rows", ly, 1, _vline(30))                            # r1 = the image's last row
    add("cut_bottom_dot", ly, 1, [(vh - 1, 30)])
    add("cut_corner_dot", ly, lx, [(vh - 1, vw - 1)])
    add("cut_corner_left", ly, lx - 1, [(vh - 1, TS - 1)])                   # spills into the corner tile
    add("cut_col63", 1, lx - 1, [(30, TS + min(1, vw - 1))])                 # column 63 only (62 and 63 at vw = 1)
    add("cut_teeth", 1, lx - 1, t_teeth())                                   # right teeth spill into the last column
    add("cut_bottom_teeth", ly - 1, 1, t_teeth())
    add("cut_bottom_heavy", ly, 1, searched()["heavy_rows"][0], "heavy" if vh == 63 else None)
    add("cut_right_heavy", 1, lx, searched()["heavy_rows"][0], "heavy" if vw == 63 else None)
    out.append(("cut_mixed", mixed(shape), None, None))
    return out


# ------------------------------------------------------------------------------------------------------------
# seam topologies: [(name, pattern, contour count)]

def _rect(p, y0, x0, y1, x1, skip=()):
    """The 1-px outline of a rectangle, but for the pixels of `skip`"""
    for x in range(x0, x1 + 1):
        p[y0, x] = p[y1, x] = 1
    for y in range(y0, y1 + 1):
        p[y, x0] = p[y, x1] = 1
    for y, x in skip:
        p[y, x] = 0
    return p


def _dot(p, y, x):
    p[y, x] = 1
    return p


def corner_dots(shape, anti):
    """Two dots whose 5 x 5 squares touch only diagonally across every four-tile corner that has 5 px around it:
    rows 59..63 against rows 64..68; cols likewise (anti: the square above lies right of the one below)"""
    W, H = shape
    p = _canvas(shape)
    n = 0
    for cy in range(TS, H - 4, TS):
        for cx in range(TS, W - 4, TS):
            _dot(p, cy - 3, cx + 2 if anti else cx - 3)
            _dot(p, cy + 2, cx - 3 if anti else cx + 2)
            n += 1
    return p, n


def ring_diagonal(shape, gap):
    """A ring whose top-left corner lies on the four-tile corner (64, 64): its top bar's first square (rows 59..63,
    from column 64) touches its left side's first square (rows 64..68, columns 59..63) only diagonally.  gap = 1
    starts the top bar one pixel later: a "C".  A dot inside, its raster-first pixel on column 0 of tile (1, 2)
    (REF_EDGE), a dot outside on column 0 of tile (0, 1), and one on the image's column 0 (REF_OUTER)."""
    W, H = shape
    p = _canvas(shape)
    y0 = x0 = 61
    y1, x1 = min(H - 14, 3 * TS + 40), min(W - 40, 4 * TS + 20)
    for x in range(x0 + 5 + gap, x1 + 1):
        p[y0, x] = 1
    for y in range(y0 + 5, y1 + 1):
        p[y, x0] = 1
    for x in range(x0, x1 + 1):
        p[y1, x] = 1
    for y in range(y0, y1 + 1):
        p[y, x1] = 1
    _dot(p, 90, 2 * TS + 2)     # inside
    _dot(p, 20, TS + 2)         # outside, REF_EDGE
    _dot(p, 30, 1)              # outside, REF_OUTER
    return p


def serpentine(shape):
    """One line through every tile: a row through each tile row, joined at alternating ends"""
    W, H = shape
    p = _canvas(shape)
    ys = [min(ty * TS + 32, H - 2) for ty in range(-(-H // TS))]
    for i, y in enumerate(ys):
        p[y, 2:W - 2] = 1
        if i:
            x = W - 3 if i % 2 else 2
            p[ys[i - 1]:y + 1, x] = 1
    return p


def spiral_in(shape):
    """test_gpu_contour_points.spiral at the largest size the shape holds"""
    W, H = shape
    p = _canvas(shape)
    size = min(W, H)
    p[:size, :size] = spiral(size) != 0
    return p


def nested_rings(shape):
    """Three rings, 14 px apart, around a dot"""
    W, H = shape
    p = _canvas(shape)
    for i in range(3):
        _rect(p, 10 + 14 * i, 10 + 14 * i, H - 11 - 14 * i, W - 11 - 14 * i)
    return _dot(p, H // 2, W // 2)


def wide_ring(shape, gap):
    """A ring around 2 x 3 whole tiles (needs 5 x 5 tiles): the tiles of its hole are empty and not candidates, a
    region that does not reach the grid border, but for tile (1, 1), which holds a dot.  gap: 8 px of the top bar
    left out, which opens the hole.  A dot outside the ring, below it."""
    W, H = shape
    assert W > 4 * TS + 50 and H > 4 * TS
    skip = [(20, x) for x in range(150, 158)] if gap else ()
    p = _rect(_canvas(shape), 20, 20, 4 * TS - 17, 5 * TS - 17, skip)
    _dot(p, 100, 100)
    return _dot(p, H - 3, 160)


def halo(shape):
    """Tile (1, 1) holds no threshold bit of its own: its dilated mask comes from all eight neighbours, dots
    every 6 px on the rows and columns next to its edges (two rows / columns deep on two sides, one on the
    others) and one in each diagonal neighbour's corner"""
    p = _canvas(shape)
    for i in range(1, TS, 6):
        _put(p, 1, 1, [(-1, i), (TS + 1, i), (i, -2), (i, TS)])
    return _put(p, 1, 1, [(-1, -1), (-2, TS + 1), (TS, -2), (TS + 1, TS)])


def mixed(shape, at=(0, 0)):
    """All six classes in the 2 x 3 tiles from tile `at`: simple, compact, light / full, heavy, empty"""
    ty, tx = at
    tab = boundary_table()
    p = _canvas(shape)
    for dy, dx, name in ((0, 0, "simple_slope"), (0, 1, "compact_64"), (0, 2, "total_256"), (1, 0, "full"),
                         (1, 1, "heavy_rows")):
        # (pixels 2 .. 61 only: dilated, they fill their own tile to its edges and leave the neighbours alone)
        _put(p, ty + dy, tx + dx, [q for q in tab[name][0] if 2 <= q[0] < TS - 2 and 2 <= q[1] < TS - 2])
    return p


def mixed_tiled(shape):
    """`mixed` repeated over the image, every second block of 2 x 3 tiles"""
    W, H = shape
    p = _canvas(shape)
    for ty in range(0, H // TS - 1, 2):
        for tx in range(0, W // TS - 2, 3):
            if (ty // 2 + tx // 3) % 2 == 0:
                p |= mixed(shape, (ty, tx))
    return p


def four_wave_set():
    """[(name, pattern)] for 8 streams of FOUR_WAVE: the mixed block at a different tile offset in every stream, and
    in the last one repeated over the image"""
    out = [(f"mixed_{s}", mixed(FOUR_WAVE, ((s % 4) * 2, (s % 5) * 3))) for s in range(7)]
    return out + [("mixed_tiled", mixed_tiled(FOUR_WAVE))]


def seam_set(shape):
    """[(name, pattern, external contours)] at a shape of at least 3 x 2 tiles"""
    out = []
    for anti in (False, True):
        p, n = corner_dots(shape, anti)
        out.append(("corner_anti" if anti else "corner_main", p, n))
    out.append(("ring_diagonal", ring_diagonal(shape, 0), 3))      # the ring and the two dots outside
    out.append(("ring_open", ring_diagonal(shape, 1), 4))          # ... and the dot inside the "C"
    out.append(("serpentine", serpentine(shape), 1))
    out.append(("spiral", spiral_in(shape), 1))
    out.append(("nested_rings", nested_rings(shape), 1))
    if shape == CHAIN:
        out.append(("wide_ring", wide_ring(shape, False), 2))      # the ring and the dot below it
        out.append(("wide_ring_open", wide_ring(shape, True), 3))
    out.append(("halo", halo(shape), None))
    out.append(("mixed", mixed(shape), None))
    return out


# ------------------------------------------------------------------------------------------------------------
# masks for the pixel-level labelling (fm_kernels.hip: 32 x 32 blocks): [(name, pattern, contour count)]

CB = 32                   # kCclBlock
NOTCH_SIDES = ("top", "bottom", "left", "right")
NOTCH_CORNERS = ("top_left", "top_right", "bottom_left", "bottom_right")


def block_corner_dots(shape, anti):
    """corner_dots at the four-block corners of the 32-px blocks that are no tile corners (x and y odd multiples
    of 32): the two 5 x 5 squares touch only diagonally across the corner, so one of k_ccl_merge's diagonal links
    is the component's only connection"""
    W, H = shape
    p = _canvas(shape)
    n = 0
    for cy in range(CB, H - 4, 2 * CB):
        for cx in range(CB, W - 4, 2 * CB):
            _dot(p, cy - 3, cx + 2 if anti else cx - 3)
            _dot(p, cy + 2, cx - 3 if anti else cx + 2)
            n += 1
    return p, n


def _hole_dots(p, pitch=24, first=10):
    """Dots on a grid inside a frame on the image border (a 1-px gap at least to the frame's dilation, rows and
    columns 0 .. 4 and the last five); returns their number"""
    H, W = p.shape
    n = 0
    for y in range(first, H - first, pitch):
        for x in range(first, W - first, pitch):
            _dot(p, y, x)
            n += 1
    return n


def _notch_top(shape, at, is_open):
    """The frame with its opening at column `at` of the top side (None: the top-left corner)"""
    W, H = shape
    p = _rect(_canvas(shape), 2, 2, H - 3, W - 3)
    if is_open and at is not None:
        p[2, at - 2:at + 3] = 0           # dilated: columns at - 1 and at + 1 stay set on rows 0 .. 4, column at is zero
    elif is_open:
        # the corner: the left bar moves to column 0 on rows 3 .. 9 (dilated: columns 0 .. 2 from row 1) and the top
        # bar starts at column 6 (columns 4 ..): row 0 up to column 3 and column 3 down to row 4 stay zero
        p[2:8, 2] = 0
        p[2, 2:6] = 0
        p[3:10, 0] = 1
    return p, _hole_dots(p)


def border_notch(shape, where, is_open, pos=1):
    """(pattern, dots, zero border pixels [(y, x)]).  A frame (pattern rows / columns 2 and the last but two) whose
    dilation covers the image border all round, around a grid of dots.  Closed, the dots are not external: one
    contour.  Open, the hole's background reaches the border through one channel 1 px wide, and every dot is
    external.  where = a side: the channel is straight, 5 px long, and exactly one border pixel is zero; pos 0, 1, 2
    puts it near the side's start, on a 32-px block edge near its middle, near its end.  where = a corner: the
    corner pixel is zero.  (A dilated mask cannot open a corner with two zero border pixels: the square that sets
    the third one, (1, 0) at the top-left corner, has its centre on row 3 and sets (1, 1) too, which shuts the
    corner pixel and its neighbour off.)  The channel runs from the corner pixel along row 0 to column 3 and down
    column 3: four zero border pixels, 1 px wide all the way."""
    W, H = shape
    side = where.split("_")[0] if where in NOTCH_CORNERS else where
    flip_x = where.endswith("right") and where in NOTCH_CORNERS
    if where in NOTCH_CORNERS:
        p, n = _notch_top(shape, None, is_open)
        zero = [(0, x) for x in range(4)] if is_open else []
        if side == "bottom":
            p, zero = p[::-1], [(H - 1 - y, x) for y, x in zero]
        if flip_x:
            p, zero = p[:, ::-1], [(y, W - 1 - x) for y, x in zero]
        return np.ascontiguousarray(p), n, zero
    length = W if side in ("top", "bottom") else H
    at = (7, (length // 2) // CB * CB, length - 8)[pos]
    if side in ("top", "bottom"):
        p, n = _notch_top(shape, at, is_open)
        zero = [(0, at)] if is_open else []
        if side == "bottom":
            p, zero = p[::-1], [(H - 1, at)] if is_open else []
    else:
        p, n = _notch_top((H, W), at, is_open)
        p = p.T
        zero = [(at, 0)] if is_open else []
        if side == "right":
            p, zero = p[:, ::-1], [(at, W - 1)] if is_open else []
    return np.ascontiguousarray(p), n, zero


def islands(shape):
    """nested_rings with dots in every hole: between the outer and the middle ring (inside a ring's hole), between
    the middle and the inner ring (inside a ring that is itself inside a ring's hole) and inside the innermost.
    Only the outer ring is external.  Returns (pattern, dots)."""
    W, H = shape
    p = nested_rings(shape)
    n = 1
    for i in (0, 1):                      # 9 zero pixels between two rings' dilations: a dot's square and 2 px each side
        y0, x0, y1, x1 = 17 + 14 * i, 17 + 14 * i, H - 18 - 14 * i, W - 18 - 14 * i
        for x in range(x0, x1 + 1, 12):
            _dot(p, y0, x)
            _dot(p, y1, x)
            n += 2
        for y in range(y0 + 12, y1 - 6, 12):
            _dot(p, y, x0)
            _dot(p, y, x1)
            n += 2
    for y in range(46, H - 46, 12):
        for x in range(46, W - 46, 12):
            if abs(y - H // 2) > 6 or abs(x - W // 2) > 6:
                _dot(p, y, x)
                n += 1
    return p, n


@functools.lru_cache(None)
def notch_table(shape):
    """name -> (pattern, dots, zero border pixels, open) of every border_notch case of a shape"""
    out = {"notch_closed": border_notch(shape, "top", False) + (False,)}
    for side in NOTCH_SIDES:
        for pos, at in enumerate(("start", "middle", "end")):
            out[f"notch_{side}_{at}"] = border_notch(shape, side, True, pos) + (True,)
    for corner in NOTCH_CORNERS:
        out[f"notch_{corner}"] = border_notch(shape, corner, True) + (True,)
    return out


def ccl_set(shape):
    """[(name, pattern, external contours)] at a shape of at least 128 x 128"""
    out = []
    for anti in (False, True):
        p, n = block_corner_dots(shape, anti)
        out.append(("block_corner_anti" if anti else "block_corner_main", p, n))
    for name, (p, dots, zero, is_open) in notch_table(shape).items():
        out.append((name, p, 1 + dots if is_open else 1))
    out.append(("islands", islands(shape)[0], 1))
    return out


# ------------------------------------------------------------------------------------------------------------
# overlays: the frames of the pool-exhaustion cases (painted through the frame itself at ksize 1)

LATTICE_PITCH, CLEARANCE = 6, 6


def lattice(shape, offset):
    """Single-pixel dots at pitch 6 from (offset, offset): dilated, 5 x 5 squares with 1-px gaps"""
    p = _canvas(shape)
    p[offset % LATTICE_PITCH::LATTICE_PITCH, offset % LATTICE_PITCH::LATTICE_PITCH] = 1
    return p


def overlay(pattern, offset=0):
    """pattern | lattice, without the lattice dots within a Chebyshev distance of 6 of a pattern pixel (three 5 x 5
    dilations): a 2-px gap at least between a dot's square and the pattern's dilation, so the pattern's contours
    stay contours of the frame"""
    H, W = pattern.shape
    near = (np.asarray(pattern) != 0).astype(np.uint8) * 255
    for _ in range(CLEARANCE // 2):
        near = oracle.dilate5(near)
    return ((pattern != 0) | ((lattice((W, H), offset) != 0) & (near == 0))).astype(np.uint8)


def overlay_sources(shape):
    """[(name, pattern)]: seam_set and a pick of ccl_set, the pictures the overlays cycle"""
    pick = ("block_corner_main", "block_corner_anti", "islands", "notch_top_middle", "notch_bottom_right",
            "notch_closed")
    return [(c[0], c[1]) for c in seam_set(shape)] + [(c[0], c[1]) for c in ccl_set(shape) if c[0] in pick]


def fallback_frames(shape, n, every, first=0):
    """[(name, pattern)] of an n-frame batch that exhausts the tile pass's nodes: a black frame, then pure lattices
    (offset = the frame's index) but for every `every`-th frame, an overlay; the overlays cycle overlay_sources
    from its entry `first`"""
    src = overlay_sources(shape)
    out, k = [("black", _canvas(shape))], first
    for t in range(1, n):
        if t % every == 0:
            name, p = src[k % len(src)]
            out.append((f"overlay_{name}_{t % LATTICE_PITCH}", overlay(p, t)))
            k += 1
        else:
            out.append((f"lattice_{t % LATTICE_PITCH}", lattice(shape, t)))
    return out


def node_allotment(ntiles, frames):
    """Union-find nodes per tile-frame that a slot of `frames` frames gives the tile pass on average: each frame's
    quota and the shared overflow pool, with the constants read from fm_internal.h and combined as fm_create does
    (nn = tf + tf * kNodesPerTileFrame + max(tf * kNodesShared, ntiles * kTileMaxRuns); the first tf are the
    empty-tile region slots)"""
    text = (pathlib.Path(__file__).resolve().parent.parent / "find_motion_amd" / "csrc" / "fm_internal.h").read_text()
    k = {n: int(re.search(rf"constexpr int {n} = (\d+);", text).group(1))
         for n in ("kNodesPerTileFrame", "kNodesShared", "kTileMaxRuns")}
    tf = ntiles * frames
    return (tf * k["kNodesPerTileFrame"] + max(tf * k["kNodesShared"], ntiles * k["kTileMaxRuns"])) / tf


def tile_components(masks):
    """The 8-connected foreground components of every 64 x 64 tile of every mask of a list, each tile on its own
    (a component that crosses a tile edge counts once in each tile): their total.  Row runs, the pairs of touching
    runs of consecutive rows, and a minimum-label sweep with pointer jumping over those pairs."""
    planes = []
    for m in masks:
        h, w = m.shape
        nty, ntx = -(-h // TS), -(-w // TS)
        pad = np.zeros((nty * TS, ntx * TS), bool)
        pad[:h, :w] = m != 0
        sep = np.zeros((nty, TS + 1, ntx, TS + 1), bool)      # a zero row and column after every tile
        sep[:, :TS, :, :TS] = pad.reshape(nty, TS, ntx, TS)
        planes.append(sep.reshape(nty * (TS + 1), ntx * (TS + 1)))
    width = max(p.shape[1] for p in planes)
    img = np.concatenate([np.pad(p, ((0, 0), (0, width - p.shape[1]))) for p in planes])
    d = np.diff(np.pad(img, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    ys, xs = np.nonzero(d == 1)                               # run starts, in raster order
    ye, xe = np.nonzero(d == -1)                              # one past each run's end
    n = len(ys)
    if n == 0:
        return 0
    K = width + 4
    skey, ekey = ys * K + xs, ye * K + xe - 1
    lo = np.searchsorted(ekey, (ys - 1) * K + xs - 1, "left")        # first run of the row above ending at xs - 1 or later
    hi = np.searchsorted(skey, (ys - 1) * K + xe, "right") - 1       # last one starting at the end + 1 or before
    cnt = np.maximum(hi - lo + 1, 0)
    a = np.repeat(np.arange(n), cnt)
    b = np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    lab = np.arange(n)
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            break
        lab = new
    return int((lab == np.arange(n)).sum())


# ------------------------------------------------------------------------------------------------------------
# references and the comparison with an engine

_REFERENCES = {}


def reference(shape, name, pattern):
    """The oracle's results on dilate5(pattern) and the model's classes, computed once per (shape, name) and
    shared, read-only, by the cases that run the pattern"""
    ref = _REFERENCES.get((shape, name))
    if ref is None:
        dil = dilated(pattern)
        cs = oracle.find_contours_ext(dil, cap=1 << 14)
        classes = tile_classes(dil)
        bits = tile_bits(pattern)
        for a in (dil, bits):
            a.setflags(write=False)
        ref = _REFERENCES[(shape, name)] = dict(
            pattern=pattern.copy(), mask=dil, boxes=[c["bbox"] for c in cs], origins=[c["origin"] for c in cs],
            areas=[c["area"] for c in cs], classes=classes, heavy=sum(1 for v in classes.values() if v[0] == "heavy"), bits=bits)
    assert np.array_equal(ref["pattern"], pattern), f"two patterns named {name} at {shape}"
    return ref


def patterns_of(shape, kind):
    """[(name, pattern)] of a case set: "boundary", "seams", "cut", "ccl" or "four_wave\""""
    if kind == "ccl":
        return [(c[0], c[1]) for c in ccl_set(shape)]
    if kind == "boundary":
        return [(c[0], c[1]) for c in boundary_set(shape)]
    if kind == "cut":
        return [(c[0], c[1]) for c in cut_set(shape)]
    if kind == "four_wave":
        return four_wave_set()
    return [(c[0], c[1]) for c in seam_set(shape)]


def run_batches(eng, shape, named, trace=False, areas=False):
    """The patterns `named` [(name, pattern)] through an engine, S per batch (a short last batch is filled from the
    list's start), T = 2, one batch after the other: every batch's masks, counts, boxes, origins, threshold bits
    and backgrounds against the oracle, no fallback, and heavy_tiles equal to the model's count.  On the per-frame
    path ("pixel": k_pixel and the pixel-level labelling, no tile pass) the bits are refused as on "fused", and
    both statistics hold the 0 a context starts with: fm_wait copies them from the tile pass's words on the
    tile paths only.  Where the engine keeps planes, the blur and delta planes are 255 on the pattern and 0
    elsewhere, and 0 on the black frame.  trace: every point of every contour (an engine with contour_points);
    areas: every contour's area against the oracle's (an engine with contour_area).  Returns the number of batches."""
    from find_motion_amd._native import PLANE_BLUR, PLANE_DELTA, FMError

    S = eng.n_streams
    W, H = shape
    assert eng.work_shape == (H, W) and (eng.params.threshold, eng.params.avg) == (0, 0.0)
    keeps_bits = eng.pixel_path not in ("fused", "pixel")
    nb = -(-len(named) // S)
    for b in range(nb):
        group = [named[(b * S + s) % len(named)] for s in range(S)]
        refs = [reference(shape, n, p) for n, p in group]
        fr, keeps = paint_frames([p for _, p in group])
        for s in range(S):
            eng.set_mask(s, keeps[s])
        eng.submit(fr)
        eng.wait()
        at = f"batch {b} {[n for n, _ in group]}"
        assert eng.fallbacks() == 0, at
        counts = eng.counts()
        for s, (name, _) in enumerate(group):
            ref = refs[s]
            assert not eng.mask(0, s).any() and counts[0, s] == 0 and eng.contours(0, s) == [], f"{at}: black frame"
            np.testing.assert_array_equal(eng.mask(1, s), ref["mask"], err_msg=f"mask {name} ({at})")
            got = eng.contours(1, s)
            assert counts[1, s] == len(ref["boxes"]) == len(got), f"{name} ({at}): {counts[1, s]} contours"
            assert [g.bbox for g in got] == ref["boxes"], f"boxes {name} ({at})"
            assert [g.origin for g in got] == ref["origins"], f"origins {name} ({at})"
            if not keeps_bits:  # (k_fused keeps dilated bits only, the per-frame path a byte mask)
                try:
                    eng.threshold_bits(1, s)
                    raise AssertionError(f"the {eng.pixel_path} path returned threshold bits")
                except FMError:
                    pass
            else:
                assert not eng.threshold_bits(0, s).any(), f"{at}: black frame's bits"
                np.testing.assert_array_equal(eng.threshold_bits(1, s), ref["bits"], err_msg=f"bits {name} ({at})")
            if eng.keep_planes:
                want = (ref["pattern"] != 0).astype(np.uint8) * 255
                for which in (PLANE_BLUR, PLANE_DELTA):
                    assert not eng.plane(which, 0, s).any(), f"plane {which} of the black frame ({at})"
                    np.testing.assert_array_equal(eng.plane(which, 1, s), want, err_msg=f"plane {which} {name} ({at})")
            assert not eng.background(s).any(), f"background {name} ({at})"
            if trace:
                from test_gpu_contour_points import check_frame
                check_frame(eng, 1, s, mask=ref["mask"], tag=f"{name} ({at})")
            if areas:
                assert [g.area for g in got] == ref["areas"], f"areas {name} ({at})"
        heavy = 0 if eng.pixel_path == "pixel" else sum(r["heavy"] for r in refs)
        shared = eng.ccl_stats()["shared_nodes"]
        assert eng.ccl_stats()["heavy_tiles"] == heavy, f"{at}: heavy_tiles {eng.ccl_stats()} != {heavy}"
        assert eng.pixel_path != "pixel" or shared == 0, f"{at}: {eng.ccl_stats()} on the per-frame path"
    return nb


_PLAIN = {}


def plain_reference(shape, name, pattern):
    """The oracle's mask, boxes and origins of a frame painted directly (ksize 1, threshold 0, a black background):
    reference() without the class model, for the large frames of the pool-exhaustion cases"""
    ref = _PLAIN.get((shape, name))
    if ref is None:
        dil = dilated(pattern)
        dil.setflags(write=False)
        cs = oracle.find_contours_ext(dil, cap=1 << 16)
        ref = _PLAIN[(shape, name)] = dict(pattern=pattern.copy(), mask=dil, boxes=[c["bbox"] for c in cs],
                                           origins=[c["origin"] for c in cs])
    assert np.array_equal(ref["pattern"], pattern), f"two frames named {name} at {shape}"
    return ref


def run_direct(eng, shape, named, fallback):
    """One batch on a one-stream engine with ksize 1, threshold 0, avg 0.0 whose background is black (or not yet
    initialised, with a black first frame): frame t is pattern t painted white; every frame's mask, count, boxes
    and origins against the oracle.  fallback: whether the batch has to exhaust the tile pass's nodes (at least one
    frame relabelled by the pixel-level labelling; a batch without one fails) or must not."""
    W, H = shape
    assert eng.work_shape == (H, W) and eng.n_streams == 1 and eng.params.ksize == 1
    assert (eng.params.threshold, eng.params.avg) == (0, 0.0)
    fr = np.zeros((len(named), 1, H, W, 3), np.uint8)
    for t, (_, p) in enumerate(named):
        fr[t, 0][p != 0] = 255
    eng.submit(fr)
    eng.wait()
    print(f"\n{W} x {H}, {len(named)} frames: {eng.fallbacks()} relabelled, {eng.ccl_stats()}")
    assert (eng.fallbacks() > 0) == fallback, f"{eng.fallbacks()} frames fell back"
    counts = eng.counts()
    for t, (name, p) in enumerate(named):
        ref = plain_reference(shape, name, p)
        np.testing.assert_array_equal(eng.mask(t, 0), ref["mask"], err_msg=f"mask of frame {t} {name}")
        got = eng.contours(t, 0)
        assert counts[t, 0] == len(ref["boxes"]) == len(got), f"frame {t} {name}: {counts[t, 0]} contours"
        assert [g.bbox for g in got] == ref["boxes"], f"boxes of frame {t} {name}"
        assert [g.origin for g in got] == ref["origins"], f"origins of frame {t} {name}"
    assert not eng.background(0).any()


TRACE_PATHS = ("reg", "lds", "lds_big", "unstaged")


def trace_paths(boxes):
    """The path of fm_trace.hip each contour box (x, y, w, h) takes, as trace_box_path decides it (restated, with
    the limits read from fm_trace.hip): the padded box in 32-bit words per row, plus one, times its rows"""
    text = (pathlib.Path(__file__).resolve().parent.parent / "find_motion_amd" / "csrc" / "fm_trace.hip").read_text()
    k = {n: int(re.search(rf"constexpr int {n} = (\d+);", text).group(1)) for n in ("kTinyBox", "kWinWords", "kBigWords")}
    out = []
    for _, _, bw, bh in boxes:
        words = (((bw + 2 + 31) >> 5) + 1) * (bh + 2)
        out.append("reg" if bw <= k["kTinyBox"] and bh <= k["kTinyBox"] else
                   "lds" if words <= k["kWinWords"] else "lds_big" if words <= k["kBigWords"] else "unstaged")
    return out
