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

test_contour_content_host.py asserts every stated class, count and contour outcome on the oracle alone;
test_gpu_contour_content.py runs the same sets through engines and compares bit for bit.
"""
import functools

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
            classes=classes, heavy=sum(1 for v in classes.values() if v[0] == "heavy"), bits=bits)
    assert np.array_equal(ref["pattern"], pattern), f"two patterns named {name} at {shape}"
    return ref


def patterns_of(shape, kind):
    """[(name, pattern)] of a case set: "boundary", "seams", "cut" or "four_wave\""""
    if kind == "boundary":
        return [(c[0], c[1]) for c in boundary_set(shape)]
    if kind == "cut":
        return [(c[0], c[1]) for c in cut_set(shape)]
    if kind == "four_wave":
        return four_wave_set()
    return [(c[0], c[1]) for c in seam_set(shape)]


def run_batches(eng, shape, named, trace=False):
    """The patterns `named` [(name, pattern)] through an engine, S per batch (a short last batch is filled from the
    list's start), T = 2, one batch after the other: every batch's masks, counts, boxes, origins, threshold bits
    and backgrounds against the oracle, no fallback, and heavy_tiles equal to the model's count.  Returns the
    number of batches."""
    from find_motion_amd._native import FMError

    S = eng.n_streams
    W, H = shape
    assert eng.work_shape == (H, W) and (eng.params.threshold, eng.params.avg) == (0, 0.0)
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
            if eng.pixel_path == "fused":  # (k_fused keeps dilated bits only)
                try:
                    eng.threshold_bits(1, s)
                    raise AssertionError("the fused path returned threshold bits")
                except FMError:
                    pass
            else:
                assert not eng.threshold_bits(0, s).any(), f"{at}: black frame's bits"
                np.testing.assert_array_equal(eng.threshold_bits(1, s), ref["bits"], err_msg=f"bits {name} ({at})")
            assert not eng.background(s).any(), f"background {name} ({at})"
            if trace:
                from test_gpu_contour_points import check_frame
                check_frame(eng, 1, s, mask=ref["mask"], tag=f"{name} ({at})")
        heavy = sum(r["heavy"] for r in refs)
        assert eng.ccl_stats()["heavy_tiles"] == heavy, f"{at}: heavy_tiles {eng.ccl_stats()} != {heavy}"
    return nb
