"""The masks of test_gpu_contour_content.py, proven on the CPU oracle and the class model alone.

For every shape the GPU module runs: the painter gives the oracle exactly dilate5(pattern) behind a Gaussian of 5,
11 and 21 (and 1 at the small shape), batch after batch on one stream without a reset; every boundary tile has
exactly the stated class and run counts by contour_content.tile_classes; each case set holds all six classes; the
seam cases give the contour counts and the external / not-external outcomes their names say; no tile exceeds
kTileMaxRuns.  The same for the per-frame path's cases (a Gaussian of 51) and for the masks aimed at the pixel-level
labelling: the block-corner contacts, the border notches (which border pixels are zero, that they are 4-connected
to the hole, the contour counts) and the islands.
"""
import numpy as np
import pytest

import contour_content as cc
import oracle

SHAPES = (cc.CHAIN, cc.FRAME, cc.SMALL) + cc.CUTS + (cc.FOUR_WAVE,)
KINDS = {cc.CHAIN: ("boundary", "seams"), cc.FRAME: ("boundary", "seams"), cc.SMALL: ("boundary",),
         cc.FOUR_WAVE: ("four_wave",), **{s: ("cut",) for s in cc.CUTS}}


def _sid(shape):
    return f"{shape[0]}x{shape[1]}"


CCL_SHAPES = (cc.CHAIN, cc.FRAME) + cc.CUTS      # the shapes that also run the masks for the pixel-level labelling


def _all(shape):
    kinds = KINDS[shape] + (("ccl",) if shape in CCL_SHAPES else ())
    return [(f"{kind}:{n}", p) for kind in kinds for n, p in cc.patterns_of(shape, kind)]


def test_shapes_take_the_layouts_they_stand_for():
    """fm_plan, which needs no device: the path and the tile count of every GPU case"""
    from find_motion_amd import _native

    def plan(shape, k, **kw):
        return _native.plan(src_w=shape[0], src_h=shape[1], box_size=shape[0], ksize=k, threshold=0, avg=0.0,
                            max_batch=2, **kw)

    assert (plan(cc.CHAIN, 5, n_streams=3)["pixel_path"], plan(cc.CHAIN, 5, n_streams=3)["tiles"]) == ("pix", 30)
    assert (plan(cc.FRAME, 5, n_streams=3)["pixel_path"], plan(cc.FRAME, 5, n_streams=3)["tiles"]) == ("pix", 12)
    assert plan(cc.CHAIN, 21, n_streams=3)["pixel_path"] == "pix"
    assert (plan(cc.CHAIN, 11, n_streams=3)["pixel_path"], plan(cc.CHAIN, 11, n_streams=3)["tiles"]) == ("fused", 30)
    assert plan(cc.SMALL, 1, n_streams=3)["pixel_path"] == "small" and cc.SMALL[0] * cc.SMALL[1] <= 16384
    for shape in cc.CUTS:
        p = plan(shape, 5, n_streams=3)
        assert (p["pixel_path"], p["tiles"]) == ("pix", 30)
        assert shape[0] % 64 in (1, 2, 63) and shape[1] % 64 in (1, 2, 63)
    assert {s[0] % 64 for s in cc.CUTS} == {s[1] % 64 for s in cc.CUTS} == {1, 2, 63}
    assert plan(cc.FOUR_WAVE, 5, n_streams=8)["tiles"] * 8 == 1024
    # a Gaussian above 49 taps: the per-frame path at 16 tiles or fewer, or where planes are kept; else fm_wide.hip
    assert (plan(cc.FRAME, 51, n_streams=3)["pixel_path"], plan(cc.FRAME, 51, n_streams=3)["tiles"]) == ("pixel", 12)
    assert plan(cc.CHAIN, 51, n_streams=3, keep_planes=True)["pixel_path"] == "pixel"
    assert (plan(cc.CHAIN, 51, n_streams=3)["pixel_path"], plan(cc.CHAIN, 51, n_streams=3)["tiles"]) == ("wide", 30)
    for shape in cc.CUTS:   # 32 x 32 labelling blocks and 64 x 16 k_pixel tiles cut at 1, 2 and 31
        assert plan(shape, 51, n_streams=3, keep_planes=True)["pixel_path"] == "pixel"
    assert {s[0] % 32 for s in cc.CUTS} == {s[1] % 32 for s in cc.CUTS} == {1, 2, 31}
    assert {s[1] % 16 for s in cc.CUTS} <= {1, 2, 15}


@pytest.mark.parametrize("shape", SHAPES[:-1], ids=_sid)
def test_painter_identity(shape):
    """One oracle stream per Gaussian size takes every pattern of the shape in turn as its keep-mask -- a black
    frame, a white frame, no reset between -- and gives dilate5(pattern), the shared reference's contours and a
    background of zeros every time."""
    W, H = shape
    for k in (1, 5) if shape == cc.SMALL else (5, 11, 21, 51):
        orc = oracle.OracleStream(oracle.OracleConfig(H=H, W=W, box=W, ksize=k, thresh=0, alpha=0.0))
        for name, p in _all(shape):
            fr, keeps = cc.paint_frames([p])
            orc.keep = keeps[0]
            first = orc.step(fr[0, 0])
            assert not first["mask"].any() and first["count"] == 0, (k, name)
            res = orc.step(fr[1, 0], cap=1 << 14)
            ref = cc.reference(shape, name.split(":")[1], p)
            np.testing.assert_array_equal(res["mask"], cc.dilated(p), err_msg=f"k {k} {name}")
            np.testing.assert_array_equal(res["mask"], ref["mask"])
            np.testing.assert_array_equal(res["delta"] > 0, p != 0, err_msg=f"threshold bits k {k} {name}")
            for plane in ("blur", "delta"):   # what an engine that keeps planes returns
                np.testing.assert_array_equal(res[plane], (p != 0) * np.uint8(255), err_msg=f"{plane} k {k} {name}")
                assert not first[plane].any(), (k, name)
            assert (res["boxes"], res["origins"]) == (ref["boxes"], ref["origins"]), (k, name)
            assert not orc.bg.any(), (k, name)


def test_tile_bits_layout():
    p = np.zeros((70, 130), np.uint8)
    p[3, 63] = p[69, 129] = p[64, 0] = 1
    b = cc.tile_bits(p)
    assert b.shape == (6, 64) and int((b != 0).sum()) == 3
    assert b[0, 63] == 1 << 3 and b[5, 1] == 1 << 5 and b[3, 0] == 1


@pytest.mark.parametrize("shape", (cc.CHAIN, cc.FRAME, cc.SMALL), ids=_sid)
def test_boundary_tiles_have_the_stated_class_and_counts(shape):
    got = {}
    for name, p, tile, cls, compact, total in cc.boundary_set(shape):
        c = cc.tile_classes(cc.dilated(p))[tile]
        got[name] = c
        assert c[0] == cls, (name, c)
        assert compact is None or c[1] == compact, (name, c)
        assert total is None or c[2] == total, (name, c)
    print(f"\n{_sid(shape)}: {got}")
    assert got["compact_64"][:2] == ("compact", 64) and got["compact_65"][1] == 65 and got["compact_65"][0] != "compact"
    if shape != cc.SMALL:
        assert got["total_256"] [0] == "light" and got["total_256"][2] == 256 and got["total_256"][1] > 64
        assert got["total_257"][0] == "heavy" and got["total_257"][2] == 257
        assert got["heavy_rows"][2] == cc.HEAVY_ROWS_RUNS >= 1400 and got["heavy_rows"][1] > 64
        assert len(cc.boundary_set(shape)) == len(cc.boundary_table())
    else:
        assert got["heavy_rows"][2] > 1300


def test_simple_variants_are_what_their_names_say():
    """On the model's own terms: r0 / r1, the diagonal contact and its near-miss, the chains, the root count"""
    tab = cc.boundary_table()

    def tile(name):
        p = cc._put(cc._canvas((192, 192)), 1, 1, tab[name][0])
        return cc._tiles(cc.dilated(p))[(1, 1)]

    t = tile("simple_all_rows")
    assert t.any(1).all() and cc.simple_roots(t) == 3          # left chain, foreground, right chain
    t = tile("simple_from_top")
    assert t[0].any() and not t[63].any() and cc.simple_roots(t) == 2   # the bottom region (both chains), foreground
    t = tile("simple_to_bottom")
    assert t[63].any() and not t[0].any() and cc.simple_roots(t) == 2   # top (with both chains), foreground
    t = tile("simple_diagonal")
    r = 23                                                     # the lower square's first row
    assert np.flatnonzero(t[r])[0] == np.flatnonzero(t[r - 1])[-1] + 1 and cc.simple_roots(t) == 2
    t = tile("simple_near_miss")
    assert np.flatnonzero(t[r])[0] == np.flatnonzero(t[r - 1])[-1] + 2 and cc.simple_roots(t) is None
    t = tile("simple_diag_left")
    assert np.flatnonzero(t[r])[-1] == np.flatnonzero(t[r - 1])[0] - 1 and cc.simple_roots(t) == 2
    assert cc.simple_roots(tile("simple_miss_left")) is None
    t = tile("simple_left_chain")
    assert t[30, 63] and not t[30, 0] and cc.simple_roots(t) == 2     # mergeTB: top = bottom, and the foreground
    t = tile("simple_right_chain")
    assert t[30, 0] and not t[30, 63] and cc.simple_roots(t) == 2
    t = tile("simple_slope")
    rows = np.flatnonzero(t.any(1))
    assert t[rows[0], 0] and t[rows[-1], 63] and 0 < rows[0] and rows[-1] < 63
    assert cc.simple_roots(t) == 3                             # top, foreground, bottom: no chain spans the band
    t = tile("simple_slope_up")
    rows = np.flatnonzero(t.any(1))
    assert t[rows[0], 63] and t[rows[-1], 0] and cc.simple_roots(t) == 3   # the bottom region's root is a right run
    assert cc.simple_roots(tile("simple_teeth")) == cc.TEETH_ROOTS
    t = tile("simple_col63")
    assert t[:, 63].sum() == 5 and not t[:, :63].any()
    t = tile("simple_col0")
    assert t[:, 0].sum() == 5 and not t[:, 1:].any()


def test_model_on_hand_made_tiles():
    """The class model against tiles written down by hand (not dilated): the run counts at each limit, the `nroots >
    64` exit, which dilated masks cannot reach, and the order of the tests"""
    t = np.zeros((64, 64), bool)
    assert cc.tile_class(t)[0] == "empty" and cc.tile_class(~t)[0] == "full"
    t[:, 1:63] = True
    t[0::2, 0] = True          # foreground from column 0 on even rows, up to column 63 on odd rows
    t[1::2, 63] = True
    assert cc.simple_roots(t) == 32 + 32 + 1 and cc.tile_class(t)[0] != "simple"
    t[0, 63] = True            # one right chain fewer
    assert cc.simple_roots(t) == 64 and cc.tile_class(t)[0] == "simple"
    t = np.zeros((64, 64), bool)
    t[::2, ::2] = True         # 64 runs on even rows, 1 on odd ones: 32 * 64 + 32 runs, every row distinct
    assert cc.run_counts(t) == (32 * 64 + 32, 32 * 64 + 32) and cc.tile_class(t)[0] == "over"
    t[8:] = False              # 4 * 64 + 4 runs on the first 8 rows, 56 on the rest (which repeat row 7)
    assert cc.run_counts(t) == (4 * 65, 4 * 65 + 56) and cc.tile_class(t)[0] == "heavy"
    t = np.zeros((64, 64), bool)
    t[10:20, 5] = t[10:20, 9] = True
    assert cc.run_counts(t) == (1 + 5 + 1, 54 + 50) and cc.tile_class(t)[0] == "compact"
    # rows 1..9; the band's 3 background runs under row 9's one; 5 runs under 5 on 9 rows; one run under 3; rows 21..63
    assert cc.pair_count(t) == 9 + 3 + 9 * 5 + 3 + 43


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_every_class_occurs_and_no_tile_is_past_the_heavy_pass(shape):
    for kind in KINDS[shape]:
        seen = dict.fromkeys(cc.CLASSES, 0)
        for name, p in cc.patterns_of(shape, kind):
            cl = cc.reference(shape, name, p)["classes"]
            for c, compact, total in cl.values():
                assert c != "over" and total <= cc.HEAVY_MAX, (kind, name, c, total)
                seen[c] += 1
        print(f"\n{_sid(shape)} {kind}: {seen}")
        assert all(seen.values()), (kind, seen)


@pytest.mark.parametrize("shape", cc.CUTS, ids=_sid)
def test_cut_tiles(shape):
    W, H = shape
    for name, p, tile, cls in cc.cut_set(shape):
        if tile is None:
            continue
        cl = cc.tile_classes(cc.dilated(p))
        assert cl[tile][0] != "empty", name
        assert cls is None or cl[tile][0] == cls, (name, cl[tile])
    named = dict((c[0], c) for c in cc.cut_set(shape))
    lx, ly = (W - 1) // 64, (H - 1) // 64
    d = cc.dilated(named["cut_col63"][1])[:, (lx - 1) * 64:lx * 64]
    assert d[:, 63].any() and not d[:, :62].any() and (W % 64 == 1) == bool(d[:, 62].any())
    d = cc.dilated(named["cut_right_all_rows"][1])
    assert d[64:128, lx * 64].all()
    d = cc.dilated(named["cut_bottom_all_rows"][1])
    assert d[ly * 64:, 64 + 30].all()
    # a heavy tile cut to 63 rows or columns
    assert any(c[3] == "heavy" for c in cc.cut_set(shape)) == (63 in (W % 64, H % 64))


def _regions(empty):
    """4-connected regions of the empty tiles of a grid: tile -> the region's tiles"""
    out, seen = {}, set()
    for start in zip(*np.nonzero(empty)):
        if start in seen:
            continue
        reg, todo = set(), [start]
        while todo:
            y, x = todo.pop()
            if (y, x) in reg or not (0 <= y < empty.shape[0] and 0 <= x < empty.shape[1]) or not empty[y, x]:
                continue
            reg.add((y, x))
            todo += [(y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)]
        seen |= reg
        for t in reg:
            out[t] = reg
    return out


@pytest.mark.parametrize("shape", (cc.CHAIN, cc.FRAME), ids=_sid)
def test_seam_cases(shape):
    W, H = shape
    seams = {n: (p, cnt) for n, p, cnt in cc.seam_set(shape)}
    refs = {n: cc.reference(shape, n, p) for n, (p, _) in seams.items()}
    for n, (p, cnt) in seams.items():
        assert cnt is None or len(refs[n]["boxes"]) == cnt, (n, len(refs[n]["boxes"]))
    # every pair of dots is one contour, 10 x 10, around a four-tile corner
    for n in ("corner_main", "corner_anti"):
        assert refs[n]["boxes"] and all(b[2:] == (10, 10) and (b[0] + 5) % 64 == 0 and (b[1] + 5) % 64 == 0
                                        for b in refs[n]["boxes"]), refs[n]["boxes"]
    d = refs["corner_main"]["mask"]
    assert d[63, 63] and d[64, 64] and not d[63, 64] and not d[64, 63]
    d = refs["corner_anti"]["mask"]
    assert d[63, 64] and d[64, 63] and not d[63, 63] and not d[64, 64]
    # the ring's only closure is the diagonal contact at (63, 64) | (64, 63); its inner dot starts on column 0 of
    # tile (1, 2) and is not external; the "C" differs by one pattern pixel and its inner dot is external
    d = refs["ring_diagonal"]["mask"]
    assert d[63, 64] and d[64, 63] and not d[63, 63] and not d[64, 64]
    inner, edge, outer = (128, 88), (64, 18), (0, 28)
    assert inner not in refs["ring_diagonal"]["origins"] and inner in refs["ring_open"]["origins"]
    for n in ("ring_diagonal", "ring_open"):
        assert edge in refs[n]["origins"] and outer in refs[n]["origins"]      # REF_EDGE and REF_OUTER starts
    assert int((seams["ring_diagonal"][0] != seams["ring_open"][0]).sum()) == 1
    d = refs["ring_open"]["mask"]
    assert not d[63, 63:65].any() and not d[64, 64]
    # one component through every tile
    for n in ("serpentine",):
        assert all(c[0] != "empty" for c in refs[n]["classes"].values()), n
        assert refs[n]["boxes"] == [(0, 30, W, H - 30)]
    side = min(W, H)
    assert refs["spiral"]["boxes"][0][2] >= side - 10 and refs["spiral"]["heavy"] >= 4
    assert refs["nested_rings"]["boxes"] == [(8, 8, W - 16, H - 16)]
    # tile (1, 1) without a bit of its own, filled from its eight neighbours on every edge and corner
    p, d = seams["halo"][0], refs["halo"]["mask"][64:128, 64:128]
    assert not p[64:128, 64:128].any() and all(p[y:y + 64, x:x + 64].any() for y in (0, 64, 128) for x in (0, 64, 128)
                                                if (y, x) != (64, 64) and y < H)
    assert d[0].any() and d[63].any() and d[:, 0].any() and d[:, 63].any() and not d[2:62, 2:62].any()
    assert d[0, 0] and d[0, 63] and d[63, 0] and d[63, 63]
    # all six classes in adjacent tiles
    cl = refs["mixed"]["classes"]
    assert {cl[(y, x)][0] for y in (0, 1) for x in (0, 1, 2)} == set(cc.CLASSES)
    if shape != cc.CHAIN:
        return
    # the wide ring: whole tiles of its hole are empty, a region that does not reach the grid border; closed, the
    # dot in the hole is not external, opened it is
    for n, is_open in (("wide_ring", False), ("wide_ring_open", True)):
        cl = refs[n]["classes"]
        nty, ntx = 1 + max(k[0] for k in cl), 1 + max(k[1] for k in cl)
        empty = np.array([[cl[(y, x)][0] == "empty" for x in range(ntx)] for y in range(nty)])
        reg = _regions(empty)
        hole = reg[(1, 2)]
        assert hole == {(1, 2), (1, 3), (2, 1), (2, 2), (2, 3)} and not empty[1, 1]
        assert all(0 < y < nty - 1 and 0 < x < ntx - 1 for y, x in hole)
        assert ((98, 98) in refs[n]["origins"]) == is_open
        assert (158, H - 5) in refs[n]["origins"]


def _flood4(zero, seeds):
    """The pixels of `zero` (bool) 4-connected to the seed pixels"""
    reach = np.zeros_like(zero)
    for y, x in seeds:
        reach[y, x] = zero[y, x]
    while True:
        grow = reach.copy()
        grow[1:] |= reach[:-1]
        grow[:-1] |= reach[1:]
        grow[:, 1:] |= reach[:, :-1]
        grow[:, :-1] |= reach[:, 1:]
        grow &= zero
        if np.array_equal(grow, reach):
            return reach
        reach = grow


@pytest.mark.parametrize("shape", CCL_SHAPES, ids=_sid)
def test_masks_for_the_pixel_level_labelling(shape):
    W, H = shape
    cases = {n: (p, cnt) for n, p, cnt in cc.ccl_set(shape)}
    refs = {n: cc.reference(shape, n, p) for n, (p, _) in cases.items()}
    for n, (p, cnt) in cases.items():
        assert len(refs[n]["boxes"]) == cnt, (n, len(refs[n]["boxes"]), cnt)
        assert all(c[0] != "over" for c in refs[n]["classes"].values()), n
    # every pair of dots is one 10 x 10 contour around a corner of four 32-px blocks that is no tile corner, and
    # the two squares touch there diagonally only
    for n, main in (("block_corner_main", True), ("block_corner_anti", False)):
        boxes = refs[n]["boxes"]
        assert len(boxes) == ((H - 5 - 32) // 64 + 1) * ((W - 5 - 32) // 64 + 1) >= 4
        d = refs[n]["mask"]
        for x, y, bw, bh in boxes:
            cx, cy = x + 5, y + 5
            assert (bw, bh) == (10, 10) and cx % 64 == 32 and cy % 64 == 32, (n, x, y, bw, bh)
            assert bool(d[cy - 1, cx - 1]) == bool(d[cy, cx]) == main, (n, cx, cy)
            assert bool(d[cy - 1, cx]) == bool(d[cy, cx - 1]) == (not main), (n, cx, cy)
    # the notches: the zero border pixels, their 4-connection to the hole, the counts
    tab = cc.notch_table(shape)
    assert len(tab) == 1 + 4 * 3 + 4
    border = np.zeros((H, W), bool)
    border[0] = border[-1] = border[:, 0] = border[:, -1] = True
    hole = (10, 7)                                 # left of the first dot's square
    for n, (p, dots, zero, is_open) in tab.items():
        d = refs[n]["mask"]
        assert dots >= 12 and not d[hole], n
        got = sorted(zip(*np.nonzero(border & (d == 0))))
        assert got == sorted(zero), (n, got, zero)
        assert len(zero) == (0 if not is_open else 4 if n[6:] in cc.NOTCH_CORNERS else 1), (n, zero)
        assert len(refs[n]["boxes"]) == (1 + dots if is_open else 1), n
        assert refs[n]["boxes"][0] == (0, 0, W, H), n
        if is_open:
            reach = _flood4(d == 0, zero)
            assert reach[hole] and all(reach[z] for z in zero), n
            # 1 px wide: with any channel pixel next to the border filled, the hole is closed again
            y, x = zero[-1] if n[6:] in cc.NOTCH_CORNERS else zero[0]
            shut = d.copy()
            shut[y, x] = 255
            assert len(oracle.find_contours_ext(shut)) == 1, n
        else:
            assert not _flood4(d == 0, [hole])[border].any()
    sides = {n: z[0] for n, (p, dots, z, o) in tab.items() if o and len(z) == 1}
    assert {sides[f"notch_top_{a}"][1] for a in ("start", "middle", "end")} == {7, (W // 2) // 32 * 32, W - 8}
    assert {sides[f"notch_right_{a}"] for a in ("start", "middle", "end")} == {(7, W - 1), ((H // 2) // 32 * 32, W - 1),
                                                                               (H - 8, W - 1)}
    assert {z[0] for z in sides.values()} >= {0, H - 1} and {z[1] for z in sides.values()} >= {0, W - 1}
    corners = {tab[f"notch_{c}"][2][0] for c in cc.NOTCH_CORNERS}
    assert corners == {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    # the islands: one contour; without the outer ring the middle ring and the dots of the outer hole are external,
    # without the two outer rings the inner ring and the dots of the middle hole
    p, dots = cc.islands(shape)
    assert refs["islands"]["boxes"] == [(8, 8, W - 16, H - 16)]
    rings = [cc._rect(cc._canvas(shape), 10 + 14 * i, 10 + 14 * i, H - 11 - 14 * i, W - 11 - 14 * i) for i in range(3)]
    left = [dots]
    for i in range(3):
        p = p & ~rings[i]
        cs = oracle.find_contours_ext(cc.dilated(p))
        left.append(len(cs) - (1 if i < 2 else 0))    # the dots now external (and the next ring)
        assert (i == 2) or (8 + 14 * (i + 1), 8 + 14 * (i + 1), W - 16 - 28 * (i + 1), H - 16 - 28 * (i + 1)) in \
            [c["bbox"] for c in cs], i
    assert left[3] == dots and 0 < left[1] < left[2] < left[3] and left[1] >= 8 and left[2] - left[1] >= 8
    assert left[3] - left[2] >= 2                 # dots inside the innermost ring


def test_four_wave_frames():
    for name, p in cc.patterns_of(cc.FOUR_WAVE, "four_wave"):
        cl = cc.reference(cc.FOUR_WAVE, name, p)["classes"]
        h = cc.histogram(cl)
        assert all(h[c] for c in cc.CLASSES) and h["over"] == 0, (name, h)


def test_which_frames_of_the_older_heavy_tiles_test_reach_the_heavy_list():
    """test_gpu_parity.test_heavy_tiles_stripes_and_rings, whose docstring says so: the stripes' tiles are compact
    (identical rows); the later frames, each holding the pattern before it too, have 8 and 9 heavy tiles"""
    H, W = 150, 200
    stripes = np.zeros((H, W), bool)
    stripes[:, ::6] = True
    rings = np.zeros((H, W), bool)
    for cy, cx in [(40, 40), (75, 130), (120, 60)]:
        for rad in (30, 18, 8):
            yy, xx = np.ogrid[:H, :W]
            rings |= np.abs(np.hypot(yy - cy, xx - cx) - rad) < 0.6
        rings[cy, cx] = True
    checker = np.zeros((H, W), bool)
    checker[::7, ::7] = True
    orc = oracle.OracleStream(oracle.OracleConfig(H=H, W=W, box=W, ksize=1, thresh=100, alpha=0.5))
    orc.step(np.zeros((H, W, 3), np.uint8))
    cl = []
    for p, union in ((stripes, stripes), (rings, stripes | rings), (checker, rings | checker)):
        mask = orc.step(np.repeat((p * 255).astype(np.uint8)[..., None], 3, 2))["mask"]
        np.testing.assert_array_equal(mask, cc.dilated(union))
        cl.append(cc.tile_classes(mask))
    assert cc.histogram(cl[0])["compact"] == 12 and all(21 <= v[1] <= 24 or v[1] <= 5 for v in cl[0].values())
    assert 1300 <= max(v[2] for v in cl[0].values()) <= 1500
    heavy = [sorted(v[2] for v in c.values() if v[0] == "heavy") for c in cl]
    assert [len(h) for h in heavy] == [0, 8, 9] and (heavy[1][0], heavy[1][-1]) == (392, 1348)
    assert (heavy[2][0], heavy[2][-1]) == (298, 838)
