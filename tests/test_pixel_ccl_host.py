"""The inputs of test_gpu_pixel_ccl.py, proven on the CPU oracle alone.

  layouts       fm_plan: every case of the GPU module takes the path it stands for -- the per-frame path ("pixel":
                k_pixel, the pixel-level labelling, the byte-mask tracer) or, for the pool-exhaustion frames, the
                tile pass whose fallback relabel_frame is.
  overlays      a pattern on a dot lattice with the dots within 6 px left out: every contour of the pattern alone is
                a contour of the frame, same origin and box -- for every overlay frame the GPU cases submit.
  density       the batch that has to exhaust the tile pass's union-find nodes holds, per tile-frame, at least 1.25
                times as many 8-connected foreground components (counted tile by tile) as the slot has nodes per
                tile-frame; the allotment is read from fm_internal.h (contour_content.node_allotment).  The two
                smaller batches (the frame layout's, the cut width's) hold more components than nodes, which is
                what makes a fallback certain: every component of a tile takes a node at least.
  tracer        the boxes of the byte-mask tracer's cases take the paths of fm_trace.hip they are named for.
"""
import numpy as np
import pytest

import contour_content as cc
import oracle
from find_motion_amd import _native

# shape, frames in the batch, an overlay every n-th frame (the others: pure lattice), the density the batch must have
# in units of the allotment
TILE_CHAIN = ((960, 540), 32, 2, 1.25)
FRAME_LAYOUT = ((200, 150), 64, 4, 1.0)
CUT_WIDTH = ((961, 540), 32, 2, 1.0)
EXHAUSTING = (TILE_CHAIN, FRAME_LAYOUT, CUT_WIDTH)
SECOND_BATCH = 4              # overlay frames of the batch after the exhausted one


def second_batch(shape):
    """[(name, overlay)] of the small batch that follows the exhausting one on the same engine: no fallback"""
    src = cc.overlay_sources(shape)
    picks = [src[i] for i in (2, 5, len(src) - 4, len(src) - 2)]   # ring_diagonal, spiral, block_corner_anti, a notch
    return [(f"overlay_{n}_3", cc.overlay(p, 3)) for n, p in picks]


# the byte-mask tracer's cases: name -> (shape, keep_planes, the paths its contours take)
def tracer_cases():
    from test_gpu_contour_points import dot_and_corner_dots, edge_blob, ring_and_blob

    return {
        "frame_seams": (cc.FRAME, False, cc.patterns_of(cc.FRAME, "seams"), {"reg", "lds"}),
        "corner_dots": ((100, 100), False, [("dot_and_corner_dots", dot_and_corner_dots() // 255)], {"reg"}),
        "edge_blob": ((200, 130), False, [("edge_blob", edge_blob() // 255)], {"lds"}),
        "chain_seams": (cc.CHAIN, True, cc.patterns_of(cc.CHAIN, "seams"), {"reg", "lds", "lds_big"}),
        "ring_and_blob": ((1040, 520), True, [("ring_and_blob", ring_and_blob(520, 1040) // 255)], {"lds", "unstaged"}),
    }


def cap_case():
    """(the 40 dots, the second stream's few dots) of the max_contours = 8 case at FRAME"""
    from test_gpu_contour_points import dots

    W, H = cc.FRAME
    return dots(H, W, 40, 3) // 255, dots(H, W, 5, 4) // 255


def _sid(case):
    return f"{case[0][0]}x{case[0][1]}"


def _plan(shape, k, **kw):
    return _native.plan(src_w=shape[0], src_h=shape[1], box_size=shape[0], ksize=k, threshold=0, avg=0.0, **kw)


def test_layouts():
    for shape, n, every, _ in EXHAUSTING:
        p = _plan(shape, 1, max_batch=n, max_contours=512)
        assert p["pixel_path"] == "fused" and (p["tiles"] > 16) == (shape != FRAME_LAYOUT[0]), (shape, p)
    assert CUT_WIDTH[0][0] % 64 == 1
    for name, (shape, planes, named, paths) in tracer_cases().items():
        p = _plan(shape, 51, max_batch=2, n_streams=len(named), keep_planes=planes, contour_points=True)
        assert p["pixel_path"] == "pixel", (name, p)
        assert p["tiles"] <= 16 or planes, name
    assert _plan(cc.FRAME, 51, max_batch=2, n_streams=2, max_contours=8)["pixel_path"] == "pixel"


@pytest.mark.parametrize("case", EXHAUSTING, ids=_sid)
def test_overlays_keep_the_patterns_contours(case):
    shape, n, every, _ = case
    frames = cc.fallback_frames(shape, n, every)
    assert frames[0][0] == "black" and not frames[0][1].any() and len(frames) == n
    src = dict(cc.overlay_sources(shape))
    assert len(src) == 15 and {"corner_main", "spiral", "islands", "notch_closed", "block_corner_anti"} <= set(src)
    seen = set()
    for t, (name, p) in list(enumerate(frames)) + [(None, f) for f in second_batch(shape)]:
        if name == "black":
            continue
        if not name.startswith("overlay_"):
            assert t % every and np.array_equal(p, cc.lattice(shape, t)), (t, name)
            continue
        base = name[len("overlay_"):].rsplit("_", 1)[0]
        seen.add(base)
        alone = oracle.find_contours_ext(cc.dilated(src[base]), cap=1 << 16)
        ref = cc.plain_reference(shape, name, p)
        both = set(zip(ref["origins"], ref["boxes"]))
        assert alone and all((c["origin"], c["bbox"]) in both for c in alone), name
        assert (p[src[base] != 0] != 0).all(), name
        # the lattice is there: more contours than the pattern has, but where the pattern closes the frame off
        assert len(both) > len(alone) or base == "notch_closed", name
    assert len(seen) >= min(15, (n - 1) // every), seen


@pytest.mark.parametrize("case", EXHAUSTING, ids=_sid)
def test_component_density_exceeds_the_node_allotment(case):
    shape, n, every, factor = case
    ntiles = -(-shape[0] // 64) * -(-shape[1] // 64)
    masks = [cc.plain_reference(shape, name, p)["mask"] for name, p in cc.fallback_frames(shape, n, every)]
    density = cc.tile_components(masks) / (ntiles * n)
    allot = cc.node_allotment(ntiles, n)
    print(f"\n{_sid(case)}: {density:.2f} components per tile-frame, {allot:.2f} nodes: {density / allot:.3f}")
    assert density >= factor * allot, (density, allot)
    # the second batch on the same engine fits: fewer components than the slot has nodes
    few = cc.tile_components([cc.dilated(p) for _, p in second_batch(shape)])
    assert few < ntiles * n * allot / 4, (few, ntiles * n * allot)


def test_tile_components_counts_tile_by_tile():
    m = np.zeros((70, 130), np.uint8)
    m[10, 60:70] = 1            # one run across the edge of tiles (0, 0) | (0, 1): a component in each
    m[63, 5] = m[64, 6] = 1     # a diagonal contact across a tile edge: two
    m[20:23, 100] = m[22, 101] = m[21, 102] = 1   # 8-connected inside a tile: one
    m[40, 20] = m[40, 22] = 1   # two pixels a gap apart: two
    assert cc.tile_components([m]) == 2 + 2 + 1 + 2
    assert cc.tile_components([m, m]) == 14 and cc.tile_components([np.zeros((5, 5), np.uint8)]) == 0
    ring = cc._rect(cc._canvas((64, 64)), 5, 5, 50, 50)
    assert cc.tile_components([ring]) == 1
    lat = cc.dilated(cc.lattice((128, 128), 0))
    assert cc.tile_components([lat]) == 4 * 11 * 11


def test_tracer_cases_take_the_paths_they_are_named_for():
    for name, (shape, planes, named, paths) in tracer_cases().items():
        got = set()
        for n, p in named:
            assert p.shape == shape[::-1] and set(np.unique(p)) <= {0, 1}, (name, n)
            got |= set(cc.trace_paths(cc.reference(shape, n, p)["boxes"]))
        assert got == paths, (name, got)
    # the spiral's box at CHAIN is the one past kWinWords, the ring's at 1040 x 520 the one past kBigWords
    sp = cc.reference(cc.CHAIN, "spiral", dict(cc.patterns_of(cc.CHAIN, "seams"))["spiral"])["boxes"]
    assert cc.trace_paths(sp) == ["lds_big"] and sp[0][2] >= 250
    ring = tracer_cases()["ring_and_blob"][2][0]
    boxes = cc.reference((1040, 520), *ring)["boxes"]
    assert cc.trace_paths(boxes) == ["unstaged", "lds"] and boxes[0][2:] == (1001, 518)
    # the blob on all four edges, the 3 x 3 squares in the corners
    assert cc.reference((200, 130), *tracer_cases()["edge_blob"][2][0])["boxes"] == [(0, 0, 200, 130)]
    corner = cc.reference((100, 100), *tracer_cases()["corner_dots"][2][0])["boxes"]
    assert sorted(b[2:] for b in corner) == [(3, 3)] * 4 + [(5, 5)]


def test_more_contours_than_the_cap():
    many, few = cap_case()
    assert len(cc.reference(cc.FRAME, "dots_40", many)["boxes"]) == 40
    assert len(cc.reference(cc.FRAME, "dots_5", few)["boxes"]) == 5 < 8
