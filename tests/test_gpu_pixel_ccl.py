"""GPU: the pixel-level labelling of fm_kernels.hip (k_ccl_local, k_ccl_merge, k_ccl_flatten, k_ccl_outer,
k_ccl_roots, k_ccl_bbox) and the tracer's byte-mask source (tr::Mask with mask != nullptr, fm_trace.hip) on the
adversarial masks of contour_content.py, everything compared exactly with the oracle.

The labelling does three jobs and each is run here:

  the per-frame path   a Gaussian above 49 taps with planes kept, or on at most 16 tiles ("pixel": k_pixel and
                       launch_ccl on the whole batch): the boundary, seam and cut sets and the masks aimed at the
                       labelling itself (diagonal contacts across the corners of its 32 x 32 blocks, holes that
                       reach the border through a 1-px channel, islands in holes), at FRAME, at CHAIN with planes and
                       at the three cut shapes (blocks cut by the image at 1, 2 and 31).  The same sets on the "wide"
                       path (fm_wide.hip), which no contour-content case ran.
  the fallback         relabel_frame on the frames of a batch that exhausts the tile pass's union-find nodes, through
                       launch_expand_bits: overlays of the patterns on the dot lattice that exhausts the pool, on the
                       kernel chain (960 x 540), on k_frame_contours (200 x 150) and at a cut width (961 x 540, one
                       pixel in the last tile column).  A batch without a fallback fails the test.
  the refetch          a frame of the per-frame path with more contours than max_contours, beside a stream with
                       fewer, with points and with areas.

The byte-mask tracer: the register path against the image's corners, the LDS window, the big LDS window and the
unstaged sliding window on bytes, and a blob on all four edges; each case again on an engine that traces areas
only (fm_ccl.hip's walker on bytes).  Which kernels ran is read from the engines' own launch names.

test_pixel_ccl_host.py proves the inputs: the layouts, that the overlays keep the patterns' contours, the component
density of the exhausting batches, and the tracer path of every box.
"""
import pytest

import contour_content as cc
from find_motion_amd import MotionEngine
from test_pixel_ccl_host import (CUT_WIDTH, FRAME_LAYOUT, TILE_CHAIN, cap_case, second_batch, tracer_cases)

pytestmark = pytest.mark.gpu

CCL_KERNELS = {"ccl_local", "ccl_merge", "ccl_flatten", "ccl_outer", "ccl_roots", "ccl_bbox"}
TILE_PASS = {"tile_flags", "frame_contours", "regions", "tile_ccl", "merge", "fold_emit"}


def _ran(eng):
    return {n for n, (ms, launches) in eng.kernel_times().items() if launches > 0}


def _engine(shape, S, **kw):
    W, H = shape
    return MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=W, ksize=51, threshold=0, avg=0.0, max_batch=2,
                        profile=True, **kw)


# ---- the per-frame path ------------------------------------------------------------------------------------------
def _per_frame(shape, kinds, **kw):
    named = [c for kind in kinds for c in cc.patterns_of(shape, kind)]
    eng = _engine(shape, 3, **kw)
    try:
        assert eng.pixel_path == "pixel", eng.pixel_path
        assert cc.run_batches(eng, shape, named) >= 2
        ran = _ran(eng)
        assert {"pixel"} | CCL_KERNELS <= ran and not ran & TILE_PASS, ran
    finally:
        eng.close()


def test_per_frame_path_at_sixteen_tiles_or_fewer():
    _per_frame(cc.FRAME, ("boundary", "seams", "ccl"))


def test_per_frame_path_with_planes_kept():
    _per_frame(cc.CHAIN, ("boundary", "seams", "ccl"), keep_planes=True)


@pytest.mark.parametrize("shape", cc.CUTS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_per_frame_path_blocks_cut_by_the_image(shape):
    _per_frame(shape, ("cut", "ccl"), keep_planes=True)


def test_wide_path():
    """A Gaussian of 51 on more than 16 tiles without planes: fm_wide.hip's blur and scan, the dilating chain"""
    named = [c for kind in ("boundary", "seams", "ccl") for c in cc.patterns_of(cc.CHAIN, kind)]
    eng = _engine(cc.CHAIN, 3)
    try:
        assert eng.pixel_path == "wide" and eng.tiles > 16
        cc.run_batches(eng, cc.CHAIN, named)
        ran = _ran(eng)
        assert {"regions", "tile_ccl", "merge", "fold_emit"} <= ran and any(n.startswith("wide") for n in ran), ran
        assert not ran & (CCL_KERNELS | {"pixel", "pix", "fused"}), ran
    finally:
        eng.close()


# ---- the fallback ------------------------------------------------------------------------------------------------
def _exhaust(case, max_contours):
    """The exhausting batch of a case (at least one frame relabelled by the pixel-level labelling, every frame equal
    to the oracle), then four overlays on the same engine with the pool re-armed: no fallback"""
    shape, n, every, _ = case
    W, H = shape
    eng = MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=W, ksize=1, threshold=0, avg=0.0, max_batch=n,
                       max_contours=max_contours)
    try:
        assert eng.pixel_path == "fused"
        cc.run_direct(eng, shape, cc.fallback_frames(shape, n, every), fallback=True)
        cc.run_direct(eng, shape, second_batch(shape), fallback=False)
    finally:
        eng.close()


def test_fallback_on_the_kernel_chain():
    _exhaust(TILE_CHAIN, 512)


def test_fallback_on_the_frame_layout():
    _exhaust(FRAME_LAYOUT, 1024)


def test_fallback_at_a_cut_width():
    _exhaust(CUT_WIDTH, 512)


# ---- more contours than max_contours on the per-frame path --------------------------------------------------------
@pytest.mark.parametrize("flag", [None, "contour_points", "contour_area"])
def test_refetch_of_a_frame_past_max_contours(flag):
    many, few = cap_case()
    named = [("dots_40", many), ("dots_5", few)]
    eng = _engine(cc.FRAME, 2, max_contours=8, **({flag: True} if flag else {}))
    try:
        assert eng.pixel_path == "pixel" and eng.max_contours == 8
        for order in (named, named[::-1], named):      # the refetched frame on either stream, the buffers reused
            cc.run_batches(eng, cc.FRAME, order, trace=flag == "contour_points", areas=flag == "contour_area")
            assert sorted(eng.counts()[1]) == [5, 40]
        assert CCL_KERNELS <= _ran(eng)
    finally:
        eng.close()


# ---- the byte-mask tracer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["frame_seams", "corner_dots", "edge_blob", "chain_seams", "ring_and_blob"])
def test_byte_mask_tracer(name):
    shape, planes, named, paths = tracer_cases()[name]
    want = [p for n, pat in named for p in cc.trace_paths(cc.reference(shape, n, pat)["boxes"])]
    eng = _engine(shape, len(named), keep_planes=planes, contour_points=True)
    try:
        assert eng.pixel_path == "pixel"
        assert cc.run_batches(eng, shape, named, trace=True) == 1
        stats, ran = eng.trace_stats(), _ran(eng)
    finally:
        eng.close()
    assert stats["unstaged"] == want.count("unstaged") and stats["staged"] == len(want) - want.count("unstaged"), stats
    assert stats["steps"] > 0 and (stats["unstaged"] > 0) == ("unstaged" in paths)
    assert {n for n in ran if n.startswith("trace_")} == {f"trace_{pas}_{p}" for pas in ("count", "emit") for p in paths}
    assert CCL_KERNELS <= ran and not ran & TILE_PASS
    eng = _engine(shape, len(named), keep_planes=planes, contour_area=True)
    try:
        assert cc.run_batches(eng, shape, named, areas=True) == 1
    finally:
        eng.close()
