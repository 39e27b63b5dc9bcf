"""GPU: the contour pass on every tile class, class boundary and seam topology, on the layouts the product runs.

The adversarial masks of the other modules are painted with ksize 1: past 16,384 pixels that is the "fused" path
(k_fused dilates itself, the chain runs k_tile_ccl<false>), below it the small-image path (k_frame_contours).  The
product chain -- k_pix5, k_tile_flags, k_regions<true>, k_tile_ccl<true> and its dilate_tile, k_tile_heavy,
k_merge, k_fold, k_emit, k_counts on more than 16 tiles -- saw the seeded synthetic streams.  contour_content.py
paints exact masks through the keep-mask behind any Gaussian, and test_contour_content_host.py proves every
class, count and outcome of them on the oracle.

  case              shape      k   sets                 what runs
  chain, dilating   324 x 260  5   boundary, seams, ccl  k_pix5, k_tile_flags, the dilating chain on 30 tiles
  frame layout      200 x 136  5   boundary + seams     k_pix5, k_frame_contours<true> on 12 tiles
  k_pixw            324 x 260  21  boundary + seams     k_pixw, the dilating chain
  fused             324 x 260  11  boundary, seams, ccl  k_fused, the non-dilating chain
  small path        128 x 96   1   boundary (13 tiles)  the small-image path, k_frame_contours on 4 tiles
  trace             324 x 260  5   seams                contour_points: every point and area (fm_trace.hip)
  cut               3 shapes   5   cut                  w % 64 and h % 64 in {1, 2, 63}: tiles cut by the image
  four-wave         8 x 1024 x 512  5  mixed frames     k_pix5's 4-wave tiles, 128 tiles per frame

("ccl": the masks aimed at the pixel-level labelling -- block-corner contacts, border notches, islands -- which the
tile pass has to get right too; test_gpu_pixel_ccl.py runs every set on the per-frame and the wide path.)

Every case: S streams carry different patterns in one batch (T = 2: a black frame, a white one), batch after
batch on one engine, so that slots are reused with other masks; masks, counts, boxes, origins, threshold bits
(where the path keeps them) and the background are compared exactly, fallbacks() is 0 and
ccl_stats()["heavy_tiles"] equals the class model's count of heavy tiles in the batch.
"""
import pytest

import contour_content as cc
from find_motion_amd import MotionEngine

pytestmark = pytest.mark.gpu


def _engine(shape, k, S=3, **kw):
    W, H = shape
    return MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=W, ksize=k, threshold=0, avg=0.0, max_batch=2, **kw)


def _run(shape, k, kinds, path, chain, S=3, reuse=False, **kw):
    named = [c for kind in kinds for c in cc.patterns_of(shape, kind)]
    eng = _engine(shape, k, S, **kw)
    try:
        assert eng.pixel_path == path, eng.pixel_path
        assert (eng.tiles > 16) == chain, eng.tiles
        nb = cc.run_batches(eng, shape, named, trace=kw.get("contour_points", False))
        if reuse:  # every slot again, with the masks in another order and another stream
            assert eng.max_inflight >= 2
            while nb <= eng.max_inflight + 1:
                named = named[1:] + named[:1]
                nb += cc.run_batches(eng, shape, named)
    finally:
        eng.close()


def test_dilating_chain():
    _run(cc.CHAIN, 5, ("boundary", "seams", "ccl"), "pix", True, reuse=True)


def test_frame_layout():
    _run(cc.FRAME, 5, ("boundary", "seams"), "pix", False, reuse=True)


def test_wide_gaussian_kernel():
    _run(cc.CHAIN, 21, ("boundary", "seams"), "pix", True)


def test_fused_non_dilating_chain():
    _run(cc.CHAIN, 11, ("boundary", "seams", "ccl"), "fused", True)


def test_small_image_path():
    _run(cc.SMALL, 1, ("boundary",), "small", False)


def test_trace_follows_the_seams():
    _run(cc.CHAIN, 5, ("seams",), "pix", True, contour_points=True)


@pytest.mark.parametrize("shape", cc.CUTS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiles_cut_by_the_image(shape):
    _run(shape, 5, ("cut",), "pix", True)


def test_four_wave_kernel():
    """8 streams x 128 tiles = 1,024 tile-streams, the smallest grid that selects k_pix5's 4-wave, 16-row tiles"""
    _run(cc.FOUR_WAVE, 5, ("four_wave",), "pix", True, S=8)
