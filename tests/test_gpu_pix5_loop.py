"""k_pix5's 8-wave frame loop (reads hoisted behind the frame barrier, one loop copy for edge tiles and one for
interior tiles, the tap stage running past the batch's last frame) against the oracle, frame by frame: masks,
counts, boxes, origins and the background bit for bit (run_pair), k = 5, box = W, no planes.

Each tile layout comes at two heights.  The short shape is the smallest image with that layout; its work image
holds <= 16,384 pixels, which the product runs on the small-image path (fm_small.hip), so it guards that path's
results for the same layouts.  The tall shape keeps the columns (the tile kinds, the `vq` mirror quads) and
accumulateWeighted's tail and adds tile rows until the image is past that limit, so that it runs k_pix5;
test_tall_shapes_run_the_pixel_kernel reads that from the engine's own launch timing.

T in {1, 2, 3, 4} with 3 batches: the first batch's init frame runs in k_pix, so k_pix5 sees t_begin = 1,
single-frame launches (the taps then read a gray buffer nothing wrote and fill an H buffer nothing reads), and
the clamped prologue and epilogue loads.
"""
import pytest

from find_motion_amd import MotionEngine
from find_motion_amd.synthetic import batch
from test_gpu_parity import run_pair

pytestmark = pytest.mark.gpu

# (W, H of the short shape, H of the tall shape)
LAYOUTS = [
    (8, 8, 2056),      # one partial tile a row (tall: 33 tile rows, the last of 8 rows)
    (64, 64, 264),     # one tile that is both the left and the right edge (tall: a fifth tile row of 8 rows)
    (68, 64, 248),     # a 4-column last tile, the vq mirror quads (tall: a last tile row of 56 rows)
    (200, 72, 136),    # edge, two interior and edge tiles, plus a last tile row of 8 valid rows
    (196, 71, 135),    # the same tile layout with accumulateWeighted's scalar tail: h * w % 16 = 12 at both heights
]
SHAPES = [(W, H) for W, Hs, Ht in LAYOUTS for H in (Hs, Ht)]
TALL = [(W, Ht) for W, Hs, Ht in LAYOUTS]


def test_layouts_are_what_the_comments_say():
    for W, Hs, Ht in LAYOUTS:
        assert Hs * W <= 16384 < Ht * W
        assert (Hs * W) % 16 == (Ht * W) % 16
    assert (196 * 71) % 16 == 12


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("W,H", SHAPES)
def test_pix5_frame_loop_vs_oracle(W, H, T):
    run_pair(W, H, W, ksize=5, T=T, n_batches=3, keep_planes=False, start=11)


@pytest.mark.parametrize("W,H", [(200, 72), (200, 136), (196, 71), (196, 135)])
def test_pix5_frame_loop_keep_mask(W, H):
    """A polygon keep-mask on the stream: the KEEP kernels, with the scalar tail at W = 196."""
    masks = [((0, 0), (W // 5, H // 4)), ((W - 1, H - 1), (W // 2, H - 1), (W - 1, H // 2))]
    run_pair(W, H, W, ksize=5, T=3, n_batches=3, masks=masks, keep_planes=False, start=23)


@pytest.mark.parametrize("W,H", TALL)
def test_tall_shapes_run_the_pixel_kernel(W, H):
    eng = MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=W, ksize=5, threshold=12, avg=0.1, max_batch=2,
                       profile="pix")
    fr = batch(W, H, 1, 0, 2)
    for _ in range(2):  # the second batch has no first-frame launch
        eng.submit(fr)
        eng.wait()
    names = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0}
    eng.close()
    assert "pix" in names and not names & {"small_scan", "fused"}, names
