"""k_pix5's 8-wave kernel takes its horizontal blur sums from the matrix cores (v_mfma_i32_16x16x32_i8 over signed
gray bytes, the taps divided by 16, REFLECT_101 folded into the tap matrix of the tile's edge blocks) and its
chain reads them as (H - 2^15) / 16.  Against the oracle, frame by frame: masks, counts, boxes, origins and the
float64 background bit for bit (run_pair), k = 5, box = W, no planes, S = 1, T = 3, three batches -- a wrong H at
any pixel of the image changes the background.

  right edge   the last tile column is w - x0 = 4, 8, ..., 64 columns wide: every place in a column block, and
               every column block, the right fold can take (W = 132 ... 192)
  saturated    columns 0..5 and w-6..w-1 alternate 0 / 255 per column and per frame, the interior is all 255 in
               one frame and all 0 in the next: the folded taps carry the largest sums of either sign
  narrow       one tile column holding both folds (64 x 264), and both folds in one block (8 x 2056)
  variants     a keep-mask and accumulateWeighted's scalar tail (196 x 135): the KEEP and TAIL instantiations

Every width comes at the smallest height with more than 16,384 pixels, past the small-image path;
test_shapes_run_the_pixel_kernel reads that from the engine's own launch timing.
"""
import numpy as np
import pytest

from find_motion_amd import MotionEngine
from find_motion_amd.synthetic import batch
from test_gpu_parity import run_pair

pytestmark = pytest.mark.gpu

T, NB = 3, 3


def _h(W):
    return 16384 // W + 1


RIGHT = [(128 + 4 * r, _h(128 + 4 * r)) for r in range(1, 17)]
SATURATED = [(W, _h(W)) for W in (132, 148, 164, 192)]
NARROW = [(8, 2056), (64, 264)]


def test_shapes_are_what_the_docstring_says():
    assert [W - 128 for W, H in RIGHT] == list(range(4, 65, 4))
    for W, H in RIGHT + SATURATED + NARROW:
        assert W * (H - 1) <= 16384 < W * H or (W, H) in NARROW
        assert W * H > 16384 and W % 4 == 0
    assert (196 * 135) % 16 == 12


@pytest.mark.parametrize("W,H", RIGHT)
def test_right_edge_fold_vs_oracle(W, H):
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, keep_planes=False, start=5)


def _saturated_frames(W, H):
    out = []
    for b in range(NB):
        fr = np.empty((T, 1, H, W, 3), np.uint8)
        for t in range(T):
            f = b * T + t
            fr[t, 0] = 255 if f % 2 == 0 else 0
            cols = np.r_[0:6, W - 6:W]
            fr[t, 0][:, cols] = (((cols + f) % 2) * 255).astype(np.uint8)[None, :, None]
        out.append(fr)
    return out


@pytest.mark.parametrize("W,H", SATURATED)
def test_saturated_edges_vs_oracle(W, H):
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, keep_planes=False, frames=_saturated_frames(W, H))


@pytest.mark.parametrize("W,H", NARROW)
def test_both_folds_in_one_tile_vs_oracle(W, H):
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, keep_planes=False, start=17)


@pytest.mark.parametrize("W,H", [(200, 136), (196, 135)])  # KEEP alone, and with TAIL (h * w % 16 = 12)
def test_keep_mask_variant_vs_oracle(W, H):
    masks = [((0, 0), (W // 5, H // 4)), ((W - 1, H - 1), (W // 2, H - 1), (W - 1, H // 2))]
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, masks=masks, keep_planes=False, start=29)


def test_scalar_tail_variant_vs_oracle():
    run_pair(196, 135, 196, ksize=5, S=1, T=T, n_batches=NB, keep_planes=False, start=31)


@pytest.mark.parametrize("W,H", RIGHT + NARROW + [(196, 135)])
def test_shapes_run_the_pixel_kernel(W, H):
    eng = MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=W, ksize=5, threshold=12, avg=0.1, max_batch=2,
                       profile="pix")
    fr = batch(W, H, 1, 0, 2)
    for _ in range(2):  # the second batch has no first-frame launch
        eng.submit(fr)
        eng.wait()
    names = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0}
    eng.close()
    assert "pix" in names and not names & {"small_scan", "fused"}, names
