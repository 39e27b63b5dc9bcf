"""k_pix5's 8-wave kernel takes the whole 5 x 5 blur from the matrix cores: two v_mfma_i32_16x16x64_i8 products over
the 5 x 24 byte gray window of each output row of a 16 x 16 block, the taps as c[dr] c[dc] / 256 with REFLECT_101
folded into the tap matrix, and runs the chain in the product's layout (a lane holds rows 4 (l / 16) .. + 3 of column
l % 16 of two blocks; lanes l and l ^ 16 put a byte of the tile's column word together).  Against the oracle, frame
by frame: masks, counts, boxes, origins and the float64 background bit for bit (run_pair), k = 5, box = W, no planes,
three batches of T = 3 of S = 1 unless a case says otherwise.

  rows in a lane   the last tile row is 1 .. 8 and 60 .. 64 rows high: every place in a lane's nibble and in a byte of
                   the column word ends the image (W = 132, H = 129 .. 136 and 188 .. 192)
  vertical         rows 0..5 and h-6..h-1 alternate 0 / 255 per row and per frame, the interior is all 255 in one
  saturation       frame and all 0 in the next; and a 2-D checkerboard that flips every frame: the largest sums of
                   either sign down a column and in both directions
  corners          both column folds with the top and bottom reflections in one tile (64 x 264, 8 x 2056), rows
                   patterned as above
  short batches    T = 1 .. 5: the prologue and the stages that run past the batch's end; the first batch of a run has
                   the first-frame launch, the later ones do not; two streams in one grid at T = 3
  keep-mask        a staircase polygon whose steps cut the 4-row groups and 16-column blocks, a one-row-high and a
                   one-column-wide strip (200 x 136)
  scalar tail      h w % 16 = 4, 8, 12 (132 x 129, 136 x 125, 196 x 135), with and without the keep-mask

Every shape has more than 16,384 pixels, past the small-image path; test_shapes_run_the_pixel_kernel reads that from
the engine's own launch timing.
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


LAST_ROWS = [(132, H) for H in list(range(129, 137)) + list(range(188, 193))]
VSAT = [(W, _h(W)) for W in (132, 192)]
CORNERS = [(64, 264), (8, 2056)]
SHORT = (132, _h(132))
TAILS = [(132, 129, 4), (136, 125, 8), (196, 135, 12)]
STAIRS = [(0, 0), (21, 0), (21, 6), (37, 6), (37, 13), (53, 13), (53, 23), (70, 23), (70, 34), (99, 34), (99, 49),
          (131, 49), (131, 67), (150, 67), (150, 90), (0, 90)]
KEEP_MASKS = [STAIRS, ((0, 101), (199, 101)), ((163, 0), (163, 135))]


def test_shapes_are_what_the_docstring_says():
    assert [H - 128 for W, H in LAST_ROWS] == list(range(1, 9)) + list(range(60, 65))
    for W, H in LAST_ROWS + VSAT + CORNERS + [SHORT] + [(w, h) for w, h, r in TAILS] + [(200, 136)]:
        assert W * H > 16384 and W % 4 == 0
    for W, H in VSAT + [SHORT]:
        assert W * (H - 1) <= 16384
    for W, H, r in TAILS:
        assert (W * H) % 16 == r
    # the staircase's steps: no x on a 16-column block's edge, no y on a 4-row group's edge (but the polygon's own ends)
    assert all(x % 16 and y % 4 for x, y in STAIRS[2:-2])


@pytest.mark.parametrize("W,H", LAST_ROWS)
def test_last_tile_row_heights_vs_oracle(W, H):
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, keep_planes=False, start=7)


def _row_frames(W, H, checker=False):
    out = []
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(NB):
        fr = np.empty((T, 1, H, W, 3), np.uint8)
        for t in range(T):
            f = b * T + t
            if checker:
                fr[t, 0] = ((((yy + xx + f) % 2) * 255).astype(np.uint8))[:, :, None]
            else:
                fr[t, 0] = 255 if f % 2 == 0 else 0
                rows = np.r_[0:6, H - 6:H]
                fr[t, 0][rows] = (((rows + f) % 2) * 255).astype(np.uint8)[:, None, None]
        out.append(fr)
    return out


@pytest.mark.parametrize("checker", [False, True], ids=["rows", "checkerboard"])
@pytest.mark.parametrize("W,H", VSAT)
def test_vertical_saturation_vs_oracle(W, H, checker):
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, keep_planes=False, frames=_row_frames(W, H, checker))


@pytest.mark.parametrize("W,H", CORNERS)
def test_corners_vs_oracle(W, H):
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, keep_planes=False, frames=_row_frames(W, H))


@pytest.mark.parametrize("Tb,S", [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (3, 2)])
def test_short_batches_vs_oracle(Tb, S):
    W, H = SHORT
    run_pair(W, H, W, ksize=5, S=S, T=Tb, n_batches=NB, keep_planes=False, start=11)


def test_keep_mask_in_the_product_layout_vs_oracle():
    run_pair(200, 136, 200, ksize=5, S=1, T=T, n_batches=NB, masks=KEEP_MASKS, keep_planes=False, start=13)


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("W,H,rem", TAILS)
def test_scalar_tail_vs_oracle(W, H, rem, keep):
    masks = [((0, 0), (W // 3, H // 2)), ((W - 1, H - 1), (W // 2, H - 1), (W - 1, H - 9))] if keep else None
    run_pair(W, H, W, ksize=5, S=1, T=T, n_batches=NB, masks=masks, keep_planes=False, start=19)


@pytest.mark.parametrize("W,H", [LAST_ROWS[0], LAST_ROWS[-1]] + VSAT + CORNERS + [(200, 136)] + [(w, h) for w, h, r in TAILS[1:]])
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
