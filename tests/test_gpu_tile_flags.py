"""The tile flags (FLAG_ANY / L / R / T / B and the four corners) that k_tile_flags forms from the stored threshold
bits, once per tile-frame on the contour stream, for the batches whose pixel stage ran the 64 x 64 tile kernels
(k_pix5 with 8 and with 4 waves, k_pixw, k_pix<K> for a first frame).  A missing flag drops a candidate tile, and
with it a contour or the part of a dilated mask that spills over a tile edge.

Every case compares eng.mask, the counts, the contours (boxes and origins) and the background with the oracle,
exactly.  Before that, each case computes from the oracle's own threshold mask (frame_delta > threshold) that the
frames do what they are built for and asserts it: in the listed frame the source tile's threshold bits lie only
within 2 px of the edge or corner that faces the neighbour, the neighbour across has none, and the neighbour's
dilated mask is not empty -- so the neighbour is labelled only if the flag for that direction was set.

k = 5 cases: frame 0 is black (background 0), every later frame holds one white pixel, none within 2 px of the
image's border.  GaussianBlur(5) gives it 255 * 36 / 256 = 36 at the pixel and at most 255 * 24 / 256 = 24 beside
it, so threshold 25 leaves one bit.  The background then holds 3.6 there and less around it: a later pixel beside
earlier ones still reaches 30 (the lowest the oracle gives over these frames), and a pixel that has gone leaves
|0 - 4|.
"""
import numpy as np
import pytest

import oracle
from find_motion_amd import MotionEngine

pytestmark = pytest.mark.gpu

TS = 64
DIRS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]  # L R T B TL TR BL BR


def _tile(a, tx, ty):
    return a[ty * TS:(ty + 1) * TS, tx * TS:(tx + 1) * TS]


def _assert_edge_only(thr, dil, tx, ty, dx, dy, tag):
    """thr / dil: the oracle's threshold and dilated masks of one frame (bool [h][w])"""
    src = _tile(thr, tx, ty)
    ys, xs = np.nonzero(src)
    assert len(ys) > 0, f"{tag}: no threshold bit in the source tile"
    if dx < 0:
        assert xs.max() < 2, tag
    if dx > 0:
        assert xs.min() >= TS - 2, tag
    if dy < 0:
        assert ys.max() < 2, tag
    if dy > 0:
        assert ys.min() >= TS - 2, tag
    assert not _tile(thr, tx + dx, ty + dy).any(), f"{tag}: the neighbour has threshold bits of its own"
    assert _tile(dil, tx + dx, ty + dy).any(), f"{tag}: nothing spills into the neighbour"


def _bits_from_mask(thr):
    """bool [h][w] -> uint64 [ntiles][64], the engine's layout: column words, bit r = row r; zero past the image"""
    h, w = thr.shape
    nty, ntx = (h + TS - 1) // TS, (w + TS - 1) // TS
    pad = np.zeros((nty * TS, ntx * TS), np.uint64)
    pad[:h, :w] = thr
    t = pad.reshape(nty, TS, ntx, TS).transpose(0, 2, 3, 1)  # [ty][tx][col][row]
    return (t << np.arange(TS, dtype=np.uint64)).sum(axis=3, dtype=np.uint64).reshape(nty * ntx, TS)


def _oracle(W, H, S, ksize, thresh, frames, T, keeps, checks):
    """every frame's oracle results, the backgrounds after each batch of T, and the checks asserted on them"""
    cfg = oracle.OracleConfig(H=H, W=W, box=W, ksize=ksize, thresh=thresh, alpha=0.1)
    orc = [oracle.OracleStream(cfg, keeps[s]) for s in range(S)]
    n = frames.shape[0]
    refs, bgs = [], {}
    for t in range(n):
        refs.append([orc[s].step(frames[t, s]) for s in range(S)])
        if (t + 1) % T == 0 or t == n - 1:
            bgs[t] = [orc[s].bg.copy() for s in range(S)]
    for (t, s, tx, ty, dx, dy) in checks:
        r = refs[t][s]
        _assert_edge_only(r["delta"] > thresh, r["mask"] != 0, tx, ty, dx, dy,
                          f"frame {t} stream {s} tile ({tx}, {ty}) -> ({dx}, {dy})")
    return refs, bgs


def _run(W, H, S, ksize, thresh, frames, T, keeps=None, checks=(), bits=False):
    """frames uint8 [n][S][H][W][3] in batches of T; checks: (frame, stream, tx, ty, dx, dy) asserted on the oracle's
    masks before the engine runs; bits: also compare the engine's threshold bits, out-of-image bits included"""
    keeps = keeps or [None] * S
    n = frames.shape[0]
    refs, bgs = _oracle(W, H, S, ksize, thresh, frames, T, keeps, checks)

    eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=W, ksize=ksize, threshold=thresh, avg=0.1, max_batch=T)
    assert eng.work_shape == (H, W)
    for s in range(S):
        if keeps[s] is not None:
            eng.set_mask(s, keeps[s])
    for b0 in range(0, n, T):
        fr = frames[b0:b0 + T]
        eng.submit(fr)
        eng.wait()
        counts = eng.counts()
        for t in range(fr.shape[0]):
            for s in range(S):
                ref, tag = refs[b0 + t][s], f"frame {b0 + t} stream {s}"
                if bits:
                    np.testing.assert_array_equal(eng.threshold_bits(t, s), _bits_from_mask(ref["delta"] > thresh),
                                                  err_msg="threshold bits " + tag)
                np.testing.assert_array_equal(eng.mask(t, s), ref["mask"], err_msg="mask " + tag)
                assert counts[t, s] == ref["count"], tag
                cs = eng.contours(t, s)
                assert [c.bbox for c in cs] == ref["boxes"], tag
                assert [c.origin for c in cs] == ref["origins"], tag
        for s in range(S):
            assert np.array_equal(eng.background(s), bgs[b0 + fr.shape[0] - 1][s]), f"background after frame {b0 + fr.shape[0] - 1}"
    eng.close()
    return refs


def _dot_plan(W):
    """(tx, ty, dx, dy, x, y) of 16 single-pixel frames: every direction out of the interior tile (1, 1), one pixel in
    from the tile's edge, then out of tiles on the image's border and into / out of the partial last tile row and
    column, on the tile's edge itself"""
    last_tx = (W + TS - 1) // TS - 1
    edge_tx = {-1: last_tx, 0: 0, 1: 0} if W % TS == 0 else {-1: last_tx, 0: last_tx, 1: last_tx - 1}
    edge_ty = {-1: 2, 0: 0, 1: 1}
    plan = []
    for interior in (True, False):
        e = 1 if interior else 0
        for dx, dy in DIRS:
            tx, ty = (1, 1) if interior else (edge_tx[dx], edge_ty[dy])
            xi = {-1: e, 0: 4, 1: TS - 1 - e}[dx]
            yi = {-1: e, 0: 4, 1: TS - 1 - e}[dy]
            plan.append((tx, ty, dx, dy, tx * TS + xi, ty * TS + yi))
    return plan


def _dot_frames(W, H):
    plan = _dot_plan(W)
    fr = np.zeros((1 + len(plan), 1, H, W, 3), np.uint8)
    for i, (_, _, _, _, x, y) in enumerate(plan):
        assert 0 <= x < W and 0 <= y < H
        fr[1 + i, 0, y, x] = 255
    checks = [(1 + i, 0, tx, ty, dx, dy) for i, (tx, ty, dx, dy, _, _) in enumerate(plan)]
    return fr, checks


@pytest.mark.parametrize("W,T", [(192, 6), (200, 4)])
def test_every_direction_from_interior_and_edge_tiles(W, T):
    """192 x 136: 3 x 3 tiles with an 8-row last tile row; 200 x 136: a fourth tile column 8 px wide.  17 frames in
    batches of T (the first batch's frame 0 runs k_pix<5>'s init launch, the rest k_pix5's 8-wave loop), one
    direction per frame; the stored bits are compared too, so bits past the image are shown to be zero."""
    fr, checks = _dot_frames(W, 136)
    assert {(dx, dy) for (_, _, tx, ty, dx, dy) in checks if (tx, ty) == (1, 1)} == set(DIRS)
    assert {(dx, dy) for (_, _, tx, ty, dx, dy) in checks if (tx, ty) != (1, 1)} == set(DIRS)
    _run(W, 136, 1, 5, 25, fr, T, checks=checks, bits=True)


def test_keep_mask_zeroes_an_edge_pixel():
    """The keep-mask (KEEP kernels) zeroes the blur at the pixel of the frame whose only bit would sit one pixel
    from tile (1, 1)'s left edge: that frame has no threshold bit and no mask at all, the other frames keep theirs."""
    W, H = 192, 136
    fr, checks = _dot_frames(W, H)
    t0, _, tx, ty, dx, dy = checks[0]
    assert (tx, ty, dx, dy) == (1, 1, -1, 0)
    keep = np.ones((H, W), np.uint8)
    keep[ty * TS + 4, tx * TS + 1] = 0
    assert fr[t0, 0, ty * TS + 4, tx * TS + 1, 0] == 255
    refs = _run(W, H, 1, 5, 25, fr, 6, keeps=[keep], checks=checks[1:])
    assert not (refs[t0][0]["delta"] > 25).any() and not refs[t0][0]["mask"].any() and refs[t0][0]["count"] == 0


def test_partial_tiles_hold_no_bits_past_the_image():
    """Bright content on the last rows and columns of a 200 x 136 image, which REFLECT_101 mirrors into the rows and
    columns the partial tiles compute past the image: the stored column words equal the oracle's threshold mask
    with zeros there, so k_tile_flags needs no mask of its own for partial tiles."""
    W, H = 200, 136
    rng = np.random.default_rng(7)
    fr = np.zeros((4, 1, H, W, 3), np.uint8)
    for t in range(1, 4):
        fr[t, 0, H - 3:, :, :] = rng.integers(0, 2, (3, W, 1)) * 255
        fr[t, 0, :, W - 3:, :] = rng.integers(0, 2, (H, 3, 1)) * 255
    refs = _run(W, H, 1, 5, 12, fr, 4, bits=True)
    thr = refs[2][0]["delta"] > 12
    assert thr[H - 2:, :].any() and thr[:, W - 2:].any()
    words = _bits_from_mask(thr).reshape(3, 4, TS)
    assert not (words[2] >> np.uint64(8)).any() and not words[:, 3, 8:].any()  # (what the comparison above held to)


def test_four_wave_kernel():
    """8 streams of 1024 x 512 = 1,024 tile-streams, the smallest grid that selects k_pix5's 4-wave, 16-row tiles;
    3 frames, stream s sends direction s out of tile (1, 1) in frame 1 and the opposite one in frame 2."""
    W, H, S = 1024, 512, 8
    fr = np.zeros((3, S, H, W, 3), np.uint8)
    checks = []
    for s in range(S):
        for t, (dx, dy) in ((1, DIRS[s]), (2, (-DIRS[s][0], -DIRS[s][1]))):
            x = TS + {-1: 1, 0: 30, 1: TS - 2}[dx]
            y = TS + {-1: 1, 0: 30, 1: TS - 2}[dy]
            fr[t, s, y, x] = 255
            checks.append((t, s, 1, 1, dx, dy))
    _run(W, H, S, 5, 25, fr, 3, checks=checks)


def test_wide_gaussian_kernel_k21():
    """k = 21 on k_pixw (192 x 136: w % 4 == 0, more than 16,384 pixels).  A 21-tap blur leaves no 2-px blob, so the
    keep-mask carves one: it keeps only a 2-px band inside tile (1, 1)'s left edge and one inside its bottom edge,
    and a bright block covers one band in frame 1 and the other in frame 2."""
    W, H, thresh = 192, 136, 40
    keep = np.zeros((H, W), np.uint8)
    keep[TS + 20:TS + 40, TS:TS + 2] = 1            # left band of tile (1, 1)
    keep[2 * TS - 2:2 * TS, TS + 20:TS + 40] = 1    # bottom band of tile (1, 1): rows 126, 127
    fr = np.zeros((3, 1, H, W, 3), np.uint8)
    fr[1, 0, TS + 10:TS + 50, TS - 16:TS + 16] = 255
    fr[2, 0, 2 * TS - 8:H, TS + 10:TS + 50] = 255
    _run(W, H, 1, 21, thresh, fr, 3, keeps=[keep], checks=[(1, 0, 1, 1, -1, 0), (2, 0, 1, 1, 0, 1)], bits=True)
