"""The colour-motion reference: the chain find_motion.py would run without its cvtColor line (fm.py:493),
composed from the stages oracle.oracle already restates.  TEST ONLY.

Per frame: small = imutils.resize(raw, width=box) (resize_area_bgr; the frame itself when box = W);
blur[..., c] = GaussianBlur(small[..., c]) for c = B, G, R (gauss_blur per channel); the keep-mask writes 0 into
all three channels; the first frame sets ref = blur; delta = absdiff(blur, convertScaleAbs(ref)) and
accumulateWeighted(blur, ref) run on the interleaved (h, w, 3) arrays, so diff_thresh and accumulate see
n = 3hw elements and apply OpenCV's SIMD rules to that count by themselves; the three threshold planes are ORed
(findContours needs one plane; dilation commutes with OR), then dilate5 and find_contours_ext as always.

Variants for tests of the reference's own properties:
  all_fma      accumulateWeighted as if every element were in the vector body (no scalar tail)
  per_plane_n  the SIMD rules applied per channel plane (n = hw), which is NOT what OpenCV does on a 3-channel Mat
"""
import numpy as np

import oracle
from oracle import oracle as oo

ISO_BG = (0, 51, 0)      # BGR; gray (1868 * 0 + 9617 * 51 + 4899 * 0 + 8192) >> 14 = 30
ISO_MOVER = (0, 0, 100)  # BGR; gray (4899 * 100 + 8192) >> 14 = 30


def work_shape(H, W, box):
    return oo.work_height(H, W, box), box


def accumulate_all_fma(blur, bg, alpha):
    """accumulate() with every element in the fma body: the arrays padded to a multiple of 16 elements."""
    n = blur.size
    pad = (-n) % 16
    b = np.concatenate([blur.reshape(-1), np.zeros(pad, np.uint8)])
    g = np.concatenate([bg.reshape(-1), np.zeros(pad, np.float64)])
    oo.accumulate(b, g, alpha)
    bg.reshape(-1)[:] = g[:n]


class ColourStream:
    """One stream's state: the (h, w, 3) float64 background, the init flag and the keep-mask."""

    def __init__(self, H, W, box, ksize, thresh=12, alpha=0.1, keep=None, all_fma=False, per_plane_n=False):
        self.H, self.W, self.box, self.ksize, self.thresh, self.alpha = H, W, box, ksize, thresh, alpha
        self.h, self.w = work_shape(H, W, box)
        self.bg = np.zeros((self.h, self.w, 3), np.float64)
        self.initialized = False
        self.keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        self.all_fma, self.per_plane_n = all_fma, per_plane_n

    def reset(self):
        self.initialized = False

    def set_background(self, bg):
        bg = np.asarray(bg, np.float64)
        assert bg.shape == self.bg.shape
        self.bg[...] = bg
        self.initialized = True

    def small(self, bgr):
        assert bgr.shape == (self.H, self.W, 3) and bgr.dtype == np.uint8
        return np.ascontiguousarray(bgr) if self.box == self.W else oo.resize_area_bgr(bgr, self.box)

    def blur(self, bgr):
        small = self.small(bgr)
        blur = np.stack([oo.gauss_blur(np.ascontiguousarray(small[..., c]), self.ksize) for c in range(3)], axis=2)
        if self.keep is not None:
            blur[self.keep == 0] = 0
        return np.ascontiguousarray(blur)

    def step(self, bgr, with_points=False):
        blur = self.blur(bgr)
        if not self.initialized:
            self.bg[...] = blur
            self.initialized = True
        if self.per_plane_n:
            parts = [oo.diff_thresh(np.ascontiguousarray(blur[..., c]), np.ascontiguousarray(self.bg[..., c]), self.thresh)
                     for c in range(3)]
            delta = np.stack([p[0] for p in parts], axis=2)
            th = np.stack([p[1] for p in parts], axis=2)
        else:
            delta, th = oo.diff_thresh(blur, self.bg, self.thresh)
        if self.all_fma:
            accumulate_all_fma(blur, self.bg, self.alpha)
        else:
            oo.accumulate(blur, self.bg, self.alpha)
        thresh = np.ascontiguousarray(th.max(axis=2))
        mask = oo.dilate5(thresh)
        cont = oo.find_contours_ext(mask, with_points=with_points)
        return {"blur": blur, "delta": delta, "thresh": thresh, "mask": mask, "count": len(cont),
                "boxes": [c["bbox"] for c in cont], "origins": [c["origin"] for c in cont], "contours": cont}


def threshold_bits(thresh):
    """The engine's layout of the undilated threshold plane (fm_read_threshold_bits): uint64 [ntiles][64], tile in
    raster order, word c = column c of the tile, bit r = row r."""
    h, w = thresh.shape
    ntx, nty = (w + 63) // 64, (h + 63) // 64
    p = np.zeros((nty * 64, ntx * 64), np.uint64)
    p[:h, :w] = thresh != 0
    t = p.reshape(nty, 64, ntx, 64).transpose(0, 2, 3, 1)  # [ty][tx][c][r]
    return (t << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64).reshape(nty * ntx, 64)


def iso_clip(W=96, H=80, n=6, size=12, step=3):
    """The isoluminant mover: a size x size block of ISO_MOVER moving step px a frame (and one row down) over
    ISO_BG; frames [n][H][W][3].  Both colours have gray 30, so the gray chain's frame_delta is 0 everywhere."""
    fr = np.empty((n, H, W, 3), np.uint8)
    fr[...] = ISO_BG
    for t in range(n):
        x, y = 10 + step * t, 20 + t
        assert x + size <= W and y + size <= H
        fr[t, y:y + size, x:x + size] = ISO_MOVER
    return fr


def noise_clip(W, H, S, n, seed):
    """Seeded noise around a mid level with two moving coloured blocks per stream, different per stream; frames
    [n][S][H][W][3].  The noise (+-3) stays under the threshold after the blur; the blocks do not."""
    rng = np.random.default_rng(seed)
    base = rng.integers(90, 140, size=(S, H, W, 3), dtype=np.int64)
    fr = np.empty((n, S, H, W, 3), np.uint8)
    colours = [(250, 20, 20), (20, 250, 20), (20, 20, 250), (250, 250, 20)]
    for t in range(n):
        f = base + rng.integers(-3, 4, size=base.shape)
        for s in range(S):
            for b in range(2):
                bw, bh = max(1, W // 5), max(1, H // 4)
                x = (7 * t + 23 * s + 31 * b) % max(1, W - bw + 1)
                y = (5 * t + 11 * s + 17 * b) % max(1, H - bh + 1)
                f[s, y:y + bh, x:x + bw] = colours[(s + 2 * b + t // 3) % 4]
        fr[t] = np.clip(f, 0, 255)
    return fr


TAIL_W, TAIL_H, TAIL_SEED = 66, 70, 2024  # 3hw % 16 = 4: the scalar tail splits a pixel's channels
TAIL_SIZES = [1, 7, 65] + [3] * 7         # batches of the GPU test, as many as the engine keeps in flight (3 .. 10)


def tail_clip():
    """The GPU test's seeded noise content at 66 x 70, two streams, frames [94][2][70][66][3]."""
    return noise_clip(TAIL_W, TAIL_H, 2, sum(TAIL_SIZES), TAIL_SEED)


def gray_counts(frames, box, ksize, thresh=12, alpha=0.1):
    """The gray oracle's contour count of each frame of one stream [n][H][W][3]."""
    cfg = oracle.OracleConfig(H=frames.shape[1], W=frames.shape[2], box=box, ksize=ksize, thresh=thresh, alpha=alpha)
    st = oracle.OracleStream(cfg)
    return [st.step(f)["count"] for f in frames]
