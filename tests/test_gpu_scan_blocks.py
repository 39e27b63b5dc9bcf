"""GPU: the block logic of the frame scan (fm_scan.h's scan_frames) on its five users, exact against each model's
reference: the oracle (k_small_scan behind k_small_blur and behind k_wide_blur), tests/colour_ref.py (k_rgb_scan)
and tests/mog2_ref.py (k_mog2_scan behind either blur).

A scan wave parks each frame's column word in lane (t - t_begin) % 64 and stores 64 frames' words at once, with the
FLAG_* word of each ORed into the tile-frame's flags; a launch's last, partial block is flushed at its end.  One
engine per case takes batches of 1, 64, 128, 63, 65 and 129 frames in that order: the lone first frame makes every
later launch of the average paths start at t_begin = 0 (no init split), and the lengths are then a block-exact flush
with no tail, two blocks, a tail only, a block plus a one-frame tail, and two blocks plus one.

After every batch: the threshold bits of every frame (the scan's stores), the contour count, boxes and origins (the
contour pass reads the tile flags: a flag missed is a contour missed), and after the last batch the background
(average, colour) or the model (mixture).  All exact.

Shapes (work w x h):
  66 x 70    small, rgb, mog2 behind k_small_blur; k 5, two streams, stream 1 under a polygon keep-mask.  The second
             tile column has the image's columns 64 and 65 only (c < 2: FLAG_L and the corner flags), the first
             tile's columns 62 and 63 are its c >= 62 ones, and the second tile row has 6 valid lanes: the smallest
             image with a padded last tile column and a partly valid tile row.
  328 x 136  wide (k 51) and mog2 behind k_wide_blur (k 5), one stream: the smallest shapes fm_plan sends there.  The
             Python mixture reference takes about 20 ms a frame here (9 s for the 450 frames), so that case runs 1,
             64 and 65 frames: a lone frame, a block-exact flush and a block plus a one-frame tail.

The content is colour_ref.noise_clip, lengthened: seeded noise under the threshold with two moving blocks per stream.
The reference side asserts that in every batch of more than one frame some frame has threshold bits in the last tile
column and some frame has none there, and the same for the last tile row, so the flags and their absence are both
exercised.  (The one-frame batch cannot have both: a stream's first frame has no bits on the average paths, where
the background becomes the blur, and every bit on the mixture path, where no mode exists yet.)
"""
import numpy as np
import pytest

import colour_ref
import mog2_ref
import oracle
from find_motion_amd import MotionEngine, rasterize_masks

pytestmark = pytest.mark.gpu

SIZES = (1, 64, 128, 63, 65, 129)
SHORT = (1, 64, 65)
SEED = 4242
KEEP_POLY = [[(8, 6), (50, 12), (40, 60), (12, 44)]]
THRESH, ALPHA = 12, 0.1


class AverageRef:
    """oracle.OracleStream with the step's undilated threshold plane beside the rest."""

    def __init__(self, H, W, k, keep):
        self.st = oracle.OracleStream(oracle.OracleConfig(H=H, W=W, box=W, ksize=k, thresh=THRESH, alpha=ALPHA), keep=keep)

    def step(self, bgr):
        r = self.st.step(bgr)
        r["thresh"] = np.where(r["delta"] > THRESH, 255, 0).astype(np.uint8)
        return r

    def check_state(self, eng, s):
        np.testing.assert_array_equal(eng.background(s), self.st.bg, err_msg=f"background stream {s}")


class ColourRef(colour_ref.ColourStream):
    def __init__(self, H, W, k, keep):
        super().__init__(H, W, W, k, THRESH, ALPHA, keep=keep)

    def check_state(self, eng, s):
        np.testing.assert_array_equal(eng.background(s), self.bg, err_msg=f"background stream {s}")


class MixtureRef(mog2_ref.Mog2Stream):
    def __init__(self, H, W, k, keep):
        super().__init__(H, W, W, k, keep=keep)

    def check_state(self, eng, s):
        got = eng.mog2_model(s)
        w, m, v, n = self.arrays()
        np.testing.assert_array_equal(got["nmodes"], n, err_msg=f"nmodes stream {s}")
        for name, want in (("weight", w), ("mean", m), ("var", v)):  # (zeros at mode >= nmodes on both sides)
            assert got[name].tobytes() == want.tobytes(), f"{name} stream {s}"
        assert got["nframes"] == self.nframes


# name: work W, H, ksize, streams, batches, reference, engine arguments, pixel_path, launches that must / must not run
CASES = {
    "small": (66, 70, 5, 2, SIZES, AverageRef, {}, "small",
              {"small_blur", "small_scan", "small_blur_init", "small_scan_init"}, {"wide_blur", "pix", "fused", "pixel"}),
    "rgb": (66, 70, 5, 2, SIZES, ColourRef, {"colour_motion": True}, "rgb",
            {"rgb_blur", "rgb_scan", "rgb_blur_init", "rgb_scan_init"}, {"small_scan", "pix", "fused", "pixel"}),
    "mog2_small": (66, 70, 5, 2, SIZES, MixtureRef, {"mog2": True}, "mog2",
                   {"small_blur", "mog2_scan"}, {"wide_blur", "small_scan", "pix", "fused", "pixel"}),
    "wide": (328, 136, 51, 1, SIZES, AverageRef, {}, "wide",
             {"wide_blur", "wide_scan", "wide_blur_init", "wide_scan_init"}, {"small_blur", "pix", "fused", "pixel"}),
    "mog2_wide": (328, 136, 5, 1, SHORT, MixtureRef, {"mog2": True}, "mog2",
                  {"wide_blur", "mog2_scan"}, {"small_blur", "small_scan", "pix", "fused", "pixel"}),
}


def make_refs(name):
    W, H, k, S, _sizes, Ref = CASES[name][:6]
    keeps = [None] * S
    if S > 1:
        keeps[1] = rasterize_masks(H, W, 1.0, KEEP_POLY)
        assert 0 < int((keeps[1] == 0).sum()) < keeps[1].size
    return keeps, [Ref(H, W, k, keeps[s]) for s in range(S)]


def batches(name):
    """The case's frames, cut into its batches: [n][S][H][W][3] each."""
    W, H, _k, S, sizes = CASES[name][:5]
    clip = colour_ref.noise_clip(W, H, S, sum(sizes), SEED)
    cuts = np.cumsum((0,) + tuple(sizes))
    return [np.ascontiguousarray(clip[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def reference_batch(refs, fr):
    """Every (frame, stream) of a batch through the references, and the coverage the docstring promises."""
    out = [[ref.step(fr[t, s]) for s, ref in enumerate(refs)] for t in range(fr.shape[0])]
    if fr.shape[0] > 1:
        h, w = out[0][0]["thresh"].shape
        x0, y0 = 64 * ((w - 1) // 64), 64 * ((h - 1) // 64)
        for what, hit in (("column", [any(r["thresh"][:, x0:].any() for r in row) for row in out]),
                          ("row", [any(r["thresh"][y0:].any() for r in row) for row in out])):
            assert any(hit) and not all(hit), f"last tile {what}: {sum(hit)} of {len(hit)} frames have bits"
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_block_flushes_and_tails(name):
    W, H, k, S, sizes, _Ref, kw, path, ran, not_ran = CASES[name]
    keeps, refs = make_refs(name)
    eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=W, ksize=k, threshold=THRESH, avg=ALPHA,
                       max_batch=max(sizes), profile="pix", **kw)
    try:
        assert eng.pixel_path == path and eng.work_shape == (H, W)
        for s in range(S):
            if keeps[s] is not None:
                eng.set_mask(s, keeps[s])
        seen = 0
        for i, fr in enumerate(batches(name)):
            want = reference_batch(refs, fr)
            eng.submit(fr)
            eng.wait()
            counts = eng.counts()
            assert counts.shape == (fr.shape[0], S)
            for t in range(fr.shape[0]):
                for s in range(S):
                    r, at = want[t][s], f"{name} batch {i} ({fr.shape[0]} frames) frame {t} stream {s}"
                    np.testing.assert_array_equal(eng.threshold_bits(t, s), colour_ref.threshold_bits(r["thresh"]),
                                                  err_msg="threshold bits " + at)
                    assert counts[t, s] == r["count"], at
                    got = eng.contours(t, s)
                    assert [c.bbox for c in got] == r["boxes"], at
                    assert [c.origin for c in got] == r["origins"], at
                    seen += r["count"]
        assert seen > 0
        for s in range(S):
            refs[s].check_state(eng, s)
        names = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0}
        assert ran <= names and not names & not_ran, names
    finally:
        eng.close()
