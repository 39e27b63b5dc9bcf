"""GPU: motion per colour channel (FM_FLAG_COLOUR_MOTION; fm_rgb.hip: k_rgb_blur + k_rgb_scan) through the C
ABI, bit for bit against tests/colour_ref.py (the chain without cvtColor, composed from the oracle's stages).

Every case compares, on every frame of every stream: the contour count, the boxes and origins, the dilated mask
and the undilated threshold bits; and the (h, w, 3) float64 background after every batch.  The conditions that
make the comparisons mean something are asserted from the reference alone in tests/test_colour_host.py.

Shapes (work w x h) and what each is for:
  96 x 80         the isoluminant mover: invisible to the gray engine, seen by the colour engine
  66 x 70         2 x 2 tiles with a 2-px last tile column and a 6-row last tile row; 3hw % 16 = 4, so
                  accumulateWeighted's scalar tail is the last pixel and channel R of the one before it
  1x1, 2x2, 3x2   3hw = 3, 12 (convertScaleAbs's double path, all tail) and 18 (float path, 2 tail elements)
  100 x 56        mode D's work image, INTER_AREA from 1920 x 1080
  64 x 129        a third tile row one row tall
"""
import numpy as np
import pytest

import colour_ref
from colour_ref import ColourStream
from find_motion_amd import MotionEngine, motion, rasterize_masks, videoio
from find_motion_amd import _native
from find_motion_amd._native import FM_ENOTSUP, FMError
from oracle.decision import written_indices

pytestmark = pytest.mark.gpu

SEED = colour_ref.TAIL_SEED


class Pair:
    """A colour engine and one ColourStream per stream, driven together."""

    def __init__(self, W, H, box, k, S=1, T=8, thresh=12, alpha=0.1, keeps=None, **kw):
        self.S = S
        self.eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=box, ksize=k, threshold=thresh, avg=alpha,
                                max_batch=T, colour_motion=True, **kw)
        assert self.eng.pixel_path == "rgb" and self.eng.colour_motion
        keeps = keeps or [None] * S
        self.ref = [ColourStream(H, W, box, k, thresh, alpha, keep=keeps[s]) for s in range(S)]
        assert self.eng.work_shape == (self.ref[0].h, self.ref[0].w)
        assert self.eng.background_shape == self.ref[0].bg.shape
        for s in range(S):
            if keeps[s] is not None:
                self.eng.set_mask(s, keeps[s])
        self.points = bool(kw.get("contour_points"))
        self.seen = 0

    def close(self):
        self.eng.close()

    def compare(self, fr, tag=""):
        """wait() for the oldest batch in flight, whose frames are fr [n][S][H][W][3], and compare all of it."""
        eng = self.eng
        eng.wait()
        counts = eng.counts()
        assert counts.shape == (fr.shape[0], self.S)
        out = []
        for t in range(fr.shape[0]):
            for s in range(self.S):
                ref = self.ref[s].step(fr[t, s], with_points=self.points)
                at = f"{tag} frame {t} stream {s}"
                np.testing.assert_array_equal(eng.threshold_bits(t, s), colour_ref.threshold_bits(ref["thresh"]),
                                              err_msg="threshold bits " + at)
                np.testing.assert_array_equal(eng.mask(t, s), ref["mask"], err_msg="mask " + at)
                assert counts[t, s] == ref["count"], at
                got = eng.contours(t, s)
                assert [c.bbox for c in got] == ref["boxes"], at
                assert [c.origin for c in got] == ref["origins"], at
                if self.points:
                    for c, r in zip(got, ref["contours"]):
                        np.testing.assert_array_equal(c.points.reshape(-1, 2), r["points"], err_msg="points " + at)
                self.seen += ref["count"]
                out.append(ref["count"])
        return out

    def compare_background(self, tag=""):
        for s in range(self.S):
            bg = self.eng.background(s)
            assert bg.shape == self.ref[s].bg.shape
            assert np.array_equal(bg, self.ref[s].bg), \
                f"{tag} background stream {s}: {int((bg != self.ref[s].bg).sum())} values differ"

    def step(self, fr, tag=""):
        self.eng.submit(fr)
        out = self.compare(fr, tag)
        self.compare_background(tag)
        return out


def test_isoluminant_mover_gray_engine_blind_colour_engine_exact():
    fr = colour_ref.iso_clip()[:, None]  # [6][1][80][96][3]
    gray = MotionEngine(n_streams=1, src_w=96, src_h=80, box_size=96, ksize=5, threshold=12, avg=0.1, max_batch=6)
    gray.submit(fr)
    gray.wait()
    assert gray.counts().tolist() == [[0]] * 6
    gray.close()
    p = Pair(96, 80, 96, 5, T=6, contour_points=True)
    counts = p.step(fr)
    assert counts[0] == 0 and all(c >= 1 for c in counts[1:]), counts
    p.close()


@pytest.fixture(scope="module")
def tail_frames():
    """66 x 70, two streams with different content, 1 + 7 + 65 frames and the batches that fill the pipeline."""
    return colour_ref.tail_clip()


@pytest.mark.parametrize("k", [1, 3, 5, 21, 49])
def test_noise_two_streams_keep_mask_batches_in_flight(tail_frames, k):
    """Batches of 1 (the init frame alone), 7 (the background carried over) and 65 frames (a block flush past 64)
    and then 3-frame ones, fm_max_inflight of them submitted before the first wait; stream 1 under a polygon
    keep-mask; the accumulate tail splits a pixel's channels."""
    W, H = 66, 70
    keep = rasterize_masks(H, W, 1.0, [[(8, 6), (50, 12), (40, 60), (12, 44)]])
    assert 0 < int((keep == 0).sum()) < keep.size
    p = Pair(W, H, W, k, S=2, T=65, keeps=[None, keep])
    assert 3 <= p.eng.max_inflight <= len(colour_ref.TAIL_SIZES)
    sizes = colour_ref.TAIL_SIZES[:p.eng.max_inflight]
    parts, pos = [], 0
    for n in sizes:
        parts.append(np.ascontiguousarray(tail_frames[pos:pos + n]))
        pos += n
    for fr in parts:
        p.eng.submit(fr)
    for i, fr in enumerate(parts):
        p.compare(fr, f"k {k} batch {i}")
    p.compare_background(f"k {k}")
    assert p.seen > 0
    p.close()


@pytest.mark.parametrize("W,H,box,shape", [(4, 4, 1, (1, 1)), (4, 4, 2, (2, 2)), (6, 4, 3, (2, 3)),
                                           (1920, 1080, 100, (56, 100))])
def test_small_work_images_after_inter_area(W, H, box, shape):
    n = 6 if W > 100 else 20
    fr = colour_ref.noise_clip(W, H, 1, n, SEED + W)
    p = Pair(W, H, box, 5, T=4)
    assert p.eng.work_shape == shape
    for i in range(0, n - 4, 4):
        p.step(np.ascontiguousarray(fr[i:i + 4]), f"{shape} batch {i // 4}")
    # .5 ties and values next to them, negatives and values above 255: convertScaleAbs's path at this 3hw
    rng = np.random.default_rng(7)
    bg = np.floor(rng.random(shape + (3,)) * 300 - 20) + rng.choice([0.5, -0.5, np.nextafter(0.5, 0), 0.25, 1.5],
                                                                  size=shape + (3,))
    bg.reshape(-1)[0] = np.nextafter(101.5, 0.0)
    p.eng.set_background(0, bg)
    p.ref[0].set_background(bg)
    p.step(np.ascontiguousarray(fr[n - 4:]), f"{shape} after the written background")
    if shape == (56, 100):
        assert p.seen > 0
    p.close()


def test_third_tile_row_one_row_tall():
    W, H = 64, 129
    fr = colour_ref.noise_clip(W, H, 1, 9, SEED + 1)
    fr[3:, 0, 126:, 20:40] = (10, 240, 10)  # something on the last rows
    p = Pair(W, H, W, 5, T=5)
    p.step(np.ascontiguousarray(fr[:5]))
    p.step(np.ascontiguousarray(fr[5:]))
    assert p.seen > 0
    p.close()


def test_reset_stream_mid_sequence_and_background_round_trip():
    W, H = 66, 70
    fr = colour_ref.noise_clip(W, H, 2, 12, SEED + 2)
    p = Pair(W, H, W, 3, S=2, T=4)
    p.step(np.ascontiguousarray(fr[:4]))
    p.eng.reset(1)          # stream 1 starts over: its next frame is its background; stream 0 carries on
    p.ref[1].reset()
    p.step(np.ascontiguousarray(fr[4:8]), "after the reset")
    # a written background comes back bit for bit, in (h, w, 3) order, and the next batch starts from it
    rng = np.random.default_rng(11)
    bg = rng.random((H, W, 3)) * 280 - 10
    bg[0, 0] = (1.0, 2.0, 3.0)
    p.eng.set_background(0, bg)
    p.ref[0].set_background(bg)
    back = p.eng.background(0)
    assert back.shape == (H, W, 3) and np.array_equal(back, bg) and back[0, 0].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        p.eng.set_background(0, bg[..., 0])
    p.step(np.ascontiguousarray(fr[8:]), "after the written background")
    p.close()


def test_status_codes_plan_and_background_channels():
    import ctypes as C

    base = dict(n_streams=1, src_w=96, src_h=80, box_size=96, threshold=12, avg=0.1, max_batch=2)
    for bad in (dict(ksize=51), dict(ksize=5, keep_planes=True)):
        with pytest.raises(FMError) as e:
            MotionEngine(colour_motion=True, **{**base, **bad})
        assert e.value.code == FM_ENOTSUP
    assert _native.plan(src_w=96, src_h=80, box_size=96, ksize=5, colour_motion=True)["pixel_path"] == "rgb"
    L = _native.load()
    for flag, want, path in ((False, 1, "small"), (True, 3, "rgb")):
        eng = MotionEngine(ksize=5, colour_motion=flag, **base)
        ch = C.c_int(0)
        assert L.fm_background_channels(eng._h, C.byref(ch)) == 0 and ch.value == want
        assert eng.pixel_path == path and eng.background_shape == (80, 96) + ((3,) if flag else ())
        eng.close()


def test_dropin_writes_what_the_reference_counts_select(tmp_path):
    fr = colour_ref.iso_clip(n=20)
    ref = ColourStream(80, 96, 96, 5, thresh=12, alpha=0.1)
    counts = [ref.step(f)["count"] for f in fr]
    want = written_indices(counts, fps=30, min_time=0.1, cache_time=0.1)
    assert want
    kw = dict(batch=4, box_size=96, blur_scale=19, threshold=12, avg=0.1, cache_time=0.1, min_time=0.1, fps=30,
              outdir=str(tmp_path))
    vm = motion.VideoMotion(filename=str(tmp_path / "colour"), capture=videoio.ArrayCapture(fr), colour_motion=True, **kw)
    assert vm.gaussian == (5, 5) and vm.engine.pixel_path == "rgb" and not vm.keep_planes
    wrote, err, _ = vm.find_motion()
    assert wrote is True and err == "" and vm.written_indices == want
    plain = motion.VideoMotion(filename=str(tmp_path / "gray"), capture=videoio.ArrayCapture(fr), **kw)
    wrote, err, _ = plain.find_motion()
    assert plain.written_indices == [] and not wrote
