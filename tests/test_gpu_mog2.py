"""GPU: the Gaussian-mixture background model (FM_FLAG_MOG2; k_small_blur or k_wide_blur + fm_mog2.hip's
k_mog2_scan) through the C ABI, bit for bit against tests/mog2_ref.py (OpenCV's MOG2 restated in float32 numpy and
composed with the oracle's stages).

Every case compares, on every frame of every stream: the undilated threshold bits, the dilated mask, the contour
count, the boxes and origins (and the points where asked); and after every batch nmodes, then weight, mean and
variance at the modes below nmodes bit for bit, nframes and the background image.  That each clip reaches every
branch of the kernel is asserted from the restatement alone in tests/test_mog2_host.py.

Shapes (work w x h) and what each is for:
  96 x 80         the flickering block: the average engine fires on it, the mixture waits for the mover
  66 x 70         2 x 2 tiles with a 2-px last tile column and a 6-row last tile row, two streams, history 6,
                  batches of 1, 7, 65 and then 3 frames in flight, a keep-mask on stream 1; ksize 1, 5, 21,
                  shadows off, a fixed learning rate
  1x1, 2x2, 3x2   the smallest images
  100 x 56        mode D's work image, INTER_AREA from 1920 x 1080
  64 x 129        a third tile row one row tall
  200 x 130       more than 16,384 pixels: k_wide_blur in front, at ksize 5
"""
import numpy as np
import pytest

import mog2_ref as R
from find_motion_amd import MotionEngine, motion, rasterize_masks, videoio
from find_motion_amd import _native
from find_motion_amd._native import FM_EINVAL, FM_ESTATE, FMError
from oracle.decision import written_indices

pytestmark = pytest.mark.gpu

F = np.float32
ENGINE_KEYS = ("history", "var_threshold", "var_threshold_gen", "background_ratio", "var_init", "var_min", "var_max",
               "complexity_reduction", "shadow_tau", "detect_shadows", "learning_rate")


class Pair:
    """A mog2 engine and one Mog2Stream per stream, driven together."""

    def __init__(self, W, H, box, k, S=1, T=8, prm=None, keeps=None, **kw):
        self.S = S
        prm = R.params() if prm is None else prm
        self.eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=box, ksize=k, threshold=12, avg=0.1,
                                max_batch=T, mog2={key: prm[key] for key in ENGINE_KEYS}, **kw)
        assert self.eng.pixel_path == "mog2" and self.eng.mog2.history == prm["history"]
        keeps = keeps or [None] * S
        self.ref = [R.Mog2Stream(H, W, box, k, prm, keep=keeps[s]) for s in range(S)]
        assert self.eng.work_shape == (self.ref[0].h, self.ref[0].w)
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
                np.testing.assert_array_equal(eng.threshold_bits(t, s), R.threshold_bits(ref["thresh"]),
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

    def compare_model(self, tag=""):
        for s in range(self.S):
            got = self.eng.mog2_model(s)
            w, m, v, n = self.ref[s].arrays()
            at = f"{tag} stream {s}"
            np.testing.assert_array_equal(got["nmodes"], n, err_msg="nmodes " + at)
            for name, want in (("weight", w), ("mean", m), ("var", v)):  # (zeros at mode >= nmodes on both sides)
                assert got[name].dtype == F and got[name].tobytes() == want.tobytes(), \
                    f"{name} {at}: {int((got[name].view(np.uint32) != want.view(np.uint32)).sum())} values differ"
            assert got["nframes"] == self.ref[s].nframes, at
            np.testing.assert_array_equal(self.eng.mog2_background(s), self.ref[s].background_image(),
                                          err_msg="background image " + at)

    def step(self, fr, tag=""):
        self.eng.submit(fr)
        out = self.compare(fr, tag)
        self.compare_model(tag)
        return out


def test_flicker_average_engine_fires_mixture_waits_for_the_mover():
    fr = R.flicker_clip()[:, None]  # [24][1][80][96][3]
    n, at = fr.shape[0], R.FLICKER_MOVER_AT
    avg = MotionEngine(n_streams=1, src_w=96, src_h=80, box_size=96, ksize=5, threshold=12, avg=0.1, max_batch=n)
    avg.submit(fr)
    avg.wait()
    fired = avg.counts()[:, 0]
    avg.close()
    assert int((fired[:at] > 0).sum()) >= at - 2, fired.tolist()
    p = Pair(96, 80, 96, 5, T=n, contour_points=True)
    counts = p.step(fr)
    assert counts[:at] == [0] * at and all(c >= 1 for c in counts[at:at + 8]), counts
    p.close()


@pytest.fixture(scope="module")
def tail_frames():
    """66 x 70, two streams, 1 + 7 + 65 frames and the batches that fill the pipeline."""
    return R.tail_clip()


@pytest.mark.parametrize("name,k,ov", R.TAIL_CONFIGS, ids=[c[0] for c in R.TAIL_CONFIGS])
def test_two_streams_keep_mask_batches_in_flight(tail_frames, name, k, ov):
    """Batches of 1, 7 (the model carried over) and 65 frames (a block flush past 64) and then 3-frame ones,
    fm_max_inflight of them submitted before the first wait; stream 1 under a polygon keep-mask."""
    W, H = R.TAIL_W, R.TAIL_H
    keep = rasterize_masks(H, W, 1.0, R.TAIL_KEEP_POLY)
    assert 0 < int((keep == 0).sum()) < keep.size
    p = Pair(W, H, W, k, S=2, T=65, prm=R.params(history=R.TAIL_HISTORY, **ov), keeps=[None, keep])
    assert 3 <= p.eng.max_inflight <= len(R.TAIL_SIZES)
    sizes = R.TAIL_SIZES[:p.eng.max_inflight]
    parts, pos = [], 0
    for n in sizes:
        parts.append(np.ascontiguousarray(tail_frames[pos:pos + n]))
        pos += n
    for fr in parts:
        p.eng.submit(fr)
    with pytest.raises(FMError) as e:  # a batch is in flight
        p.eng.mog2_model(0)
    assert e.value.code == FM_ESTATE
    for i, fr in enumerate(parts):
        p.compare(fr, f"{name} batch {i}")
    p.compare_model(name)
    # and one batch at a time from there, the model compared after each
    while pos + 3 <= tail_frames.shape[0]:
        p.step(np.ascontiguousarray(tail_frames[pos:pos + 3]), f"{name} frame {pos}")
        pos += 3
    assert p.seen > 0
    p.close()


@pytest.mark.parametrize("name,shape,T", [("1x1", (1, 1), 5), ("2x2", (2, 2), 5), ("3x2", (2, 3), 5),
                                          ("100x56", (56, 100), 8), ("64x129", (129, 64), 7), ("200x130", (130, 200), 9)])
def test_shapes(name, shape, T):
    """The smallest images, mode D's work image after INTER_AREA, a third tile row one row tall, and an image past
    k_small_blur's (k_wide_blur in front, at ksize 5)."""
    fr, (H, W, box, k, prm), S = R.band_case(name)
    p = Pair(W, H, box, k, S=S, T=T, prm=prm)
    assert p.eng.work_shape == shape
    for i in range(0, fr.shape[0], T):
        p.step(np.ascontiguousarray(fr[i:i + T]), f"{name} batch {i // T}")
    assert p.seen > 0
    p.close()


def test_reset_stream_mid_sequence():
    fr, (H, W, box, k, prm), S = R.band_case("reset")
    p = Pair(W, H, box, k, S=S, T=8, prm=prm)
    p.step(np.ascontiguousarray(fr[:8]))
    p.eng.reset(1)  # stream 1 starts over (nmodes = 0, nframes = 0); stream 0 carries on
    p.ref[1].reset()
    got = p.eng.mog2_model(1)
    assert got["nframes"] == 0 and not got["nmodes"].any() and not got["weight"].any()
    assert not p.eng.mog2_background(1).any()
    p.step(np.ascontiguousarray(fr[8:16]), "after the reset")
    p.step(np.ascontiguousarray(fr[16:24]), "second batch after the reset")
    assert p.ref[0].nframes == 24 and p.ref[1].nframes == 16
    p.close()


def adversarial_model(h, w, prm, nframes):
    """Models at the edges of the update's comparisons, column by column (every row the same); the rate of the next
    frame is that of frame nframes + 1."""
    a = R.learning_rate(prm, nframes + 1)
    a1 = F(1) - a
    cut = a * F(prm["complexity_reduction"])  # -prune
    TB = F(prm["background_ratio"])
    up, dn = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
    wt, mean, var = (np.zeros((5, h, w), F) for _ in range(3))
    nm = np.zeros((h, w), np.uint8)

    def put(x, modes):
        nm[:, x] = len(modes)
        for i, (ww, mm, vv) in enumerate(modes):
            wt[i, :, x], mean[i, :, x], var[i, :, x] = ww, mm, vv

    x = 0
    for lvl in (100.0, 125.0):
        # equal weights in adjacent modes: the second one fits and meets `w < weight[i - 1]` at a tie or next to it
        for w1 in (F(0.4), up(0.4), dn(0.4)):
            put(x, [(F(0.4), F(30), F(15)), (w1, F(lvl), F(15)), (F(0.2), F(220), F(15))])
            x += 1
        # five modes, the last one's decayed weight just above and just below -prune (it does not fit)
        for w5 in (up((cut + cut) / a1), dn((cut + cut) / a1), (cut + cut) / a1):
            put(x, [(F(0.5), F(lvl), F(15)), (F(0.2), F(10), F(15)), (F(0.15), F(60), F(15)), (F(0.1), F(180), F(15)),
                    (w5, F(240), F(15))])
            x += 1
        # a mode of mean 0 ahead of the fitting one; variances at var_min and var_max
        put(x, [(F(0.6), F(0), F(prm["var_min"])), (F(0.4), F(lvl), F(prm["var_max"]))])
        put(x + 1, [(F(0.7), F(lvl), F(prm["var_min"])), (F(0.3), F(0), F(prm["var_max"]))])
        x += 2
        # total just below and just above TB when the second mode is reached
        for w0 in (dn(TB), TB, up(TB)):
            put(x, [(w0, F(30), F(15)), (F(1) - w0, F(lvl), F(15))])
            x += 1
        for w0 in (dn((TB + cut) / a1), (TB + cut) / a1, up((TB + cut) / a1)):  # ... after this frame's decay
            put(x, [(w0, F(30), F(15)), (F(1) - w0, F(lvl), F(15))])
            x += 1
    assert x <= w and float(wt.max()) < 1.0 and float(wt.min()) >= 0.0
    return wt, mean, var, nm


def test_written_models_round_trip_and_continue():
    fr, (H, W, box, k, prm), S = R.band_case("written")
    p = Pair(W, H, box, k, T=8, prm=prm)
    p.step(np.ascontiguousarray(fr[:8]))
    for nframes in (8, 40):  # (the rate is the history's 1 / 12 from frame 6 on)
        wt, mean, var, nm = adversarial_model(H, W, prm, nframes)
        p.eng.set_mog2_model(0, wt, mean, var, nm, nframes)
        p.ref[0].set_arrays(wt, mean, var, nm, nframes)
        got = p.eng.mog2_model(0)  # back bit for bit, zeros at mode >= nmodes
        assert got["nframes"] == nframes and np.array_equal(got["nmodes"], nm)
        for name, want in (("weight", wt), ("mean", mean), ("var", var)):
            assert got[name].tobytes() == want.tobytes(), name
        p.compare_model(f"written at {nframes}")
        # uniform frames at the levels the written modes sit at, then the clip again
        lv = np.full((4, 1, H, W), 100, np.uint8)
        lv[1], lv[2], lv[3] = 125, 240, 0
        p.step(R.gray_frames(lv), f"levels after the model written at {nframes}")
        p.step(np.ascontiguousarray(fr[8:16]), f"clip after the model written at {nframes}")
    # what lies at mode >= nmodes is ignored
    wt, mean, var, nm = adversarial_model(H, W, prm, 5)
    junk = [np.where(np.arange(5)[:, None, None] >= nm[None], F(7), a) for a in (wt, mean, var)]
    p.eng.set_mog2_model(0, *junk, nm, 5)
    p.ref[0].set_arrays(wt, mean, var, nm, 5)
    p.compare_model("junk above nmodes")
    p.step(np.ascontiguousarray(fr[16:24]), "after junk above nmodes")
    bad = nm.copy()
    bad[3, 4] = 6
    with pytest.raises(FMError) as e:
        p.eng.set_mog2_model(0, wt, mean, var, bad, 5)
    assert e.value.code == FM_EINVAL
    with pytest.raises(ValueError):
        p.eng.set_mog2_model(0, wt[:4], mean, var, nm, 5)
    p.close()


def test_state_calls_by_context_kind_and_profile_name():
    base = dict(n_streams=1, src_w=96, src_h=80, box_size=96, ksize=5, threshold=12, avg=0.1, max_batch=4)
    fr = R.flicker_clip(4)[:, None]
    plain = MotionEngine(**base)
    assert plain.mog2 is None and plain.pixel_path == "small"
    plain.submit(fr)
    plain.wait()
    for call in (lambda: plain.mog2_model(0), lambda: plain.mog2_background(0),
                 lambda: plain.set_mog2_model(0, *(np.zeros((5, 80, 96), F),) * 3, np.zeros((80, 96), np.uint8), 0)):
        with pytest.raises(FMError) as e:
            call()
        assert e.value.code == FM_ESTATE
    assert plain.background(0).shape == (80, 96)
    plain.close()
    eng = MotionEngine(mog2=True, profile=True, **base)  # fm_create_mog2 with the defaults
    assert eng.mog2.as_dict() == _native.Mog2Params().as_dict()
    eng.submit(fr)
    eng.wait()
    with pytest.raises(FMError) as e:
        eng.background(0)
    assert e.value.code == FM_ESTATE and "mog2_background" in str(e.value)
    with pytest.raises(FMError) as e:
        eng.set_background(0, np.zeros((80, 96)))
    assert e.value.code == FM_ESTATE
    names = eng.kernel_times()
    assert "mog2_scan" in names and "small_blur" in names, names
    assert eng.mog2_background(0)[0, 0] == 30
    eng.close()


def test_dropin_writes_what_the_restatement_counts_select(tmp_path):
    fr = R.flicker_clip()
    ref = R.Mog2Stream(R.FLICKER_H, R.FLICKER_W, R.FLICKER_W, 5)
    counts = [ref.step(f)["count"] for f in fr]
    want = written_indices(counts, fps=30, min_time=0.1, cache_time=0.1)
    assert want
    kw = dict(batch=4, box_size=96, blur_scale=19, threshold=12, avg=0.1, cache_time=0.1, min_time=0.1, fps=30,
              outdir=str(tmp_path))
    vm = motion.VideoMotion(filename=str(tmp_path / "mog2"), capture=videoio.ArrayCapture(fr), background_model="mog2", **kw)
    assert vm.gaussian == (5, 5) and vm.engine.pixel_path == "mog2" and not vm.keep_planes
    wrote, err, _ = vm.find_motion()
    assert wrote is True and err == "" and vm.written_indices == want
    plain = motion.VideoMotion(filename=str(tmp_path / "avg"), capture=videoio.ArrayCapture(fr), **kw)
    wrote, err, _ = plain.find_motion()
    assert wrote is True and set(plain.written_indices) > set(want)
