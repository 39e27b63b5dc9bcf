"""CPU: the Gaussian-mixture reference's own properties (tests/mog2_ref.py), asserted from the restatement alone,
the status codes of the C ABI that are decided before any device call, and the drop-in's plumbing.

These are the conditions under which the GPU tests of tests/test_gpu_mog2.py mean something: the scalar (line for
line) and the vectorised statement of apply() agree bit for bit; the single-pixel sequences behave as
BackgroundSubtractorMOG2 does; and every clip the GPU tests run reaches every branch the kernel has (the event
counters), so a clip that stops exercising a branch fails here.
"""
import ctypes as C
import logging

import numpy as np
import pytest

import mog2_ref as R
from fake_engine import OracleEngine
from find_motion_amd import _native, cli, motion, rasterize_masks, videoio
from find_motion_amd._native import FM_EINVAL, FM_ENOTSUP, FM_OK, FMError, FMParams, Mog2Params

H6 = R.params(history=6)


def seeded_levels(n=40, h=6, w=7, seed=3):
    """Per-pixel content that reaches every event: columns play SEQ_ALL at different phases, the rest seeded
    PALETTE levels with +-3 noise."""
    rng = np.random.default_rng(seed)
    lv = rng.choice(R.PALETTE, size=(n, h, w)) + rng.integers(-3, 4, size=(n, h, w))
    for x in range(3):
        lv[:, :, x] = np.asarray(R.SEQ_ALL)[(np.arange(n) + 5 * x) % len(R.SEQ_ALL)][:, None]
    return np.clip(lv, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("ov", [{}, {"detect_shadows": 0}, {"learning_rate": 0.05}, {"learning_rate": 0.0}])
def test_scalar_and_vectorised_agree_bit_for_bit(ov):
    prm = R.params(history=R.ALL_HISTORY, **ov)
    lv = seeded_levels()
    n, h, w = lv.shape
    model = R.Mog2Model(h * w)
    pix = [R.PixelModel() for _ in range(h * w)]
    evv, evs = dict.fromkeys(R.EVENTS, 0), dict.fromkeys(R.EVENTS, 0)
    for t in range(n):
        a = R.learning_rate(prm, t + 1)
        d = lv[t].reshape(-1)
        fg = model.apply(d.astype(np.float32), a, prm, evv)
        fs = [R.apply_scalar(pix[i], d[i], a, prm, evs) for i in range(h * w)]
        assert fg.tolist() == fs, f"frame {t}"
        assert evv == evs, f"frame {t}"
        for i, px in enumerate(pix):
            assert model.n[i] == px.n
            for arr, lst in ((model.w, px.w), (model.m, px.m), (model.v, px.v)):
                got, want = arr[:px.n, i], np.asarray(lst[:px.n], np.float32)
                assert got.tobytes() == want.tobytes(), f"frame {t} pixel {i}"
        bgv = model.background(prm)
        assert bgv.tolist() == [R.background_scalar(px, prm) for px in pix]
    if not ov:
        assert min(evv.values()) > 0, evv


def test_flickering_pixel_is_learnt_and_the_average_fires():
    out, _, px = R.run_pixel(R.SEQ_FLICKER)
    assert out == [127, 127] + [0] * 38 and px.n == 2
    # the project's chain at -t 12 -a 0.1 on the same pixel (a uniform frame: the blur is the level)
    fr = R.gray_frames(np.broadcast_to(np.asarray(R.SEQ_FLICKER, np.uint8)[:, None, None], (40, 16, 16)))
    fired = sum(c > 0 for c in R.gray_counts(fr, box=16, ksize=5, thresh=12, alpha=0.1))
    assert fired >= 30, fired
    # and a value the mixture has not seen is still foreground
    assert R.run_pixel(R.SEQ_FLICKER[:10] + [200])[0][-1] == 255


def test_single_pixel_sequences():
    assert R.run_pixel(R.SEQ_SHADOW)[0][20:23] == [127] * 3
    assert R.run_pixel(R.SEQ_SHADOW, shadows=0)[0][20:23] == [255] * 3
    assert R.run_pixel(R.SEQ_DARK)[0][20:] == [255] * 3   # darker than half the background: no shadow
    out, ev, px = R.run_pixel(R.SEQ_PRUNE, H6)
    assert ev["prunes"] == 1 and px.n == 1
    out, ev, px = R.run_pixel(R.SEQ_VARMAX, H6)
    assert ev["var_max_clamps"] > 0 and np.float32(75) in px.v[:px.n]
    out, ev, px = R.run_pixel(R.SEQ_ZERO, H6)
    assert out == [255, 0, 0, 0, 0, 255, 0, 0, 0] and ev["zero_mean_outs"] > 0
    out, ev, _ = R.run_pixel(R.SEQ_ALL, R.params(history=R.ALL_HISTORY))
    assert min(ev.values()) > 0, ev


def test_first_frame_is_shadow_where_the_blur_is_not_zero():
    lv = np.array([[0, 1], [200, 255]], np.uint8)
    for shadows, want in ((1, [[255, 127], [127, 127]]), (0, [[255, 255], [255, 255]])):
        st = R.Mog2Stream(2, 2, 2, 1, R.params(detect_shadows=shadows))
        assert st.step(R.gray_frames(lv))["fgmask"].tolist() == want
    # a masked pixel's blur is 0: foreground on the first frame
    st = R.Mog2Stream(2, 2, 2, 1, keep=np.array([[1, 0], [1, 1]], np.uint8))
    assert st.step(R.gray_frames(np.full((2, 2), 90, np.uint8)))["fgmask"].tolist() == [[127, 255], [127, 127]]


def events_of(frames, args, S, keeps=None):
    H, W, box, k, prm = args
    sts = [R.Mog2Stream(H, W, box, k, prm, keep=None if keeps is None else keeps[s]) for s in range(S)]
    counts = [[sts[s].step(frames[t, s])["count"] for s in range(S)] for t in range(frames.shape[0])]
    return {e: sum(st.events[e] for st in sts) for e in R.EVENTS}, counts


@pytest.fixture(scope="module")
def tail_frames():
    return R.tail_clip()


@pytest.mark.parametrize("name,k,ov", R.TAIL_CONFIGS, ids=[c[0] for c in R.TAIL_CONFIGS])
def test_tail_clip_reaches_every_event(tail_frames, name, k, ov):
    keep = rasterize_masks(R.TAIL_H, R.TAIL_W, 1.0, R.TAIL_KEEP_POLY)
    prm = R.params(history=R.TAIL_HISTORY, **ov)
    ev, counts = events_of(tail_frames, (R.TAIL_H, R.TAIL_W, R.TAIL_W, k, prm), 2, [None, keep])
    # (without shadow detection the two counters of detectShadowGMM cannot move: that run is there for the other path)
    need = [e for e in R.EVENTS if prm["detect_shadows"] or e not in ("shadows", "zero_mean_outs")]
    assert all(ev[e] > 0 for e in need), ev
    assert sum(map(sum, counts)) > 0


@pytest.mark.parametrize("name", list(R.BAND_CASES))
def test_band_clips_reach_every_event(name):
    fr, args, S = R.band_case(name)
    ev, counts = events_of(fr, args, S)
    assert min(ev.values()) > 0, ev
    assert sum(map(sum, counts)) > 0


def test_flicker_clip_average_fires_mixture_waits_for_the_mover():
    """The flicker clip runs at OpenCV's defaults, where nothing is pruned or replaced within 24 frames (a mode made
    at frame k starts at 1 / 2k and the prune level is 0.05 / 2n): it is there for the decision, and reaches the
    events of a two-mode pixel."""
    fr = R.flicker_clip()
    st = R.Mog2Stream(R.FLICKER_H, R.FLICKER_W, R.FLICKER_W, 5)
    counts = [st.step(f)["count"] for f in fr]
    at = R.FLICKER_MOVER_AT
    assert counts[:at] == [0] * at and all(c >= 1 for c in counts[at:at + 8]), counts
    avg = R.gray_counts(fr, box=R.FLICKER_W, ksize=5, thresh=12, alpha=0.1)
    assert sum(c > 0 for c in avg[:at]) >= at - 2, avg
    assert all(st.events[e] > 0 for e in ("fits", "swaps", "var_min_clamps", "shadows")), st.events


# ---------------------------------------------------------------------------------------------------------------
# the C ABI: what is decided before any device call


def _params(flags=_native.FM_FLAG_MOG2, **kw):
    base = dict(device=0, n_streams=1, src_w=96, src_h=80, box_size=96, ksize=5, threshold=12, avg=0.1, max_batch=2,
                max_contours=64)
    base.update(kw)
    return FMParams(base["device"], base["n_streams"], base["src_w"], base["src_h"], base["box_size"], base["ksize"],
                    base["threshold"], base["avg"], base["max_batch"], base["max_contours"], flags)


def test_defaults_and_exported_names():
    L = _native.load()
    d = Mog2Params(history=1)
    assert L.fm_mog2_defaults(C.byref(d)) == FM_OK
    for k, v in R.DEFAULTS.items():  # the floats as float32 holds them
        assert getattr(d, k) == (v if k in ("history", "detect_shadows", "learning_rate") else float(np.float32(v))), k
    assert Mog2Params().as_dict() == d.as_dict()
    assert L.fm_mog2_defaults(None) == FM_EINVAL
    for name in ("fm_mog2_defaults", "fm_create_mog2", "fm_mog2_read_model", "fm_mog2_write_model", "fm_mog2_background"):
        assert name in _native.EXPORTED and hasattr(L, name)
    assert _native.FM_FLAG_MOG2 == 0x80 and L.fm_abi_version() == 1


@pytest.mark.parametrize("bad", [dict(history=0), dict(var_threshold=float("nan")), dict(var_threshold_gen=-1.0),
                                 dict(var_init=float("inf")), dict(var_min=80.0), dict(var_max=3.0),
                                 dict(background_ratio=0.0), dict(background_ratio=1.5), dict(shadow_tau=-0.5),
                                 dict(complexity_reduction=float("nan")), dict(learning_rate=1.5)])
def test_create_refuses_bad_parameters_before_any_device_call(bad):
    L = _native.load()
    h = C.c_void_p(1)
    p, m = _params(device=12345), Mog2Params(**bad)  # no such device: a device call would fail with FM_EHIP
    assert L.fm_create_mog2(C.byref(h), C.byref(p), C.byref(m)) == FM_EINVAL and not h.value
    with pytest.raises(FMError) as e:
        _native.MotionEngine(n_streams=1, src_w=96, src_h=80, box_size=96, ksize=5, threshold=12, avg=0.1, mog2=bad,
                             device=12345)
    assert e.value.code == FM_EINVAL


def test_plan_names_the_path_and_refuses_what_it_cannot_take():
    base = dict(src_w=1920, src_h=1080, box_size=100, ksize=5)
    assert _native.plan(**base)["pixel_path"] == "small"
    p = _native.plan(mog2=True, **base)
    assert p["pixel_path"] == "mog2" and p["work_shape"] == (56, 100) and p["max_inflight"] == 4
    for ok in (dict(box_size=1920, ksize=5), dict(box_size=1920, ksize=97), dict(box_size=100, ksize=1),
               dict(box_size=384, ksize=19)):
        assert _native.plan(mog2={"history": 6}, **{**base, **ok})["pixel_path"] == "mog2"
    for bad in (dict(colour_motion=True), dict(keep_planes=True),
                dict(src_w=8192, src_h=8192, box_size=8192),  # 16,384 tiles
                dict(box_size=1920, ksize=1)):                # k_wide_blur's taps are bytes; the image is not small
        with pytest.raises(FMError) as e:
            _native.plan(mog2=True, **{**base, **bad})
        assert e.value.code == FM_ENOTSUP, bad
    # the same codes from fm_create_mog2 and from fm_create with the flag, before any device call
    L = _native.load()
    h = C.c_void_p()
    for flags, kw in ((_native.FM_FLAG_COLOUR_MOTION, {}), (_native.FM_FLAG_KEEP_PLANES, {}),
                      (0, dict(src_w=8192, src_h=8192, box_size=8192)), (0, dict(src_w=1920, src_h=1080, box_size=1920, ksize=1))):
        p = _params(flags=flags, device=12345, **kw)
        assert L.fm_create_mog2(C.byref(h), C.byref(p), None) == FM_ENOTSUP
        p.flags |= _native.FM_FLAG_MOG2
        assert L.fm_create(C.byref(h), C.byref(p)) == FM_ENOTSUP
    # without the flag nothing about a plan changes
    assert _native.plan(**base) == _native.plan(mog2=None, **base) == _native.plan(mog2=False, **base)


def test_mog2_argument_forms():
    assert _native.mog2_params(None) is None and _native.mog2_params(False) is None
    assert _native.mog2_params(True).as_dict() == Mog2Params().as_dict()
    m = _native.mog2_params({"history": 6, "detect_shadows": False})
    assert m.history == 6 and m.detect_shadows == 0 and m.var_max == 75.0
    assert _native.mog2_params(m) is m
    with pytest.raises(TypeError):
        _native.mog2_params({"nmixtures": 3})
    with pytest.raises(TypeError):
        _native.mog2_params(7)


# ---------------------------------------------------------------------------------------------------------------
# the drop-in's plumbing


class Mog2Engine(OracleEngine):
    """fake_engine's stand-in with the restatement behind it, as MotionEngine(mog2=...) is from outside."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.mog2 = _native.mog2_params(kw.get("mog2"))
        c = self.cfg
        prm = R.params(**{k: v for k, v in self.mog2.as_dict().items() if k in ("history", "detect_shadows", "learning_rate")})
        self.mstreams = [R.Mog2Stream(c.H, c.W, c.box, c.ksize, prm) for _ in range(self.n_streams)]

    def initialized(self, s):
        return self.mstreams[s].nframes > 0

    def background(self, s):
        raise FMError(_native.FM_ESTATE, "use mog2_background")

    def mog2_background(self, s):
        return self.mstreams[s].background_image()

    def submit(self, frames):
        frames = np.asarray(frames)
        frames = frames[None] if frames.ndim == 4 else frames
        out = []
        for t in range(frames.shape[0]):
            row = []
            for s, st in enumerate(self.mstreams):
                r = st.step(frames[t, s])
                r["areas"] = [c["area"] for c in r["contours"]]
                row.append(r)
            out.append(row)
        self._queue.append(out)
        self.submits += 1

    def plane(self, which, t, s):
        raise AssertionError("planes requested on a mog2 engine")


class Factory:
    def __init__(self):
        self.kwargs = None

    def __call__(self, **kw):
        self.kwargs = dict(kw)
        return Mog2Engine(**kw) if kw.get("mog2") is not None else OracleEngine(**kw)


def test_dropin_passes_the_model_on_and_requests_no_planes(tmp_path):
    fr = R.flicker_clip(16)
    make = Factory()
    grp = motion.StreamGroup([str(tmp_path / "a")], batch=4, captures=[videoio.ArrayCapture(fr)], engine=make, box_size=96,
                             blur_scale=19, background_model="mog2", mog2_history=6, mog2_detect_shadows=False,
                             log_level=logging.DEBUG, cache_time=0.1, min_time=0.0, outdir=str(tmp_path), codec="MJPG")
    assert make.kwargs["mog2"] == {"history": 6, "var_threshold": 16.0, "detect_shadows": False, "learning_rate": -1.0}
    assert make.kwargs["keep_planes"] is False  # debug logging asks for no planes on this path
    vm = grp.videos[0]
    assert vm.background_model == "mog2" and vm.mog2 == make.kwargs["mog2"] and vm.keep_planes is False
    assert vm.ref_frame is None
    it = iter(motion.BatchFeeder(grp.engine, [vm.cap], 4))
    try:
        b = next(it)
        vfs = vm.make_frames(b, 0)
        vm.bind_results(vfs, grp.engine, 0)
        f = vfs[1]
        assert f.gray is None and f.blur is None and f.frame_delta is None
        assert f.thresh.shape == (80, 96) and f.contours is not None
        ref = vm.ref_frame  # the background image as float (h, w)
        assert ref.shape == (80, 96) and ref.dtype == np.float64 and ref[0, 0] == 30.0
    finally:
        it.close()
    # without the option nothing about the engine's construction changes
    plain = Factory()
    motion.StreamGroup([str(tmp_path / "b")], batch=4, captures=[videoio.ArrayCapture(fr)], engine=plain, box_size=96,
                       outdir=str(tmp_path))
    assert "mog2" not in plain.kwargs
    with pytest.raises(ValueError):
        motion.StreamGroup([str(tmp_path / "c")], batch=4, captures=[videoio.ArrayCapture(fr)], engine=Factory(), box_size=96,
                           background_model="knn", outdir=str(tmp_path))


def test_cli_and_ini_carry_the_model(tmp_path):
    from argparse import ArgumentParser

    parser = ArgumentParser()
    cli.get_args(parser)
    args = parser.parse_args(["x.avi"])
    assert args.background_model == "average" and "background_model" not in cli._job_kwargs(args)
    args = parser.parse_args(["x.avi", "--background-model", "mog2", "--mog2-history", "60", "--mog2-var-threshold", "25",
                              "--mog2-no-shadows", "--mog2-learning-rate", "0.01"])
    kw = cli._job_kwargs(args)
    assert (kw["background_model"], kw["mog2_history"], kw["mog2_var_threshold"], kw["mog2_detect_shadows"],
            kw["mog2_learning_rate"]) == ("mog2", 60, 25.0, False, 0.01)
    ini = tmp_path / "c.ini"
    ini.write_text("[settings]\nbackground_model = mog2\nmog2_history = 60\nmog2_var_threshold = 25\n"
                   "mog2_no_shadows = True\nmog2_learning_rate = 0.01\n")
    args = cli.process_config(str(ini), parser.parse_args(["x.avi"]))
    assert cli._job_kwargs(args) == {**cli._job_kwargs(parser.parse_args(["x.avi"])), **{
        k: kw[k] for k in ("background_model", "mog2_history", "mog2_var_threshold", "mog2_detect_shadows", "mog2_learning_rate")}}
    for bad in ("background_model = knn", "mog2_no_shadows = yes", "mog2_history = many"):
        ini.write_text("[settings]\n" + bad + "\n")
        with pytest.raises(ValueError):
            cli.process_config(str(ini), parser.parse_args(["x.avi"]))


def test_cv2_agrees_with_the_restatement():
    """Optional: against OpenCV's own subtractor on seeded content, where cv2 is installed."""
    cv2 = pytest.importorskip("cv2")
    lv = seeded_levels(n=40, h=24, w=31, seed=9)
    for shadows in (True, False):
        sub = cv2.createBackgroundSubtractorMOG2(history=6, varThreshold=16, detectShadows=shadows)
        st = R.Mog2Stream(24, 31, 31, 1, R.params(history=6, detect_shadows=int(shadows)))
        for t in range(lv.shape[0]):
            want = sub.apply(np.ascontiguousarray(lv[t]))
            got, _ = st.apply(lv[t])
            assert np.array_equal(got, want), f"frame {t}"
            assert np.array_equal(st.background_image(), sub.getBackgroundImage()), f"background {t}"


def test_scan_kernel_uses_no_scratch():
    """An array indexed by a lane's value goes to scratch memory; the scan's modes must stay in registers.  The
    compiler's own resource usage remarks for gfx950 (`make resources`: device code only, nothing is written)."""
    import os
    import re
    import subprocess

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "find_motion_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "resources", "SRC=fm_mog2.hip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stdout + r.stderr)[1:]
    scan = [b for b in blocks if "k_mog2_scan" in b.split()[0]]
    assert len(scan) == 1
    nums = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", scan[0])}
    assert nums["ScratchSize"] == 0 and nums["VGPRs Spill"] == 0 and nums["SGPRs Spill"] == 0, nums
    assert nums["VGPRs"] <= 128 and nums["Occupancy"] >= 4, nums  # 104 VGPRs, 4 waves per SIMD
