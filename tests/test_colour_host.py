"""CPU: the colour-motion reference's own properties (tests/colour_ref.py, composed from the oracle's stages),
asserted from the reference alone, and the drop-in's plumbing of colour_motion.

These are the conditions under which the GPU tests of tests/test_gpu_colour.py mean something: the isoluminant
mover is invisible to the gray chain and visible to the colour chain; on gray content the two chains agree; the
SIMD rules count the 3hw interleaved elements (a per-plane count quantises a .5 tie differently); and on the GPU
test's 66 x 70 content the scalar tail of accumulateWeighted really differs from the fma body in a tail element.
"""
import logging

import numpy as np
import pytest

import colour_ref
import oracle
from colour_ref import ColourStream
from fake_engine import OracleEngine
from find_motion_amd import cli, motion, videoio
from oracle import oracle as oo


def test_isoluminant_colours_share_a_gray_level():
    px = np.array([[colour_ref.ISO_BG, colour_ref.ISO_MOVER]], np.uint8)
    assert oo.bgr2gray(px).tolist() == [[30, 30]]


def test_isoluminant_mover_gray_blind_colour_sees():
    fr = colour_ref.iso_clip()  # 96 x 80, 12 x 12 block, 3 px a frame, 6 frames
    assert fr.shape == (6, 80, 96, 3)
    assert colour_ref.gray_counts(fr, box=96, ksize=5, thresh=12) == [0] * 6
    st = ColourStream(80, 96, 96, 5, thresh=12)
    counts = [st.step(f)["count"] for f in fr]
    assert counts[0] == 0 and all(c >= 1 for c in counts[1:]), counts


def test_gray_frames_equal_the_gray_oracle():
    W, H, n = 64, 48, 8  # h * w a multiple of 16: the gray chain has no scalar tail either
    g = oracle_gray_frames(W, H, n)
    fr = np.repeat(g[..., None], 3, axis=3)  # B = G = R
    # BGR2GRAY of (v, v, v) is v: (1868 + 9617 + 4899) v + 8192 >> 14 = (16384 v + 8192) >> 14
    assert np.array_equal(oo.bgr2gray(fr[0]), g[0])
    cfg = oracle.OracleConfig(H=H, W=W, box=W, ksize=5, thresh=12, alpha=0.1)
    gs, cs = oracle.OracleStream(cfg), ColourStream(H, W, W, 5)
    moved = 0
    for f in fr:
        a, b = gs.step(f), cs.step(f)
        assert np.array_equal(a["mask"], b["mask"]) and a["count"] == b["count"] and a["boxes"] == b["boxes"]
        moved += a["count"]
        for c in range(3):
            assert np.array_equal(cs.bg[..., c], gs.bg)  # bit for bit
    assert moved > 0


def oracle_gray_frames(W, H, n):
    rng = np.random.default_rng(5)
    g = np.full((n, H, W), 60, np.uint8)
    for t in range(n):
        x = 4 + 5 * t
        g[t, 10:24, x:x + 12] = 200
        g[t] += rng.integers(0, 3, size=(H, W), dtype=np.uint8)
    return g


def test_simd_rule_counts_interleaved_elements():
    """3 x 2 work image: hw = 6 < 16 <= 18 = 3hw.  convertScaleAbs on the 3-channel Mat takes the float path
    (n = 18): 101.49999999999999 rounds to 101.5f and then to even, 102; a per-plane count (n = 6) would round the
    double itself, 101."""
    tie = np.nextafter(101.5, 0.0)
    assert float(np.float32(tie)) == 101.5 and round(tie) == 101
    bg = np.full((2, 3, 3), tie)
    frame = np.full((2, 3, 3), 110, np.uint8)
    a = ColourStream(2, 3, 3, 1, thresh=8)
    b = ColourStream(2, 3, 3, 1, thresh=8, per_plane_n=True)
    a.set_background(bg)
    b.set_background(bg)
    ra, rb = a.step(frame), b.step(frame)
    assert (ra["delta"] == 8).all() and (rb["delta"] == 9).all()   # |110 - 102|, |110 - 101|
    assert ra["count"] == 0 and rb["count"] == 1                   # 8 > 8 is false, 9 > 8 true
    d, _ = oo.diff_thresh(frame, bg, 8)                            # the interleaved call itself
    assert np.array_equal(ra["delta"], d)


def test_tail_elements_differ_from_the_fma_body():
    """66 x 70: 3hw = 13860, 13860 % 16 = 4: the scalar tail is the last pixel's B, G, R and channel R of the
    pixel before it.  On the GPU test's content (stream 0, no keep-mask), at every frame count at which that test
    can end (73 frames and 3 more for each further batch in flight), an all-fma accumulate differs from the
    reference in a tail element of the background."""
    W, H = colour_ref.TAIL_W, colour_ref.TAIL_H
    n3 = 3 * W * H
    assert n3 % 16 == 4
    fr = colour_ref.tail_clip()[:, 0]
    ends = set(np.cumsum(colour_ref.TAIL_SIZES)[2:].tolist())
    a, b = ColourStream(H, W, W, 5), ColourStream(H, W, W, 5, all_fma=True)
    for i, f in enumerate(fr):
        a.step(f)
        b.step(f)
        if i + 1 in ends:
            fa, fb = a.bg.reshape(-1), b.bg.reshape(-1)
            assert np.array_equal(fa[:n3 - 4], fb[:n3 - 4])  # the body is the same arithmetic
            assert (fa[n3 - 4:] != fb[n3 - 4:]).any(), f"reseed: after {i + 1} frames the tail equals the fma"
    assert len(ends) == 8


class ColourFactory:
    """An engine factory with MotionEngine's signature that records what it was asked for and serves the colour
    reference's results behind OracleEngine's interface."""

    def __init__(self):
        self.kwargs = None

    def __call__(self, **kw):
        self.kwargs = dict(kw)
        return ColourEngine(**kw)


class ColourEngine(OracleEngine):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.colour_motion = bool(kw.get("colour_motion"))
        c = self.cfg
        self.cstreams = [ColourStream(c.H, c.W, c.box, c.ksize, c.thresh, c.alpha) for _ in range(self.n_streams)]

    def initialized(self, s):
        return self.cstreams[s].initialized

    def background(self, s):
        return self.cstreams[s].bg.copy()

    def submit(self, frames):
        frames = np.asarray(frames)
        frames = frames[None] if frames.ndim == 4 else frames
        out = []
        for t in range(frames.shape[0]):
            row = []
            for s, st in enumerate(self.cstreams):
                r = st.step(frames[t, s])
                r["areas"] = [c["area"] for c in r["contours"]]
                row.append(r)
            out.append(row)
        self._queue.append(out)
        self.submits += 1

    def plane(self, which, t, s):
        raise AssertionError("planes requested on a colour engine")


def test_dropin_passes_colour_motion_and_requests_no_planes(tmp_path):
    fr = colour_ref.iso_clip(n=12)
    make = ColourFactory()
    grp = motion.StreamGroup([str(tmp_path / "a")], batch=4, captures=[videoio.ArrayCapture(fr)], engine=make,
                             box_size=96, blur_scale=19, threshold=12, colour_motion=True, log_level=logging.DEBUG,
                             cache_time=0.1, min_time=0.0, outdir=str(tmp_path), codec="MJPG")
    assert make.kwargs["colour_motion"] is True and make.kwargs["keep_planes"] is False  # debug logging: no planes
    vm = grp.videos[0]
    assert vm.colour_motion and vm.keep_planes is False
    assert vm.ref_frame is None
    it = iter(motion.BatchFeeder(grp.engine, [vm.cap], 4))
    try:
        b = next(it)
        vfs = vm.make_frames(b, 0)
        vm.bind_results(vfs, grp.engine, 0)
        f = vfs[1]
        assert f.gray is None and f.blur is None and f.frame_delta is None
        assert f.thresh.shape == (80, 96) and len(f.contours) >= 1
        assert vm.ref_frame.shape == (80, 96, 3)
    finally:
        it.close()
    # without the option nothing about the engine's construction changes
    plain = ColourFactory()
    motion.StreamGroup([str(tmp_path / "b")], batch=4, captures=[videoio.ArrayCapture(fr)], engine=plain, box_size=96,
                       outdir=str(tmp_path))
    assert "colour_motion" not in plain.kwargs and plain.kwargs["keep_planes"] is False
    shown = ColourFactory()
    motion.StreamGroup([str(tmp_path / "c")], batch=4, captures=[videoio.ArrayCapture(fr)], engine=shown, box_size=96,
                       outdir=str(tmp_path), log_level=logging.DEBUG)
    assert shown.kwargs["keep_planes"] is True


def test_cli_and_ini_carry_colour_motion(tmp_path):
    from argparse import ArgumentParser

    parser = ArgumentParser()
    cli.get_args(parser)
    args = parser.parse_args(["x.avi"])
    assert args.colour_motion is False and cli._job_kwargs(args)["colour_motion"] is False
    args = parser.parse_args(["x.avi", "--colour-motion"])
    assert cli._job_kwargs(args)["colour_motion"] is True
    ini = tmp_path / "c.ini"
    ini.write_text("[settings]\ncolour_motion = True\n")
    args = cli.process_config(str(ini), parser.parse_args(["x.avi"]))
    assert cli._job_kwargs(args)["colour_motion"] is True
    ini.write_text("[settings]\ncolour_motion = yes\n")
    with pytest.raises(ValueError):
        cli.process_config(str(ini), parser.parse_args(["x.avi"]))


def test_plan_names_the_colour_path_and_refuses_what_it_cannot_take():
    from find_motion_amd import _native
    from find_motion_amd._native import FM_ENOTSUP, FMError

    base = dict(src_w=1920, src_h=1080, box_size=100, ksize=5)
    assert _native.plan(**base)["pixel_path"] == "small"
    p = _native.plan(colour_motion=True, **base)
    assert p["pixel_path"] == "rgb" and p["work_shape"] == (56, 100)
    assert _native.plan(colour_motion=True, src_w=1920, src_h=1080, box_size=1920, ksize=49)["pixel_path"] == "rgb"
    for bad in (dict(ksize=51), dict(keep_planes=True), dict(src_w=8192, src_h=8192, box_size=8192)):  # 16,384 tiles
        with pytest.raises(FMError) as e:
            _native.plan(colour_motion=True, **{**base, **bad})
        assert e.value.code == FM_ENOTSUP
    assert "fm_background_channels" in _native.EXPORTED
