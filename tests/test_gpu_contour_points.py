"""Contour points on the GPU (FM_FLAG_CONTOUR_POINTS, MotionEngine(contour_points=True)): every external
contour's CHAIN_APPROX_SIMPLE points against the oracle's (oracle.find_contours_ext(with_points=True): the
literal icvFetchContour restatement), exactly -- the same contours, the same npts, the same points in the
same order -- on the register, LDS and unstaged paths of fm_trace.hip, both mask representations, batches in
flight with regrown buffers, frames past max_contours, and through VideoMotion.

Masks are painted through the engine as tests/test_gpu_configs.py::_area_case does (frame 0 black, the
pattern in a later frame, ksize 1, threshold 0, avg 0): the mask is the pattern dilated 5 x 5, so gaps
are painted at least 7 px wide.  Because every mask is dilated, the smallest contour an engine can
return is the 5 x 5 square of an isolated dot (3 x 3 in a corner), 4 points: the 1-point contour of a
single mask pixel (the walker's isolated-pixel exit) cannot be reached through fm_submit; the isolated
dot is checked for what the oracle says about its dilated mask.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from find_motion_amd import MotionEngine, _native
from find_motion_amd.synthetic import batch

pytestmark = pytest.mark.gpu

PAINT = dict(ksize=1, threshold=0, avg=0.0)


def reference(mask):
    """The oracle's contours of mask, with every point (pts_cap raised above the largest npts)."""
    first = oracle.find_contours_ext(mask, cap=1 << 14)
    pts_cap = max([c["npts"] for c in first], default=0) + 1
    ref = oracle.find_contours_ext(mask, cap=len(first) + 1, with_points=True, pts_cap=pts_cap)
    assert len(ref) == len(first)
    assert all(c["npts"] < pts_cap and len(c["points"]) == c["npts"] for c in ref)
    return ref


def shoelace(p):
    x, y = p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)
    return abs(int(np.sum(x * np.roll(y, -1) - y * np.roll(x, -1)))) / 2


def check_frame(eng, t, s, mask=None, tag=""):
    """Frame (t, s) of the last waited batch against the oracle on `mask` (default: the engine's own
    mask, which the parity tests pin to the oracle's).  Returns the oracle's contours."""
    m = eng.mask(t, s)
    if mask is not None:
        np.testing.assert_array_equal(m, mask, err_msg=f"mask {tag}")
    ref = reference(m)
    got = eng.contours(t, s)
    assert len(got) == len(ref) == eng.counts()[t, s], tag
    for i, (g, r) in enumerate(zip(got, ref)):
        where = f"{tag} contour {i} at {r['origin']}"
        assert g.bbox == r["bbox"] and g.origin == r["origin"], where
        assert g.points is not None and g.points.dtype == np.int32, where
        assert g.points.shape == (r["npts"], 1, 2), where
        np.testing.assert_array_equal(g.points[:, 0, :], r["points"], err_msg=where)
        assert tuple(g.points[0, 0]) == g.origin, where
        p = g.points[:, 0, :]
        assert (p[:, 0].min(), p[:, 1].min(), np.ptp(p[:, 0]) + 1, np.ptp(p[:, 1]) + 1) == g.bbox, where
        assert g.area == r["area"] == shoelace(p), where
    return ref


def paint(patterns, **kw):
    """An engine that has waited for [black, *patterns] (one stream); frame t + 1 holds patterns[t] dilated."""
    h, w = patterns[0].shape
    fr = np.zeros((len(patterns) + 1, 1, h, w, 3), np.uint8)
    for t, p in enumerate(patterns):
        fr[t + 1, 0] = p[..., None]
    eng = MotionEngine(n_streams=1, src_w=w, src_h=h, box_size=w, max_batch=fr.shape[0], contour_points=True,
                       **{**PAINT, **kw})
    eng.submit(fr)
    eng.wait()
    return eng


def painted_case(pattern, **kw):
    eng = paint([pattern], **kw)
    ref = check_frame(eng, 1, 0, mask=oracle.dilate5(pattern))
    stats = eng.trace_stats()
    eng.close()
    return ref, stats


# ---- patterns ---------------------------------------------------------------------------------
def dots(h, w, n, seed, margin=4, pitch=12):
    """n isolated dots on a pitch grid (their 5 x 5 dilations never touch)."""
    rng = np.random.default_rng(seed)
    cells = [(y, x) for y in range(margin, h - margin, pitch) for x in range(margin, w - margin, pitch)]
    m = np.zeros((h, w), np.uint8)
    for k in rng.choice(len(cells), n, replace=False):
        m[cells[k]] = 255
    return m


def staircase(steps=12, run=8):
    m = np.zeros((steps * run + 20, steps * run + 20), np.uint8)
    for i in range(steps):
        m[10 + run * i:10 + run * (i + 1), 10:10 + run * (i + 1)] = 255
    return m


def comb(width=330, pitch=8):
    m = np.zeros((140, width), np.uint8)
    m[68:72, 8:width - 10] = 255
    for x in range(8, width - 10, pitch):
        m[20:120, x] = 255  # teeth on both sides of the spine
    return m


def spiral(size=210, pitch=6):
    """A 1-px line spiralling inwards at pitch 6: 5 px wide after dilation, a 1-px gap between the arms."""
    m = np.zeros((size, size), np.uint8)
    x, y, length, k = 5, 5, size - 11, 0
    while length > pitch:
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[k % 4]
        for i in range(length + 1):
            m[y + dy * i, x + dx * i] = 255
        x, y, k = x + dx * length, y + dy * length, k + 1
        if k >= 3 and k % 2 == 1:
            length -= pitch
    return m


def ring_and_blob(h, w):
    """A thin ring around most of the image and, outside it, a small two-box blob."""
    m = np.zeros((h, w), np.uint8)
    m[3:h - 3, 40:w - 3] = 255
    m[5:h - 5, 42:w - 5] = 0
    m[100:120, 5:25] = 255
    m[90:100, 10:20] = 255
    return m


def dot_and_corner_dots():
    """An isolated dot and a dot in each corner of a 100 x 100 image (dilated: 5 x 5, and 3 x 3 against the
    corners, where the register path's window starts left of and above the image)."""
    m = np.zeros((100, 100), np.uint8)
    m[50, 40] = m[0, 0] = m[99, 99] = m[0, 99] = m[99, 0] = 255
    return m


def edge_blob():
    """A 200 x 130 blob (not a multiple of 64; outside the image is zero) that touches all four edges, with a
    notch cut into each."""
    m = np.full((130, 200), 255, np.uint8)
    m[0:30, 50:59] = 0
    m[60:69, 170:200] = 0
    m[100:130, 20:29] = 0
    m[40:49, 0:25] = 0
    return m


def box_words(bbox):
    """32-bit words of a contour box's staged window, as trace_box_path counts them: the padded box's words per
    row, plus one, times its rows."""
    return (((bbox[2] + 2 + 31) >> 5) + 1) * (bbox[3] + 2)


# ---- fixtures and random masks -----------------------------------------------------------------
def test_fixture_masks_and_random_speckle():
    from golden_cases import contour_cases

    total = 0
    for name, case in sorted(contour_cases().items()):
        eng = paint([case["mask"]])
        total += len(check_frame(eng, 1, 0, mask=oracle.dilate5(case["mask"]), tag=name))
        eng.close()
    # (dilated, each small fixture is one blob: at least one contour per non-empty mask)
    assert total >= sum(bool(c["mask"].any()) for c in contour_cases().values()) >= 9
    rng = np.random.default_rng(11)
    pats = [((rng.random((150, 230)) < 0.003 * t) * 255).astype(np.uint8) for t in range(1, 4)]  # 3 x 4 tiles
    eng = paint(pats)
    for t, p in enumerate(pats):
        ref = check_frame(eng, t + 1, 0, mask=oracle.dilate5(p), tag=f"speckle {t}")
        assert len(ref) > 10
        if t == 2:  # contours that cross tile edges, and some with many points
            assert any(c["bbox"][0] // 64 != (c["bbox"][0] + c["bbox"][2] - 1) // 64 for c in ref)
            assert max(c["npts"] for c in ref) >= 12
    eng.close()


# ---- shapes the walk can get wrong -------------------------------------------------------------
def test_isolated_dot_and_corner_dots():
    ref, stats = painted_case(dot_and_corner_dots())
    assert len(ref) == 5
    assert sorted(c["bbox"][2:] for c in ref) == [(3, 3)] * 4 + [(5, 5)] and all(c["npts"] == 4 for c in ref)
    assert stats["staged"] == 5 and stats["unstaged"] == 0 and stats["steps"] > 0


def test_blob_touching_all_four_edges():
    ref, _ = painted_case(edge_blob())
    assert len(ref) == 1 and ref[0]["bbox"] == (0, 0, 200, 130) and ref[0]["npts"] >= 20


def test_staircase_has_a_point_at_every_step():
    ref, _ = painted_case(staircase(12, 8))
    assert len(ref) == 1 and ref[0]["npts"] >= 2 * 12


def test_comb_overflows_the_point_buffer_many_times():
    ref, stats = painted_case(comb())
    assert len(ref) == 1 and ref[0]["npts"] >= 400 and ref[0]["npts"] % 64 != 0
    assert stats == {"staged": 1, "unstaged": 0, "steps": stats["steps"]} and stats["steps"] > ref[0]["npts"]


def test_spiral_long_walk_across_tiles():
    ref, stats = painted_case(spiral())
    big = max(ref, key=lambda c: c["npts"])
    assert big["bbox"][2] >= 190 and big["bbox"][3] >= 190
    assert stats["steps"] >= 4000 and stats["staged"] >= 1 and stats["unstaged"] == 0


# ---- both paths ---------------------------------------------------------------------------------
def test_staged_and_unstaged_contours_in_one_frame():
    """The ring grows with the image until its window no longer fits the big LDS window; every size visited is
    compared with the oracle.  At 640 x 360 the ring's box needs more than kWinWords (2,048) words and at most
    kBigWords (16,256): staged by k_trace_lds<EMIT, 1, kBigWords>, the 63.5 KiB window."""
    for w, h in ((640, 360), (1280, 720), (1920, 1080)):
        eng = paint([ring_and_blob(h, w)], profile=True)
        stats = eng.trace_stats()
        ran = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0 and n.startswith("trace_")}
        ref = check_frame(eng, 1, 0, mask=oracle.dilate5(ring_and_blob(h, w)), tag=f"{w} x {h}")
        eng.close()
        assert len(ref) == 2 and ref[0]["bbox"][2] >= w - 50 and ref[1]["bbox"][2] <= 40, (w, h)
        if (w, h) == (640, 360):
            assert stats["staged"] == 2 and stats["unstaged"] == 0, stats
            assert 2048 < box_words(ref[0]["bbox"]) <= 16256 and box_words(ref[1]["bbox"]) <= 2048, ref
            assert ran == {"trace_count_lds", "trace_emit_lds", "trace_count_lds_big", "trace_emit_lds_big"}, ran
        if stats["unstaged"] >= 1:
            break
    else:
        pytest.fail("the ring's contour is still staged at 1920 x 1080")
    assert len(ref) == 2 and stats["staged"] >= 1 and stats["unstaged"] >= 1
    assert ref[0]["bbox"][2] >= w - 50 and ref[1]["bbox"][2] <= 40
    assert box_words(ref[0]["bbox"]) > 16256 and "trace_emit_unstaged" in ran, (ref[0]["bbox"], ran)


# ---- both mask representations ------------------------------------------------------------------
@pytest.mark.parametrize("W,H,box,k", [(640, 360, 640, 5), (128, 96, 128, 51), (192, 108, 100, 5)],
                         ids=["fused_k5", "bytes_k51", "small_image"])
def test_mask_representations(W, H, box, k):
    T = 8
    fr = batch(W, H, 1, 20, T)
    if k == 51:  # the wide blur needs large bright shapes to cross the threshold
        fr[:] = 0
        fr[2:, 0, 20:60, 30:90] = 255
        fr[4:, 0, 70:90, 10:40] = 200
    eng = MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=box, ksize=k, threshold=12, avg=0.1, max_batch=T,
                       contour_points=True)
    eng.submit(fr)
    eng.wait()
    n = sum(len(check_frame(eng, t, 0, tag=f"frame {t}")) for t in range(T))
    eng.close()
    assert n >= 3


# ---- batching -----------------------------------------------------------------------------------
def test_batches_in_flight_and_buffer_regrowth():
    S, T, h, w = 2, 3, 96, 160
    rng = np.random.default_rng(5)

    def frames(make):
        fr = np.zeros((T, S, h, w, 3), np.uint8)
        for t in range(T):
            for s in range(S):
                fr[t, s] = make(t, s)[..., None]
        return fr

    small = frames(lambda t, s: dots(h, w, 2, 10 * t + s) if t else np.zeros((h, w), np.uint8))
    dense = frames(lambda t, s: ((rng.random((h, w)) < 0.012) * 255).astype(np.uint8))
    small2 = frames(lambda t, s: dots(h, w, 3, 100 + 10 * t + s))
    eng = MotionEngine(n_streams=S, src_w=w, src_h=h, box_size=w, max_batch=T, contour_points=True, **PAINT)
    assert eng.max_inflight >= 2
    eng.submit(small)
    eng.submit(dense)
    npoints = []
    for bi, fr in enumerate((small, dense, small2)):
        if bi == 2:
            eng.submit(small2)
        eng.wait()
        n = 0
        for t in range(T):
            for s in range(S):
                ref = check_frame(eng, t, s, mask=oracle.dilate5(fr[t, s, :, :, 0]), tag=f"batch {bi} t {t} s {s}")
                n += sum(c["npts"] for c in ref)
        npoints.append(n)
    eng.close()
    assert npoints[0] > 0 and npoints[1] >= 10 * npoints[0] and 0 < npoints[2] < npoints[1]


def test_more_contours_than_max_contours():
    m = dots(120, 160, 40, 3)
    ref, stats = painted_case(m, max_contours=8)
    assert len(ref) == 40 and stats["staged"] == 40


# ---- refusals and unchanged results -------------------------------------------------------------
def _raw_records(eng, t, s):
    buf = (_native.FMContour * 4096)()
    n = eng._L.fm_get_contours(eng._h, t, s, C.cast(buf, C.c_void_p), 4096)
    assert 0 <= n <= 4096
    return buf[:n]


def test_refusals_and_flag_off_results_unchanged():
    W, H, T = 640, 360, 12
    fr = batch(W, H, 1, 24, T)
    kw = dict(n_streams=1, src_w=W, src_h=H, box_size=W, ksize=5, threshold=12, avg=0.1, max_batch=T)
    off, on, area = MotionEngine(**kw), MotionEngine(contour_points=True, **kw), MotionEngine(contour_area=True, **kw)
    total = C.c_size_t(99)
    xy = np.zeros((4, 2), np.int32)
    # before the first wait, and without the flag
    assert on._L.fm_get_contour_points(on._h, 0, 0, xy.ctypes.data, 4, C.byref(total)) == _native.FM_ESTATE
    for e in (off, on, area):
        e.submit(fr)
        e.wait()
    assert off._L.fm_get_contour_points(off._h, 1, 0, xy.ctypes.data, 4, C.byref(total)) == _native.FM_ESTATE
    assert total.value == 0
    np.testing.assert_array_equal(off.counts(), on.counts())
    seen = 0
    for t in range(T):
        a, b, c = off.contours(t, 0), on.contours(t, 0), area.contours(t, 0)
        assert [x.bbox for x in a] == [x.bbox for x in b] and [x.origin for x in a] == [x.origin for x in b], t
        assert all(x.points is None and x.area is None for x in a)
        assert all(r.npts == 0 and r.area2 == -1 for r in _raw_records(off, t, 0))
        assert [r.npts for r in _raw_records(on, t, 0)] == [len(x.points) for x in b]
        assert [x.area for x in b] == [x.area for x in c], t
        np.testing.assert_array_equal(off.mask(t, 0), on.mask(t, 0))
        n = sum(len(x.points) for x in b)
        seen += n
        if n > 4:  # a cap too small: FM_EINVAL, *total set, nothing written
            xy[:] = -1
            assert on._L.fm_get_contour_points(on._h, t, 0, xy.ctypes.data, 4, C.byref(total)) == _native.FM_EINVAL
            assert total.value == n and (xy == -1).all()
            assert len(on.contour_points_xy(t, 0)) == n
    assert seen > 4
    with pytest.raises(_native.FMError):
        on.contour_points_xy(T, 0)
    for e in (off, on, area):
        e.close()


# ---- drop-in ------------------------------------------------------------------------------------
def test_video_motion_contours_are_cv2_arrays(tmp_path):
    from find_motion_amd import motion, videoio

    W, H, n = 192, 108, 60

    class Recording(motion.VideoMotion):
        def step(self):
            self.seen.append((self.current_frame.index, list(self.current_frame.contours)))
            super().step()

    runs = {}
    for flag in (True, False):
        vm = Recording(filename=str(tmp_path / f"v{int(flag)}"), capture=videoio.SyntheticCapture(W, H, n, 0),
                       box_size=100, threshold=12, cache_time=0.3, min_time=0.1, batch=8, outdir=str(tmp_path),
                       contour_points=flag)
        vm.seen = []
        vm.find_motion()
        runs[flag] = vm
    assert runs[True].written_indices == runs[False].written_indices and runs[True].written_indices
    assert all(c.points is None for _, cs in runs[False].seen for c in cs)
    vid = videoio.SyntheticCapture(W, H, n, 0).video
    frames = np.stack([vid.frame(i) for i in range(n)])
    st = oracle.OracleStream(oracle.OracleConfig(H=H, W=W, box=100, ksize=runs[True].gaussian[0], thresh=12, alpha=0.1))
    res = st.run(frames, mask_frames=range(n))
    assert [i for i, _ in runs[True].seen] == list(range(n))
    total = 0
    for i, cs in runs[True].seen:
        ref = reference(res.masks[i])
        assert len(cs) == len(ref), i
        for c, r in zip(cs, ref):
            a = np.asarray(c)
            assert a.shape == (r["npts"], 1, 2) and a.dtype == np.int32
            np.testing.assert_array_equal(a[:, 0, :], r["points"], err_msg=f"frame {i}")
            total += 1
    assert total >= 10
