"""GPU: Gaussian sizes above 49 on the batched tile path (fm_wide.hip: k_wide_blur + k_small_scan).

A context with ksize > 49, more than 16 tiles and no kept planes runs its per-pixel chain as a frame-parallel
strip blur and the small-image scan, with the contour pass, the batch slots and the in-flight pipeline of the
other tile paths behind it.  Every comparison is bit for bit against oracle.OracleStream: masks, counts, boxes,
origins and the float64 background after every batch; every compared batch is required to show at least one
contour per stream in the oracle, so no comparison is of empty masks.

Shapes (W x H, k) and what each is for:
  328 x 136, 51   18 tiles, the smallest shape and the smallest k the path takes; the last tile column is 8 px
                  wide, the last tile row 8 rows tall; a first-frame launch of S frames is cut into two row bands
  400 x 136, 97   the reference's default blur at -B 1920
  329 x 137, 65   npx % 16 = 1: the unfused accumulate tail, an odd width
  1100 x 72, 255  r = 127 > h - 1: rows reflect repeatedly; 256-column strips, so five strips and their boundaries
  72 x 1100, 255  r > w - 1: columns reflect repeatedly; 1100 rows in bands
  600 x 136, 51   two 512-column strips: a strip boundary of the wider geometry
"""
import numpy as np
import pytest

import oracle
from find_motion_amd import MotionEngine, rasterize_masks
from find_motion_amd._native import FM_ESTATE, FMError, PLANE_BLUR, PLANE_DELTA, PLANE_GRAY
from find_motion_amd.synthetic import batch

pytestmark = pytest.mark.gpu

START, STEP = 40, 12  # frames START, START + STEP, ... of the synthetic streams (as test_gpu_engine_state.py)
WIDE_LAUNCHES = {"wide_blur", "wide_scan", "wide_blur_init", "wide_scan_init"}


def crafted_plane(blur, seed):
    """test_gpu_engine_state.crafted_plane's recipe: exact .5 ties, values just off them, negatives and values
    above 255 (convertScaleAbs's rounding and saturation) in the top third, the blur's own values below."""
    h, w = blur.shape
    rng = np.random.default_rng(seed)
    p = blur.astype(np.float64)
    rows = max(2, h // 3)
    base = np.floor(rng.random((rows, w)) * 300 - 20)
    frac = rng.choice([0.5, -0.5, 0.4999999999, 0.5000000001, 0.25, 0.0, 1.5, 2.5], size=(rows, w))
    p[:rows] = base + frac
    p[0, :8] = [-0.5, -1.5, 255.5, 256.5, 254.5, 0.5, 1e9, -1e9]
    return p


def painted(W, H, S, start, n):
    """Frames of a flat field with one 40 x 200 block (clipped to the frame) per stream that moves between
    frames: what the seeded streams do not give at 72 x 1100 under a 255-tap blur."""
    out = np.full((n, S, H, W, 3), 30, np.uint8)
    for t in range(n):
        for s in range(S):
            i = start + t
            y = (37 * i + 101 * s) % max(1, H - 200) if H > 200 else 0
            x = (53 * i + 67 * s) % max(1, W - 40)
            out[t, s, y:y + 200, x:x + 40] = 230
    return out


class Pair:
    """An engine and one OracleStream per stream, driven together."""

    def __init__(self, W, H, box, k, S, T, thresh=12, alpha=0.1, source=batch, **kw):
        self.W, self.H, self.box, self.k, self.S, self.T = W, H, box, k, S, T
        self.eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=box, ksize=k, threshold=thresh, avg=alpha,
                                max_batch=T, **kw)
        self.cfg = oracle.OracleConfig(H=H, W=W, box=box, ksize=k, thresh=thresh, alpha=alpha)
        assert (self.cfg.h, self.cfg.w) == self.eng.work_shape
        self.orc = [oracle.OracleStream(self.cfg) for _ in range(S)]
        self.pos = START
        self.source = source
        self.nb = 0

    def frames(self, n=None):
        n = self.T if n is None else n
        fr = np.concatenate([self.source(self.W, self.H, self.S, self.pos + STEP * t, 1) for t in range(n)])
        self.pos += STEP * n
        return fr

    def compare(self, fr, background=True):
        """wait() for the batch of frames fr and compare every frame of every stream with the oracle."""
        eng = self.eng
        tag = f"batch {self.nb}"
        self.nb += 1
        eng.wait()
        counts = eng.counts()
        refs, seen, steady = [], [0] * self.S, [0] * self.S
        for t in range(fr.shape[0]):
            row = []
            for s in range(self.S):
                first = not self.orc[s].initialized
                ref = self.orc[s].step(fr[t, s])
                row.append(ref)
                at = f"{tag}: frame {t} stream {s}"
                np.testing.assert_array_equal(eng.mask(t, s), ref["mask"], err_msg="mask " + at)
                assert counts[t, s] == ref["count"], at
                got = eng.contours(t, s)
                assert [c.bbox for c in got] == ref["boxes"], at
                assert [c.origin for c in got] == ref["origins"], at
                if not first:
                    steady[s] += 1
                    seen[s] += ref["count"]
            refs.append(row)
        for s in range(self.S):
            assert seen[s] > 0 or steady[s] == 0, f"{tag}: the oracle finds no contour on stream {s}"
        if background:
            self.compare_background(tag)
        return refs

    def compare_background(self, tag=""):
        for s in range(self.S):
            bg = self.eng.background(s)
            assert np.array_equal(bg, self.orc[s].bg), \
                f"{tag}: background stream {s}: {int((bg != self.orc[s].bg).sum())} values differ"

    def step(self, n=None):
        fr = self.frames(n)
        self.eng.submit(fr)
        return fr, self.compare(fr)


SHAPES = [
    # W, H, k, streams, frames per batch, batches, engine / source options
    pytest.param(328, 136, 51, 2, 3, 3, {}, id="328x136-k51"),
    pytest.param(400, 136, 97, 2, 3, 3, {}, id="400x136-k97"),
    pytest.param(329, 137, 65, 2, 3, 3, {}, id="329x137-k65"),
    # (the oracle takes a third of a second per frame under 255 taps: one stream, two batches of two frames)
    pytest.param(1100, 72, 255, 1, 2, 2, {}, id="1100x72-k255"),
    pytest.param(72, 1100, 255, 1, 2, 2, dict(source=painted, thresh=2, alpha=0.5), id="72x1100-k255"),
    pytest.param(600, 136, 51, 2, 3, 2, {}, id="600x136-k51"),
]


@pytest.mark.parametrize("W,H,k,S,T,NB,kw", SHAPES)
def test_parity(W, H, k, S, T, NB, kw):
    """Batches of several frames at each shape: a first-frame launch, then steady ones."""
    p = Pair(W, H, W, k, S, T, **kw)
    try:
        assert (W, H) != (329, 137) or p.cfg.h * p.cfg.w % 16 == 1  # the unfused accumulate tail has a pixel
        for _ in range(NB):
            p.step()
    finally:
        p.eng.close()


@pytest.mark.parametrize("W,H", [(656, 272), (500, 208)], ids=["integer-scale", "general-scale"])
def test_resize_in_front(W, H):
    """INTER_AREA to box 328 in front of the wide blur: the 2 x 2 integer-scale kernel and the general one."""
    p = Pair(W, H, 328, 51, 2, 3)
    try:
        assert p.eng.work_shape == (136, 328)
        for _ in range(2):
            p.step()
    finally:
        p.eng.close()


def test_streams_masks_resets_and_written_background():
    """S = 3 with a rectangle mask on one stream and a triangle on another; a stream reset between batches, so
    one batch holds a first frame and steady frames; a background written with .5 ties, values above 255 and
    negatives."""
    p = Pair(328, 136, 328, 51, 3, 3)
    eng = p.eng
    try:
        h, w = eng.work_shape
        A = rasterize_masks(h, w, 1.0, [((0, 0), (p.W // 3, p.H // 2))])
        B = rasterize_masks(h, w, 1.0, [((p.W - 1, p.H - 1), (p.W // 2, p.H - 1), (p.W - 1, p.H // 3))])
        assert A.min() == 0 and B.min() == 0 and A.max() == 1 and not np.array_equal(A, B)
        for s, m in ((0, A), (2, B)):
            eng.set_mask(s, m)
            p.orc[s].keep = np.ascontiguousarray(m, dtype=np.uint8)
        p.step()
        p.step()
        eng.reset(1)
        p.orc[1].reset()
        assert [eng.initialized(s) for s in range(3)] == [True, False, True]
        _, refs = p.step()
        assert all(refs[t][0]["blur"][A == 0].max() == 0 for t in range(3))  # masked pixels blur to 0
        fr = batch(p.W, p.H, 3, p.pos, 1)[0, 0]
        P = crafted_plane(oracle.gauss_blur(oracle.bgr2gray(fr), p.k), 3)
        eng.set_background(0, P)
        p.orc[0].set_background(P)
        assert np.array_equal(eng.background(0), P)
        p.step()
        p.step(1)  # a batch of one frame
    finally:
        eng.close()


def test_in_flight_slots_and_their_reuse():
    """eng.max_inflight batches submitted before the first wait, a further submit refused, then a second round
    that reuses every slot and ends with a batch shorter than max_batch."""
    p = Pair(328, 136, 328, 51, 1, 2)
    eng = p.eng
    try:
        depth = eng.max_inflight
        assert depth >= 2
        for rnd in range(2):
            frs = [p.frames(1 if (rnd == 1 and i == depth - 1) else None) for i in range(depth)]
            for fr in frs:
                eng.submit(fr)
            with pytest.raises(FMError) as e:
                eng.submit(frs[0])
            assert e.value.code == FM_ESTATE
            for fr in frs:
                p.compare(fr, background=False)
            p.compare_background(f"round {rnd}")
    finally:
        eng.close()


def _reference_contours(mask):
    first = oracle.find_contours_ext(mask, cap=1 << 14)
    pts_cap = max([c["npts"] for c in first], default=0) + 1
    ref = oracle.find_contours_ext(mask, cap=len(first) + 1, with_points=True, pts_cap=pts_cap)
    assert len(ref) == len(first)
    return ref


def test_contour_points():
    """FM_FLAG_CONTOUR_POINTS behind the wide blur: every contour's points and area equal the oracle's."""
    p = Pair(328, 136, 328, 51, 1, 3, contour_points=True)
    try:
        for _ in range(2):
            fr, refs = p.step()
        n = 0
        for t in range(3):
            ref = _reference_contours(refs[t][0]["mask"])
            got = p.eng.contours(t, 0)
            assert len(got) == len(ref)
            for g, r in zip(got, ref):
                assert g.bbox == r["bbox"] and g.origin == r["origin"]
                np.testing.assert_array_equal(g.points[:, 0, :], r["points"])
                assert g.area == r["area"]
                n += 1
        assert n > 0
    finally:
        p.eng.close()


def test_contour_area():
    """FM_FLAG_CONTOUR_AREA behind the wide blur: every contour's area equals the oracle's."""
    p = Pair(328, 136, 328, 51, 1, 3, contour_area=True)
    try:
        for _ in range(2):
            fr, refs = p.step()
        n = 0
        for t in range(3):
            got = [c.area for c in p.eng.contours(t, 0)]
            assert got == [float(a) for a in refs[t][0]["areas"]]
            n += len(got)
        assert n > 0
    finally:
        p.eng.close()


def test_selection_by_launch_names():
    """The engine's own launch timing names the wide kernels, neither the per-frame kernel nor k_fused; more
    than one batch may be in flight."""
    p = Pair(328, 136, 328, 51, 2, 3, profile="pix")
    eng = p.eng
    try:
        for _ in range(2):
            eng.submit(p.frames())
            eng.wait()
        names = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0}
        assert {"wide_blur", "wide_scan", "wide_scan_init"} <= names, names
        assert not names & {"pixel", "fused", "pix", "small_scan"}, names
        assert eng.max_inflight >= 2
        assert eng.pixel_path == "wide"
    finally:
        eng.close()


def test_kept_planes_stay_on_the_per_frame_path():
    """keep_planes=True at the same shape: the per-frame path, one batch in flight, equal to the oracle with its
    gray, blur and delta planes."""
    p = Pair(328, 136, 328, 51, 2, 3, keep_planes=True, profile=True)
    eng = p.eng
    try:
        assert eng.pixel_path == "pixel" and eng.max_inflight == 1
        for _ in range(2):
            fr, refs = p.step()
            for t in range(3):
                for s in range(2):
                    for which, key in ((PLANE_GRAY, "gray"), (PLANE_BLUR, "blur"), (PLANE_DELTA, "delta")):
                        np.testing.assert_array_equal(eng.plane(which, t, s), refs[t][s][key], err_msg=key)
        names = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0}
        assert "pixel" in names and not names & WIDE_LAUNCHES, names
    finally:
        eng.close()
