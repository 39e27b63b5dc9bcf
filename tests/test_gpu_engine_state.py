"""GPU: an engine whose state changes between batches, and input ordered on a caller's stream.

The parity suite (test_gpu_parity.py) follows one history: create, set masks once, submit, read.  The C ABI
also lets a caller change a context between batches -- fm_reset_stream, fm_set_mask (replace, clear),
fm_write_background, fm_set_hip_stream -- and after a reset the next batch is a first frame for one stream
and a steady-state frame for the others, which every pixel path selects per stream.  Here one script of such
changes runs on every product pixel path (the smallest shape that still selects it), each batch compared with
the CPU oracle bit for bit: masks, counts, boxes, origins and the float64 background.

Frames are the seeded streams of find_motion_amd.synthetic, every STEP-th frame from START (consecutive frames
move the rectangles less than a pixel at these sizes, which the wide blurs swallow); every batch is required to
show at least one contour on every stream, so no comparison is of empty masks.
"""
import time

import numpy as np
import pytest

import oracle
from find_motion_amd import MotionEngine, rasterize_masks
from find_motion_amd._native import FM_EINVAL, FM_ESTATE, FMError, PLANE_BLUR, PLANE_DELTA, PLANE_GRAY
from find_motion_amd.synthetic import batch

pytestmark = pytest.mark.gpu

# path -> (W, H, box, k, keep_planes, the launch name fm_kernel_times shows for it, its first-frame launch)
PATHS = {
    # fm_small.hip without a resize.  Its blur keeps the frame's gray bytes, u32 row sums and the reflected
    # indices in 64 KB of LDS (small_supported: 64,672 bytes at 176 x 72, a two-tile-row image it takes) ...
    "small":   (176, 72, 176, 5, False, "small_scan", "small_scan_init"),
    # ... and 200 x 72 (73,408 bytes) is past it: k_pix5 / k_pix<5> with an 8-row second tile row
    "pix5_72": (200, 72, 200, 5, False, "pix", "pix_init"),
    "small_d": (640, 480, 100, 5, False, "small_scan", "small_scan_init"),  # ... behind INTER_AREA (mode D)
    "pix5":    (200, 136, 200, 5, False, "pix", "pix_init"),                # k_pix5 (steady), k_pix<5> (init)
    "pix7p":   (200, 136, 200, 7, True, "pix", "pix_init"),                 # k_pix<7> writing the planes
    "pix21":   (200, 131, 200, 21, False, "pix", "pix_init"),               # k = 21
    "fused11": (256, 200, 256, 11, False, "fused", None),                   # k_fused, generic taps
    "pixel51": (256, 200, 256, 51, False, "pixel", None),                   # per-frame k_pixel + pixel-level CCL
}
PIXEL_LAUNCHES = {"small_scan", "pix", "fused", "pixel"}
START, STEP = 40, 12  # frames START, START + STEP, ... of the synthetic streams


def _raises(code, call, *args):
    with pytest.raises(FMError) as e:
        call(*args)
    assert e.value.code == code, e.value


def crafted_plane(blur, seed):
    """A float64 background as test_convert_scale_abs_ties_and_saturation builds it -- exact .5 ties, values just
    off them, other non-integers, negatives and values above 255 (convertScaleAbs's rounding and saturation) -- in
    the top third of the plane, and the blur's own values below it (a background that matches the scene)."""
    h, w = blur.shape
    rng = np.random.default_rng(seed)
    p = blur.astype(np.float64)
    rows = max(2, h // 3)
    base = np.floor(rng.random((rows, w)) * 300 - 20)
    frac = rng.choice([0.5, -0.5, 0.4999999999, 0.5000000001, 0.25, 0.0, 1.5, 2.5], size=(rows, w))
    p[:rows] = base + frac
    p[0, :8] = [-0.5, -1.5, 255.5, 256.5, 254.5, 0.5, 1e9, -1e9]
    return p


class Run:
    """An engine and one OracleStream per stream, driven together: every state change goes to both."""

    def __init__(self, name, S, T, profile=False):
        self.W, self.H, self.box, self.k, self.planes, self.launch, self.init_launch = PATHS[name]
        self.S, self.T = S, T
        self.eng = MotionEngine(n_streams=S, src_w=self.W, src_h=self.H, box_size=self.box, ksize=self.k,
                                threshold=12, avg=0.1, max_batch=T, keep_planes=self.planes, profile=profile)
        self.cfg = oracle.OracleConfig(H=self.H, W=self.W, box=self.box, ksize=self.k, thresh=12, alpha=0.1)
        assert (self.cfg.h, self.cfg.w) == self.eng.work_shape
        self.orc = [oracle.OracleStream(self.cfg) for _ in range(S)]
        self.pos = START
        self.nb = 0

    # -- frames ------------------------------------------------------------------
    def frames(self):
        fr = np.concatenate([batch(self.W, self.H, self.S, self.pos + STEP * t, 1) for t in range(self.T)])
        self.pos += STEP * self.T
        return fr

    def next_blur(self, s):
        """blur of stream s's next frame (fm.py:490-494)."""
        fr = batch(self.W, self.H, self.S, self.pos, 1)[0, s]
        return oracle.gauss_blur(oracle.bgr2gray(oracle.resize_area_bgr(fr, self.box)), self.k)

    def mask(self, polygon):
        h, w = self.eng.work_shape
        return rasterize_masks(h, w, self.box / self.W, [polygon])

    # -- state, mirrored ------------------------------------------------------------
    def set_background(self, s, bg):
        self.eng.set_background(s, bg)
        self.orc[s].set_background(bg)
        got = self.eng.background(s)
        assert np.array_equal(got, bg), f"background({s}) after set_background: {int((got != bg).sum())} values differ"

    def reset(self, s):
        self.eng.reset(s)
        self.orc[s].reset()

    def set_mask(self, s, keep):
        self.eng.set_mask(s, keep)
        self.orc[s].keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)

    def clone(self, s):
        o = self.orc[s]
        c = oracle.OracleStream(self.cfg, None if o.keep is None else o.keep.copy())
        if o.initialized:
            c.set_background(o.bg)
        return c

    def check_state(self):
        for s, o in enumerate(self.orc):
            assert self.eng.initialized(s) == o.initialized, f"initialized({s})"
            if not o.initialized:
                _raises(FM_ESTATE, self.eng.background, s)

    # -- batches ---------------------------------------------------------------------
    def finish(self, fr, tag=""):
        """wait() for the batch of frames fr [T][S][H][W][3] and compare every frame of every stream with
        the oracle, then every stream's background.  Returns the oracle's results [t][s]."""
        eng = self.eng
        tag = f"batch {self.nb} {tag}"
        self.nb += 1
        eng.wait()
        counts = eng.counts()
        refs = []
        seen = [0] * self.S
        steady = [0] * self.S
        for t in range(fr.shape[0]):
            row = []
            for s in range(self.S):
                first = not self.orc[s].initialized
                ref = self.orc[s].step(fr[t, s])
                row.append(ref)
                at = f"{tag}: frame {t} stream {s}"
                if self.planes:
                    for which, key in ((PLANE_GRAY, "gray"), (PLANE_BLUR, "blur"), (PLANE_DELTA, "delta")):
                        np.testing.assert_array_equal(eng.plane(which, t, s), ref[key], err_msg=f"{key} {at}")
                np.testing.assert_array_equal(eng.mask(t, s), ref["mask"], err_msg="mask " + at)
                assert counts[t, s] == ref["count"], at
                got = eng.contours(t, s)
                assert [c.bbox for c in got] == ref["boxes"], at
                assert [c.origin for c in got] == ref["origins"], at
                if first:  # a first frame is its own background: its delta is zero whatever it shows
                    assert ref["count"] == 0, at
                else:
                    steady[s] += 1
                    seen[s] += ref["count"]
            refs.append(row)
        for s in range(self.S):
            assert eng.initialized(s)
            bg = eng.background(s)
            assert np.array_equal(bg, self.orc[s].bg), \
                f"{tag}: background stream {s}: {int((bg != self.orc[s].bg).sum())} values differ"
            # the comparison is not of empty masks (a stream whose only frame was its first has none to show)
            assert seen[s] > 0 or steady[s] == 0, f"{tag}: the oracle finds no contour on stream {s}"
        return refs

    def batch(self, tag=""):
        fr = self.frames()
        self.eng.submit(fr)
        return fr, self.finish(fr, tag)


# --- 2. one script on every pixel path ------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PATHS))
def test_script_shapes_run_the_kernel_they_name(name):
    """Each shape of the script selects the pixel path it stands for, read from the engine's own launch timing
    (as test_product_kernel_selection does): the steady-state launch, no other path's, and -- where first
    frames have a launch of their own -- that launch, on the mixed batch after a reset."""
    r = Run(name, 3, 3, profile="pix")
    eng = r.eng
    try:
        for b in range(3):
            if b == 2:
                eng.reset(1)
            eng.submit(r.frames())
            eng.wait()
        names = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0}
    finally:
        eng.close()
    assert names & PIXEL_LAUNCHES == {r.launch}, names
    if r.init_launch:
        assert r.init_launch in names, names


@pytest.mark.parametrize("name,T", [(n, 3) for n in PATHS] + [("pix5", 1), ("small", 1)])
def test_state_changes_between_batches(name, T):
    """The script, S = 3.  bg_cur (the background plane the next launch reads, and fm_write_background writes)
    flips once per pixel launch: a batch with a first frame is two launches on the k_pix / small-image paths at
    T = 3, one at T = 1 and on k_fused, T on the per-frame path.  Launches before the two set_background(0, P2):
    k_pix / small T = 3: 5 and 8; one launch per batch: 3 and 6; per-frame T = 3: 9 and 18 -- odd and even on
    every path."""
    S = 3
    r = Run(name, S, T)
    eng = r.eng
    try:
        # 1. a background written before any frame: batch 0 initialises streams 0 and 2 only
        r.check_state()
        assert not any(eng.initialized(s) for s in range(S))
        r.set_background(1, crafted_plane(r.next_blur(1), 1))
        r.check_state()
        assert [eng.initialized(s) for s in range(S)] == [False, True, False]
        r.batch("mixed first frames (0, 2)")
        # 2. steady state
        r.batch("steady")
        # 3. stream 1 re-initialises from its own frame while 0 and 2 continue
        r.reset(1)
        r.check_state()
        assert [eng.initialized(s) for s in range(S)] == [True, False, True]
        r.batch("stream 1 reset")
        # 7a. a background written directly after a batch that had a first-frame launch
        P2 = crafted_plane(r.next_blur(0), 2)
        r.set_background(0, P2)
        # 4. the first mask of the context, on one stream: the KEEP kernel variants
        A = r.mask(((0, 0), (r.W // 3, r.H // 2)))
        B = r.mask(((r.W - 1, r.H - 1), (r.W // 2, r.H - 1), (r.W - 1, r.H // 3)))
        assert A.min() == 0 and B.min() == 0 and A.max() == 1 and not np.array_equal(A, B)
        r.set_mask(2, A)
        r.batch("mask A on stream 2, background P2 on stream 0")
        # 5. the mask replaced, and a second stream masked
        r.set_mask(2, B)
        r.set_mask(0, A)
        r.batch("mask B on stream 2, A on stream 0")
        # 6. the mask cleared: the stale bytes of B stay in the context behind a zero flag
        stale = r.clone(2)
        r.set_mask(2, None)
        fr, refs = r.batch("mask cleared on stream 2")
        # Not vacuous: an oracle that still applies B ends the batch with another background wherever B masks
        # (its blur stays 0 there).  The masks may coincide -- under B the background decayed to 0.73 of the
        # scene, so both |scene - bg| and |0 - bg| pass the threshold -- which is why the background, compared
        # bit for bit after every batch, is what pins this step.
        for t in range(T):
            stale.step(fr[t, 2])
        assert (stale.bg != r.orc[2].bg)[B == 0].any() and np.array_equal(stale.bg[B == 1], r.orc[2].bg[B == 1])
        assert all(refs[t][2]["blur"][B == 0].any() for t in range(T))
        # 7b. the same write after a batch that had no first-frame launch
        r.set_background(0, P2)
        r.batch("background P2 on stream 0 again")
        # 8. every stream reset mid-run
        for s in range(S):
            r.reset(s)
        r.check_state()
        assert not any(eng.initialized(s) for s in range(S))
        r.batch("all streams reset")
        r.batch("steady after the reset")
        r.check_state()
    finally:
        eng.close()


# --- 3. refusals while a batch is in flight ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pix5", "pixel51"])
def test_state_calls_are_refused_while_a_batch_is_in_flight(name):
    """fm_set_mask, fm_reset_stream, fm_write_background, fm_read_background and fm_set_hip_stream return
    FM_ESTATE between fm_submit and fm_wait and change nothing: the batch in flight and the next one equal the
    oracle.  Afterwards each succeeds and takes effect; stream indices out of range are FM_EINVAL."""
    import torch

    S, T = 2, 3
    r = Run(name, S, T)
    eng = r.eng
    st = torch.cuda.Stream()
    try:
        r.batch("first")
        keep = r.mask(((0, 0), (r.W // 3, r.H // 2)))
        plane = crafted_plane(r.next_blur(0), 5)
        fr = r.frames()
        eng.submit(fr)
        _raises(FM_ESTATE, eng.set_mask, 0, keep)
        _raises(FM_ESTATE, eng.set_mask, 0, None)
        _raises(FM_ESTATE, eng.reset, 1)
        _raises(FM_ESTATE, eng.set_background, 0, plane)
        _raises(FM_ESTATE, eng.background, 0)
        _raises(FM_ESTATE, eng.set_hip_stream, st.cuda_stream)
        _raises(FM_ESTATE, eng.set_hip_stream, None)
        assert all(eng.initialized(s) for s in range(S))
        r.finish(fr, "in flight during the refused calls")
        r.batch("after the refused calls")
        # idle: each call succeeds and shows in the next batch
        h, w = eng.work_shape
        for bad in (-1, S):
            _raises(FM_EINVAL, eng.set_mask, bad, keep)
            _raises(FM_EINVAL, eng.set_mask, bad, None)
            _raises(FM_EINVAL, eng.reset, bad)
            _raises(FM_EINVAL, eng.set_background, bad, plane)
            _raises(FM_EINVAL, eng.background, bad)
        r.set_mask(0, keep)
        r.reset(1)
        r.set_background(0, crafted_plane(r.next_blur(0), 5))
        eng.set_hip_stream(st.cuda_stream)
        r.check_state()
        r.batch("mask, reset, background and the caller's stream")
        eng.set_hip_stream(None)
        r.batch("own stream again")
    finally:
        eng.close()


# --- 4. the caller's stream ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pix5", "small_d"])
def test_callers_stream_results_and_teardown(name):
    """fm_set_hip_stream with a torch stream's handle (identity mode, and mode D whose resize runs on the
    context's input stream): batches on it, then on the context's own stream again, equal the oracle; the
    context's teardown leaves the caller's stream usable."""
    import torch

    S, T = 2, 3
    st = torch.cuda.Stream()
    r = Run(name, S, T)
    eng = r.eng
    try:
        eng.set_hip_stream(st.cuda_stream)
        for b in range(3):
            r.batch("on the caller's stream")
            if b == 1:
                r.reset(0)
        with torch.cuda.stream(st):
            mid = torch.arange(4096, device="cuda").sum()
        eng.set_hip_stream(None)
        for b in range(2):
            r.batch("on the context's stream")
        eng.set_hip_stream(st.cuda_stream)
        r.batch("back on the caller's stream")
    finally:
        eng.close()
    with torch.cuda.stream(st):
        x = torch.arange(4096, device="cuda").sum()
    st.synchronize()
    assert int(x) == int(mid) == 4095 * 4096 // 2


_DELAY = {}


def _enqueue_delay(torch, st, ms):
    """About `ms` milliseconds of device work on stream st: torch.cuda._sleep, its cycles per millisecond measured
    once with events, or (without it) a chain of matmuls timed the same way."""
    if not _DELAY:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if hasattr(torch.cuda, "_sleep"):
            n = 2_000_000
            torch.cuda._sleep(1000)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            _DELAY["sleep"] = n / max(a.elapsed_time(b), 1e-3)
        else:
            m = torch.ones((2048, 2048), device="cuda")
            torch.mm(m, m)
            a.record()
            for _ in range(8):
                torch.mm(m, m)
            b.record()
            b.synchronize()
            _DELAY["mm"] = (m, max(a.elapsed_time(b), 1e-3) / 8)
    with torch.cuda.stream(st):
        if "sleep" in _DELAY:
            torch.cuda._sleep(int(ms * _DELAY["sleep"]))
        else:
            m, each = _DELAY["mm"]
            for _ in range(int(ms / each) + 1):
                torch.mm(m, m)


def _nv12(bgr):
    """A tight NV12 frame with the BGR frame's content as luma and chroma (there is motion in all three)."""
    f = bgr.astype(np.int32)
    Y = ((f[..., 2] * 77 + f[..., 1] * 150 + f[..., 0] * 29) >> 8).astype(np.uint8)
    return np.concatenate([Y.ravel(), np.stack([bgr[::2, ::2, 0], bgr[::2, ::2, 2]], -1).ravel()])


def _nv12_to_bgr(buf, W, H):
    """cv2.cvtColor(COLOR_YUV2BGR_NV12) of a tight frame: yuv_ref.pixel's integers on whole planes."""
    Y = buf[:W * H].reshape(H, W).astype(np.int64)
    uv = buf[W * H:W * H * 3 // 2].reshape(H // 2, W // 2, 2).astype(np.int64) - 128
    U, V = (np.repeat(np.repeat(uv[..., i], 2, 0), 2, 1) for i in range(2))
    y = np.maximum(Y - 16, 0) * 1220542 + 524288
    bgr = np.stack([(y + 2116026 * U) >> 20, (y - 852492 * V - 409993 * U) >> 20, (y + 1673527 * V) >> 20], -1)
    return np.clip(bgr, 0, 255).astype(np.uint8)


def test_nv12_reference_of_this_file_equals_yuv_ref():
    import yuv_ref

    W, H = 16, 8
    buf = yuv_ref.random_frames(np.random.default_rng(3), 1, W, H, "NV12")
    np.testing.assert_array_equal(_nv12_to_bgr(buf, W, H), yuv_ref.yuv_ref(buf, W, H, "NV12"))


# Measured on an MI355X (the test prints the figure of each case): the racing fm_submit* call returned after
# 0.040 (device, identity), 0.077 (device, mode D), 0.073 (streams, identity), 0.233 (streams, mode D) and
# 0.281 ms (NV12, mode D) of host time.  The delay queued in front of the fill is ten times the largest.
SUBMIT_HOST_MS = 0.3
DELAY_MS = 10 * SUBMIT_HOST_MS


@pytest.mark.parametrize("case", ["device_identity", "device_mode_d", "streams_identity", "streams_mode_d",
                                  "yuv_mode_d"])
def test_device_input_is_read_after_the_callers_stream_wrote_it(case):
    """On a caller's stream a batch is ordered after the work queued there before the submit.  The caller's
    stream gets a delay, then the asynchronous copy that fills the device buffer (which holds zeros until then),
    then -- with no host synchronisation -- the submit.  An event recorded after the fill must still be pending
    when the submit returns (else the race window was closed and the test has shown nothing: it fails); the
    batch's results must be those of the new frames.

    submit_device in identity mode reads in place on the caller's stream.  In mode D the INTER_AREA resize, and
    in either mode submit_streams' strided copy and submit_yuv's conversion, run on the context's input stream,
    which waits for an event recorded on the caller's stream first (without it these four cases read the zeros).

    Figures (MI355X): the submit call's host time is 0.04 to 0.28 ms (SUBMIT_HOST_MS = 0.3), the delay
    DELAY_MS = 10 x SUBMIT_HOST_MS = 3 ms."""
    import torch

    kind = case.split("_")[0]
    name = "pix5" if case.endswith("identity") else "small_d"
    S, T = 2, 2
    r = Run(name, S, T)
    eng = r.eng
    W, H = r.W, r.H
    st = torch.cuda.Stream()

    def make():
        """(the device buffer's bytes, the batch as BGR frames [T][S][H][W][3])"""
        fr = r.frames()
        if kind == "device":
            return fr, fr
        if kind == "streams":
            return np.ascontiguousarray(fr.transpose(1, 0, 2, 3, 4)), fr  # [S][T]: one buffer per stream
        yuv = np.stack([[_nv12(fr[t, s]) for s in range(S)] for t in range(T)])
        bgr = np.stack([[_nv12_to_bgr(yuv[t, s], W, H) for s in range(S)] for t in range(T)])
        return yuv, bgr

    try:
        eng.set_hip_stream(st.cuda_stream)
        host, bgr = make()
        dev = torch.zeros(host.shape, dtype=torch.uint8, device="cuda")

        def submit():
            if kind == "device":
                eng.submit_device(dev.data_ptr(), T)
            elif kind == "streams":
                eng.submit_streams([dev[s].data_ptr() for s in range(S)], on_device=True, n_frames=T)
            else:
                eng.submit_yuv_device(dev.data_ptr(), T, "NV12")

        for b in range(2):  # the first batches, the fill synchronised: the slots' streams and the background exist
            pin = torch.from_numpy(host).pin_memory()
            with torch.cuda.stream(st):
                dev.copy_(pin, non_blocking=True)
            st.synchronize()
            submit()
            r.finish(bgr, "synchronised fill")
            host, bgr = make()
        # what the batch would give if the zeros were read: not the new frames' results
        zeros = np.zeros_like(bgr) if kind != "yuv" else np.broadcast_to(
            _nv12_to_bgr(np.zeros(W * H * 3 // 2, np.uint8), W, H), bgr.shape)
        for s in range(S):
            a, z = r.clone(s), r.clone(s)
            assert any(not np.array_equal(a.step(bgr[t, s])["mask"], z.step(zeros[t, s])["mask"]) for t in range(T))
        pin = torch.from_numpy(host).pin_memory()
        with torch.cuda.stream(st):
            dev.zero_()
        _enqueue_delay(torch, st, 0.01)  # (the delay's calibration, outside the window)
        torch.cuda.synchronize()
        filled = torch.cuda.Event()
        _enqueue_delay(torch, st, DELAY_MS)
        with torch.cuda.stream(st):
            dev.copy_(pin, non_blocking=True)
            filled.record(st)
        t0 = time.perf_counter()
        submit()
        host_ms = (time.perf_counter() - t0) * 1e3
        window_open = not filled.query()
        print(f"\n{case}: submit returned after {host_ms:.3f} ms of host time; delay {DELAY_MS} ms; "
              f"fill pending at return: {window_open}")
        assert window_open, f"the fill had completed when submit returned ({host_ms:.3f} ms): no race window"
        r.finish(bgr, "fill queued behind a delay, no host synchronisation")
        assert filled.query()
        r.batch("host frames afterwards")
    finally:
        eng.close()
    st.synchronize()


# --- 5. the drop-in ----------------------------------------------------------------------------------------------------

def test_video_motion_ref_frame_assignments(tmp_path):
    """VideoMotion.ref_frame on the GPU (fm.py:363, 414): None before the first frame, the oracle's background
    after a batch, None assigned -> the next frame re-initialises, an array assigned -> the stream continues from
    it; every frame's mask and contours against the oracle.  pipeline_depth = 1: the engine is idle whenever
    read() has handed out a batch's first frame."""
    from find_motion_amd import motion, videoio

    W, H, T, NB = 192, 108, 4, 4
    cap = videoio.SyntheticCapture(W, H, T * NB, 0, start=START)
    vm = motion.VideoMotion(filename=str(tmp_path / "v"), capture=cap, box_size=100, threshold=12, batch=T,
                            pipeline_depth=1, outdir=str(tmp_path))
    cfg = oracle.OracleConfig(H=H, W=W, box=100, ksize=5, thresh=12, alpha=0.1)
    st = oracle.OracleStream(cfg)
    vid = videoio.SyntheticCapture(W, H, T * NB, 0, start=START)
    assert vm.ref_frame is None
    for b in range(NB):
        if b == 2:
            vm.ref_frame = None
            st.reset()
            assert vm.ref_frame is None
        if b == 3:
            fr = vid.video.frame(START + b * T)
            plane = crafted_plane(oracle.gauss_blur(oracle.bgr2gray(oracle.resize_area_bgr(fr, 100)), 5), 7)
            vm.ref_frame = plane
            st.set_background(plane)
            np.testing.assert_array_equal(vm.ref_frame, plane)
        refs = [st.step(vid.video.frame(START + b * T + t)) for t in range(T)]
        seen = 0
        for t in range(T):
            assert vm.read()
            if t == 0:  # the batch is done and nothing is in flight
                np.testing.assert_array_equal(vm.ref_frame, st.bg, err_msg=f"ref_frame after batch {b}")
            vf = vm.current_frame
            np.testing.assert_array_equal(vf.thresh, refs[t]["mask"], err_msg=f"batch {b} frame {t}")
            assert [c.bbox for c in vf.contours] == refs[t]["boxes"], (b, t)
            seen += refs[t]["count"]
        assert seen > 0, b
        if b in (0, 2):
            assert refs[0]["count"] == 0 and not refs[0]["delta"].any()  # a first frame
    assert not vm.read()
    vm.engine.close()
