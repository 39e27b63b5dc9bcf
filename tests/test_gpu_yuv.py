"""YUV input on the GPU (fm_submit_yuv / fm_submit_yuv_list, fm_yuv.hip): NV12, I420, YUY2 and UYVY frames
converted into the batch slot's BGR input buffer in front of the unchanged hot path.

The reference is tests/yuv_ref.py, a per-pixel Python restatement of cv2.cvtColor's COLOR_YUV2BGR_* arithmetic;
every comparison is byte for byte (the conversion is integer).  Inputs are seeded random full-range bytes --
padding included, which nothing may read -- with the known-answer triples planted.
"""
import ctypes as C

import numpy as np
import pytest

import yuv_ref
from find_motion_amd import MotionEngine, motion, videoio
from find_motion_amd._native import FM_EINVAL, FM_OK, FMError, FMYuvLayout, yuv_format
from find_motion_amd.synthetic import SyntheticVideo, batch

pytestmark = pytest.mark.gpu

FORMATS = yuv_ref.FORMATS
# the minimum size; a tail shorter than a lane's run of 16 pixels; widths that cross a lane group and a wave;
# then widths that are multiples of 16, the only ones whose rows keep every address 16-byte aligned, so that
# the wide (16-byte load / store) path runs at all: 3 runs, and 17 (more than one 16-lane group)
SIZES = [(2, 2), (6, 4), (34, 18), (130, 66), (258, 34), (48, 6), (272, 4)]


def layouts(fmt, W, H):
    """(pitch, chroma_offset, frame_stride): tight; the odd one (every row at another alignment: the narrow
    path); an aligned one with padding (the wide path over a pitch that is not the width)."""
    planar = fmt in yuv_ref.PLANAR
    out = [(0, 0, 0)]
    for pad, gap in ((2, 6), (16, 32)):
        pitch = W + pad if planar else 2 * W + 2 * pad
        coff = pitch * H + gap if planar else 0
        out.append((pitch, coff, yuv_ref.frame_bytes(W, H, fmt, pitch, coff) + gap + 4 * (gap == 6)))
    return out


def frame_of(buf, i, W, H, fmt, pitch=0, coff=0, stride=0):
    size = yuv_ref.frame_bytes(W, H, fmt, pitch, coff)
    stride = stride or size
    return buf[i * stride: i * stride + size]


def refs_of(buf, n, W, H, fmt, pitch=0, coff=0, stride=0):
    return [yuv_ref.yuv_ref(frame_of(buf, i, W, H, fmt, pitch, coff, stride), W, H, fmt, pitch, coff) for i in range(n)]


def engine(W, H, S, T, box=None, ksize=1, **kw):
    return MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=box or W, ksize=ksize, threshold=12, avg=0.1,
                        max_batch=T, **kw)


# --- exactness --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_conversion_is_exact(fmt, W, H):
    """fm_read_frame of every (t, s) of a 3-frame, 2-stream batch equals yuv_ref byte for byte, for the tight
    layout and for pitched ones with a chroma offset and a frame stride.  fm_create takes every size here
    (2 x 2 included: the work image is the frame, ksize 1)."""
    S, T = 2, 3
    eng = engine(W, H, S, T)
    rng = np.random.default_rng(1000 * W + 10 * H + FORMATS.index(fmt))
    for pitch, coff, stride in layouts(fmt, W, H):
        buf = yuv_ref.random_frames(rng, T * S, W, H, fmt, pitch, coff, stride)
        want = refs_of(buf, T * S, W, H, fmt, pitch, coff, stride)
        eng.submit_yuv(buf, fmt, pitch, coff, stride, n_frames=T)
        eng.wait()
        for t in range(T):
            for s in range(S):
                np.testing.assert_array_equal(eng.read_frame(t, s), want[t * S + s],
                                              err_msg=f"{fmt} {W}x{H} layout {(pitch, coff, stride)} frame {t} stream {s}")
    eng.close()


def test_known_answers_on_the_gpu():
    """Each KAT triple as its own pixel group of one frame, every format."""
    W, H = 2 * len(yuv_ref.KAT), 2
    eng = engine(W, H, 1, 1)
    for fmt in FORMATS:
        buf = np.full(yuv_ref.frame_bytes(W, H, fmt), 77, np.uint8)
        for k, (yuv, _) in enumerate(yuv_ref.KAT):
            for y in range(H):
                for x in (2 * k, 2 * k + 1):
                    yuv_ref.plant(buf, W, H, fmt, x, y, yuv)
        eng.submit_yuv(buf, fmt, n_frames=1)
        eng.wait()
        got = eng.read_frame(0, 0)
        for k, (yuv, bgr) in enumerate(yuv_ref.KAT):
            assert (got[:, 2 * k: 2 * k + 2] == np.array(bgr, np.uint8)).all(), (fmt, yuv, got[0, 2 * k].tolist())
    eng.close()


# --- equivalence with BGR input -----------------------------------------------------------------------------

def pack(fmt, Y, U, V):
    """A tight frame from a luma plane (H, W) and full-resolution chroma planes, subsampled by dropping."""
    if fmt == "NV12":
        return np.concatenate([Y.ravel(), np.stack([U[::2, ::2], V[::2, ::2]], -1).ravel()])
    if fmt == "I420":
        return np.concatenate([Y.ravel(), U[::2, ::2].ravel(), V[::2, ::2].ravel()])
    u, v = U[:, ::2], V[:, ::2]
    q = [Y[:, ::2], u, Y[:, 1::2], v] if fmt == "YUY2" else [u, Y[:, ::2], v, Y[:, 1::2]]
    return np.stack(q, -1).ravel()


def yuv_batch(fmt, W, H, S, start, T):
    """[T][S][frame bytes]: the synthetic streams' moving content as luma and chroma (so there is motion)."""
    out = np.empty((T, S, yuv_ref.frame_bytes(W, H, fmt)), np.uint8)
    for s in range(S):
        vid = SyntheticVideo(W, H, s)
        for t in range(T):
            bgr = vid.frame((start + t) * 16)  # every 16th frame: the rectangles move several pixels a step
            f = bgr.astype(np.int32)
            Y = ((f[..., 2] * 77 + f[..., 1] * 150 + f[..., 0] * 29) >> 8).astype(np.uint8)
            out[t, s] = pack(fmt, Y, bgr[..., 0], bgr[..., 2])
    return out


def results(eng, T, S):
    out = {"counts": eng.counts().copy()}
    for t in range(T):
        for s in range(S):
            out[f"mask{t},{s}"] = eng.mask(t, s)
            out[f"rec{t},{s}"] = [(c.bbox, c.origin) for c in eng.contours(t, s)]
    return out


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag} {k}")
        else:
            assert a[k] == b[k], f"{tag} {k}"


@pytest.mark.parametrize("box", [130, 64])  # the work image is the frame; a resize in front of the pixel kernel
@pytest.mark.parametrize("fmt", FORMATS)
def test_same_results_as_bgr_input(fmt, box):
    W, H, S, T = 130, 66, 2, 3
    a, b = engine(W, H, S, T, box, ksize=5), engine(W, H, S, T, box, ksize=5)
    for nb in range(2):
        yuv = yuv_batch(fmt, W, H, S, nb * T, T)
        bgr = np.stack([yuv_ref.yuv_ref(yuv[t, s], W, H, fmt) for t in range(T) for s in range(S)]).reshape(T, S, H, W, 3)
        a.submit_yuv(yuv, fmt)
        b.submit(bgr)
        a.wait()
        b.wait()
        ra, rb = results(a, T, S), results(b, T, S)
        if nb:
            assert ra["counts"].sum() > 0  # (the streams move: the comparison is not of empty masks)
        assert_same(ra, rb, f"{fmt} box {box} batch {nb}")
        for s in range(S):
            np.testing.assert_array_equal(a.background(s), b.background(s), err_msg=f"background {fmt} batch {nb} stream {s}")
    a.close()
    b.close()


# --- host memory, device memory, a list of surfaces -----------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_host_device_and_list_agree(fmt):
    torch = pytest.importorskip("torch")
    W, H, S, T = 34, 18, 2, 3
    pitch, coff, stride = layouts(fmt, W, H)[1]
    rng = np.random.default_rng(7 + FORMATS.index(fmt))
    buf = yuv_ref.random_frames(rng, T * S, W, H, fmt, pitch, coff, stride)
    want = refs_of(buf, T * S, W, H, fmt, pitch, coff, stride)
    size = yuv_ref.frame_bytes(W, H, fmt, pitch, coff)
    host, dev, lst = (engine(W, H, S, T, ksize=3) for _ in range(3))
    host.submit_yuv(buf, fmt, pitch, coff, stride, n_frames=T)
    dbuf = torch.from_numpy(buf).cuda()
    # the same frames scattered, in another order and at odd addresses, in a larger allocation
    big = torch.from_numpy(rng.integers(0, 256, T * S * (size + 101) + 64, dtype=np.uint8)).cuda()
    ptrs = [0] * (T * S)
    for k, i in enumerate(reversed(range(T * S))):
        off = 3 + k * (size + 101)
        big[off: off + size] = dbuf[i * stride: i * stride + size]
        ptrs[i] = big.data_ptr() + off
    torch.cuda.synchronize()
    dev.submit_yuv_device(dbuf.data_ptr(), T, fmt, pitch, coff, stride)
    lst.submit_yuv_list(ptrs, fmt, pitch, coff)
    engs = {"host": host, "device": dev, "list": lst}
    res = {}
    for name, e in engs.items():
        e.wait()
        res[name] = results(e, T, S)
        for t in range(T):
            for s in range(S):
                np.testing.assert_array_equal(e.read_frame(t, s), want[t * S + s], err_msg=f"{name} {fmt} {t},{s}")
        res[name]["bg"] = np.stack([e.background(s) for s in range(S)])
    assert_same(res["host"], res["device"], f"{fmt} host vs device")
    assert_same(res["host"], res["list"], f"{fmt} host vs list")
    for e in engs.values():
        e.close()
    del dbuf, big


# --- batches in flight ----------------------------------------------------------------------------------------

def test_batches_in_flight_keep_their_own_staging():
    """fm_max_inflight YUV batches of different content submitted before the first wait, then another round
    that wraps the slot ring: each batch's frames and counts are its own (a staging buffer shared between
    slots would hold the last batch's frames)."""
    W, H, S, T, fmt = 34, 18, 1, 2, "NV12"
    eng, ref = engine(W, H, S, T, ksize=3), engine(W, H, S, T, ksize=3)
    n = eng.max_inflight
    rng = np.random.default_rng(99)
    for rnd in range(2):
        bufs = [yuv_ref.random_frames(rng, T * S, W, H, fmt) for _ in range(n)]
        for b in bufs:
            eng.submit_yuv(b, fmt, n_frames=T)
        for i, b in enumerate(bufs):
            want = refs_of(b, T * S, W, H, fmt)
            ref.submit(np.stack(want).reshape(T, S, H, W, 3))
            ref.wait()
            eng.wait()
            for t in range(T):
                np.testing.assert_array_equal(eng.read_frame(t, 0), want[t], err_msg=f"round {rnd} batch {i} frame {t}")
            np.testing.assert_array_equal(eng.counts(), ref.counts(), err_msg=f"round {rnd} batch {i}")
    np.testing.assert_array_equal(eng.background(0), ref.background(0))
    eng.close()
    ref.close()


# --- mixing with BGR batches ------------------------------------------------------------------------------------

def test_yuv_and_bgr_batches_mix_on_one_context():
    W, H, S, T, fmt = 130, 66, 2, 3, "YUY2"
    mixed, plain = engine(W, H, S, T, ksize=5), engine(W, H, S, T, ksize=5)
    for nb in range(3):
        yuv = yuv_batch(fmt, W, H, S, nb * T, T)
        bgr = np.stack([videoio.yuv_to_bgr(yuv[t, s], W, H, fmt) for t in range(T) for s in range(S)]).reshape(T, S, H, W, 3)
        if nb == 1:
            mixed.submit(bgr)
        else:
            mixed.submit_yuv(yuv, fmt)
        plain.submit(bgr)
        mixed.wait()
        plain.wait()
        assert_same(results(mixed, T, S), results(plain, T, S), f"batch {nb}")
        for s in range(S):
            np.testing.assert_array_equal(mixed.background(s), plain.background(s))
    mixed.close()
    plain.close()


# --- errors -----------------------------------------------------------------------------------------------------

def test_bad_arguments_enqueue_nothing():
    W, H, S, T = 34, 18, 1, 2
    eng = engine(W, H, S, T, ksize=3)
    L, h = eng._L, eng._h
    buf = np.zeros(4 * yuv_ref.frame_bytes(W, H, "YUY2") + 4096, np.uint8)
    ptr = buf.ctypes.data
    arr = (C.c_void_p * (T * S))(*([ptr] * (T * S)))
    lay = lambda *a: C.byref(FMYuvLayout(*a))  # noqa: E731
    bad = [
        (ptr, 1, None), (None, 1, lay(0, 0, 0, 0)),                       # null layout, null frames
        (ptr, 1, lay(4, 0, 0, 0)), (ptr, 1, lay(-1, 0, 0, 0)),            # unknown format
        (ptr, 1, lay(0, W - 1, 0, 0)), (ptr, 1, lay(2, 2 * W - 1, 0, 0)),  # pitch below tight
        (ptr, 1, lay(1, W + 1, 0, 0)),                                    # odd pitch, I420
        (ptr, 1, lay(0, 0, W * H - 1, 0)), (ptr, 1, lay(1, 36, 36 * H - 1, 0)),  # chroma inside the luma plane
        (ptr, 1, lay(0, 0, 0, W * H * 3 // 2 - 1)), (ptr, 1, lay(3, 0, 0, 2 * W * H - 1)),  # stride below the frame
        (ptr, 0, lay(0, 0, 0, 0)), (ptr, T + 1, lay(0, 0, 0, 0)), (ptr, -1, lay(2, 0, 0, 0)),  # n_frames
    ]
    for frames, n, layout in bad:
        for on_device in (0, 1):
            assert L.fm_submit_yuv(h, frames, n, layout, on_device) == FM_EINVAL, (n, on_device)
            assert L.fm_last_error(h)
        if frames is not None:
            assert L.fm_submit_yuv_list(h, C.cast(arr, C.c_void_p), n, layout) == FM_EINVAL
    assert L.fm_submit_yuv_list(h, None, 1, lay(0, 0, 0, 0)) == FM_EINVAL
    hole = (C.c_void_p * (T * S))(ptr, None)
    assert L.fm_submit_yuv_list(h, C.cast(hole, C.c_void_p), T, lay(0, 0, 0, 0)) == FM_EINVAL  # a null surface
    with pytest.raises(FMError) as e:
        eng.submit_yuv(buf, "NV12", pitch=W - 2, n_frames=1)
    assert e.value.code == FM_EINVAL
    assert L.fm_wait(h) == FM_OK  # nothing was in flight
    # every slot is still free: fm_max_inflight valid submits go through, and their results are right
    rng = np.random.default_rng(3)
    bufs = [yuv_ref.random_frames(rng, T, W, H, "UYVY") for _ in range(eng.max_inflight)]
    for b in bufs:
        eng.submit_yuv(b, "UYVY", n_frames=T)
    for b in bufs:
        eng.wait()
        np.testing.assert_array_equal(eng.read_frame(1, 0), yuv_ref.yuv_ref(frame_of(b, 1, W, H, "UYVY"), W, H, "UYVY"))
    eng.close()


def test_odd_width_context_refuses_yuv_but_takes_bgr():
    W, H = 33, 18
    eng = engine(W, H, 1, 1, ksize=3)
    buf = np.zeros(4 * W * H, np.uint8)
    for fmt in FORMATS:
        lay = FMYuvLayout(yuv_format(fmt), 0, 0, 0)
        assert eng._L.fm_submit_yuv(eng._h, buf.ctypes.data, 1, C.byref(lay), 0) == FM_EINVAL
        with pytest.raises(FMError):
            eng.submit_yuv(buf, fmt, n_frames=1)
    odd_h = engine(34, 17, 1, 1, ksize=3)  # an odd height: no 4:2:0, but the packed formats convert
    for fmt in ("NV12", "I420"):
        lay = FMYuvLayout(yuv_format(fmt), 0, 0, 0)
        assert odd_h._L.fm_submit_yuv(odd_h._h, buf.ctypes.data, 1, C.byref(lay), 0) == FM_EINVAL
    yb = yuv_ref.random_frames(np.random.default_rng(1), 1, 34, 17, "YUY2")
    odd_h.submit_yuv(yb, "YUY2", n_frames=1)
    odd_h.wait()
    np.testing.assert_array_equal(odd_h.read_frame(0, 0), yuv_ref.yuv_ref(yb, 34, 17, "YUY2"))
    odd_h.close()
    fr = batch(W, H, 1, 0, 1)
    eng.submit(fr)
    eng.wait()
    np.testing.assert_array_equal(eng.read_frame(0, 0), fr[0, 0])
    eng.close()


def test_profile_names_the_kernel_and_footprint_counts_the_staging():
    W, H, S, T = 130, 66, 1, 2
    eng = engine(W, H, S, T, ksize=5, profile=True)
    before = eng.footprint()["device_bytes"]
    buf = yuv_ref.random_frames(np.random.default_rng(4), T, W, H, "NV12")
    eng.submit_yuv(buf, "NV12", n_frames=T)
    eng.wait()
    times = eng.kernel_times()
    assert "yuv2bgr" in times and times["yuv2bgr"][1] == 1 and times["yuv2bgr"][0] > 0
    # the slot's BGR input buffer and its YUV staging, both allocated by the first host submit
    grown = eng.footprint()["device_bytes"] - before
    assert grown == T * S * W * H * 3 + T * S * yuv_ref.frame_bytes(W, H, "NV12")
    eng.close()


# --- the drop-in ------------------------------------------------------------------------------------------------

def test_video_motion_on_an_nv12_avi_equals_the_bgr_run(tmp_path):
    """VideoMotion over a small NV12 AVI (BatchFeeder's YUV mode, raw frames fetched lazily from the engine's
    input slot or converted on the host once their batch is gone) writes the same frame indices and the same
    raw AVI bytes as the run over the BGR AVI of the converted frames."""
    W, H, n = 320, 240, 40
    vid = SyntheticVideo(W, H, 1)
    yw = videoio.RawAviWriter(str(tmp_path / "yuv.avi"), 30, (W, H), fourcc="NV12")
    bw = videoio.RawAviWriter(str(tmp_path / "bgr.avi"), 30, (W, H))
    for i in range(n):
        f = vid.frame(i)
        g = f.astype(np.int32)
        Y = ((g[..., 2] * 77 + g[..., 1] * 150 + g[..., 0] * 29) >> 8).astype(np.uint8)
        fr = pack("NV12", Y, f[..., 0], f[..., 2])
        yw.write(fr)
        bw.write(videoio.yuv_to_bgr(fr, W, H, "NV12"))
    yw.release()
    bw.release()
    runs = {}
    for name in ("yuv", "bgr"):
        out = tmp_path / name
        out.mkdir()
        cap = videoio.RawAviCapture(str(tmp_path / f"{name}.avi"))
        vm = motion.VideoMotion(filename=str(tmp_path / f"{name}.avi"), capture=cap, box_size=100, threshold=12,
                                cache_time=0.3, min_time=0.1, batch=8, outdir=str(out), codec="DIB ")
        assert vm.cap.yuv_format == ("NV12" if name == "yuv" else None)
        vm.find_motion()
        runs[name] = (vm.written_indices, open(vm.outfile_name, "rb").read() if vm.wrote_frames else b"")
    assert runs["yuv"][0] and runs["yuv"][0] == runs["bgr"][0]
    assert runs["yuv"][1] == runs["bgr"][1]
