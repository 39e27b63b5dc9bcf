"""Retained source frames on the GPU (fm_retain_reserve / fm_retain_frames / fm_release_frames / fm_read_retained,
k_retain_frames in fm_kernels.hip) through MotionEngine: frames of a waited batch copied into the context's pool
stay readable, and encodable where they lie, after every batch slot has been overwritten.

Every comparison is byte for byte.  The frame shapes separate the copy kernel's paths: a slot frame starts at
(t * S + s) * frame_bytes, so an odd frame size puts every frame but (0, 0) at another alignment (the dword path and
the byte tail), a multiple of 16 keeps them all on the 16-byte path, 3 bytes is a tail only, and 320 x 240 takes
many workgroups per frame.
"""
import numpy as np
import pytest

import jpeg_cases as jc
from find_motion_amd import MJpegDecoder, MJpegEncoder, MotionEngine
from find_motion_amd._native import FM_EINVAL, FM_ENOMEM, FM_ESTATE, FMError

pytestmark = pytest.mark.gpu

# (W, H, box of the resize mode): 3 B; 1,281 B and 1,005 B (odd); 240 B and 1,536 B (multiples of 16); 230,400 B
SHAPES = [(1, 1, None), (61, 7, 30), (67, 5, 33), (20, 4, 10), (64, 8, 32), (320, 240, 100)]
CASES = [(W, H, box, S, T) for W, H, rbox in SHAPES for box in ([W] if rbox is None else [W, rbox])
         for S in (1, 2) for T in (1, 3, 8)]


def engine(W, H, S, T, box=None, **kw):
    return MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=box or W, ksize=1, threshold=12, avg=0.1, max_batch=T,
                        **kw)


def subset(T, S):
    """Pairs to retain: the first and last frame of each stream, a middle one, and one pair twice."""
    pairs = [(t, s) for s in range(S) for t in sorted({0, T // 2, T - 1})]
    return pairs + [pairs[-1]]


def overwrite_every_slot(eng, other):
    """max_inflight + 1 further batches of other content: every batch slot has been written again."""
    for _ in range(eng.max_inflight + 1):
        eng.submit(other)
        eng.wait()


def frames_of(rng, T, S, H, W):
    return rng.integers(0, 256, (T, S, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("W,H,box,S,T", CASES)
def test_round_trip(W, H, box, S, T):
    rng = np.random.default_rng(W * 1000 + H * 10 + S + T)
    frames, other = frames_of(rng, T, S, H, W), frames_of(rng, T, S, H, W)
    with engine(W, H, S, T, box) as eng:
        pairs = subset(T, S)
        eng.reserve_retained(len(pairs))
        assert eng.retained == (0, len(pairs))
        eng.submit(frames)
        eng.wait()
        ptrs = eng.retain(pairs)
        assert len(set(ptrs)) == len(pairs) and all(p % 256 == 0 for p in ptrs)  # a pair named twice: two copies
        assert eng.retained == (len(pairs), len(pairs))
        overwrite_every_slot(eng, other)
        for p, (t, s) in zip(ptrs, pairs):
            np.testing.assert_array_equal(eng.read_retained(p), frames[t, s], err_msg=f"pair {(t, s)}")
        eng.release(ptrs)
        assert eng.retained == (0, len(pairs))


@pytest.mark.parametrize("W,H", [(1, 1), (61, 7), (64, 8), (320, 240)])
def test_retained_frames_encode_where_they_lie(W, H):
    S, T = 2, 3
    rng = np.random.default_rng(W + H)
    frames = np.stack([jc.image(H, W, "smooth", s) for s in range(T * S)]).reshape(T, S, H, W, 3)
    with engine(W, H, S, T) as eng:
        pairs = [(t, s) for t in range(T) for s in range(S)]
        eng.reserve_retained(len(pairs))
        eng.submit(frames)
        eng.wait()
        ptrs = eng.retain(pairs)
        overwrite_every_slot(eng, frames_of(rng, T, S, H, W))
        enc = MJpegEncoder(W, H, max_frames=len(pairs))
        assert enc.encode_device(ptrs) == enc.encode(frames.reshape(T * S, H, W, 3))
        enc.close()
        eng.release(ptrs)


@pytest.mark.parametrize("W,H", [(61, 7), (64, 8)])
def test_round_trip_of_a_device_batch(W, H):
    """fm_submit(on_device = 1): the frames are read from the caller's buffer -- here a torch tensor that starts one
    byte into its allocation, so that no frame of it is aligned."""
    torch = pytest.importorskip("torch")
    S, T = 2, 3
    rng = np.random.default_rng(5)
    frames = frames_of(rng, T, S, H, W)
    big = torch.zeros(frames.size + 16, dtype=torch.uint8, device="cuda")
    dev = big[1:1 + frames.size]
    dev.copy_(torch.from_numpy(frames.reshape(-1)))
    torch.cuda.synchronize()
    with engine(W, H, S, T) as eng:
        pairs = subset(T, S)
        eng.reserve_retained(len(pairs))
        eng.submit_device(dev.data_ptr(), T)
        eng.wait()
        ptrs = eng.retain(pairs)
        dev.zero_()  # the caller's buffer is the "slot" of such a batch
        torch.cuda.synchronize()
        overwrite_every_slot(eng, frames_of(rng, T, S, H, W))
        for p, (t, s) in zip(ptrs, pairs):
            np.testing.assert_array_equal(eng.read_retained(p), frames[t, s], err_msg=f"pair {(t, s)}")
        eng.release(ptrs)


@pytest.mark.parametrize("fmt", ["NV12", "YUY2"])
def test_round_trip_of_a_yuv_batch(fmt):
    W, H, S, T = 34, 18, 2, 3
    rng = np.random.default_rng(6)
    size = W * H * 3 // 2 if fmt == "NV12" else W * H * 2
    yuv = rng.integers(0, 256, (T, S, size), dtype=np.uint8)
    with engine(W, H, S, T) as eng:
        pairs = subset(T, S)
        eng.reserve_retained(len(pairs))
        eng.submit_yuv(yuv, fmt)
        eng.wait()
        want = [eng.read_frame(t, s) for t, s in pairs]  # the converted frames, while the batch is current
        ptrs = eng.retain(pairs)
        overwrite_every_slot(eng, frames_of(rng, T, S, H, W))
        for p, w, pair in zip(ptrs, want, pairs):
            np.testing.assert_array_equal(eng.read_retained(p), w, err_msg=f"pair {pair}")
        eng.release(ptrs)


def test_round_trip_of_a_jpeg_batch():
    W, H, S, T = 53, 37, 2, 3
    rng = np.random.default_rng(7)
    jpegs = [jc.encode(jc.image(H, W, "smooth", i), quality=80) for i in range(T * S)]
    dec = MJpegDecoder(W, H, max_frames=T * S)
    with engine(W, H, S, T) as eng:
        pairs = subset(T, S)
        eng.reserve_retained(len(pairs))
        eng.submit_jpeg(dec, jpegs)
        eng.wait()
        ptrs = eng.retain(pairs)
        overwrite_every_slot(eng, frames_of(rng, T, S, H, W))
        for p, (t, s) in zip(ptrs, pairs):
            np.testing.assert_array_equal(eng.read_retained(p), jc.reference_decode(jpegs[t * S + s]),
                                          err_msg=f"pair {(t, s)}")
        eng.release(ptrs)
    dec.close()


# --- refusals ------------------------------------------------------------------------------------------------------

def code_of(call, *a):
    with pytest.raises(FMError) as e:
        call(*a)
    return e.value.code


def test_refusals_leave_the_pool_as_it_was():
    W, H, S, T = 67, 5, 2, 3
    rng = np.random.default_rng(8)
    frames = frames_of(rng, T, S, H, W)
    with engine(W, H, S, T) as eng:
        assert eng.retained == (0, 0)
        eng.retain([])  # n = 0: nothing to do, whatever the state
        eng.release([])
        assert code_of(eng.reserve_retained, -1) == FM_EINVAL
        eng.reserve_retained(3)
        assert code_of(eng.retain, [(0, 0)]) == FM_ESTATE  # no batch waited
        eng.submit(frames)
        assert code_of(eng.retain, [(0, 0)]) == FM_ESTATE  # submitted, not waited
        eng.wait()
        with pytest.raises(FMError, match=r"pair 1: \(frame 3, stream 0\)") as e:  # out of range: named, nothing copied
            eng.retain([(0, 0), (T, 0)])
        assert e.value.code == FM_EINVAL
        assert code_of(eng.retain, [(0, S)]) == FM_EINVAL and code_of(eng.retain, [(-1, 0)]) == FM_EINVAL
        assert eng.retained == (0, 3)
        first = eng.retain([(0, 0), (2, 1)])
        # pool exhausted: capacity 3, two in use, a request for two more (and one for four) copies nothing
        assert code_of(eng.retain, [(1, 0), (1, 1)]) == FM_ENOMEM
        assert code_of(eng.retain, [(0, 0)] * 4) == FM_ENOMEM
        assert eng.retained == (2, 3)
        np.testing.assert_array_equal(eng.read_retained(first[0]), frames[0, 0])
        np.testing.assert_array_equal(eng.read_retained(first[1]), frames[2, 1])
        # reserve while entries are in use
        assert code_of(eng.reserve_retained, 8) == FM_ESTATE and code_of(eng.reserve_retained, 0) == FM_ESTATE
        # bad releases: a foreign address, an address inside an entry, a double release -- nothing is released
        assert code_of(eng.release, [first[0], 0x1000]) == FM_EINVAL
        assert code_of(eng.release, [first[0] + 16]) == FM_EINVAL
        assert code_of(eng.release, [first[0], first[1], first[0]]) == FM_EINVAL
        assert eng.retained == (2, 3)
        eng.release([first[0]])
        assert code_of(eng.release, [first[0]]) == FM_EINVAL and code_of(eng.read_retained, first[0]) == FM_EINVAL
        assert code_of(eng.release, [first[1], first[0]]) == FM_EINVAL
        assert eng.retained == (1, 3)
        more = eng.retain([(1, 0), (1, 1)])  # after the release the request succeeds
        np.testing.assert_array_equal(eng.read_retained(more[0]), frames[1, 0])
        np.testing.assert_array_equal(eng.read_retained(more[1]), frames[1, 1])
        np.testing.assert_array_equal(eng.read_retained(first[1]), frames[2, 1])
        eng.release(more + [first[1]])
        # re-reserve, larger and smaller, after releasing everything
        eng.reserve_retained(5)
        assert eng.retained == (0, 5)
        got = eng.retain([(t, s) for t in range(T) for s in range(S)][:5])
        np.testing.assert_array_equal(eng.read_retained(got[4]), frames[2, 0])
        eng.release(got)
        eng.reserve_retained(0)
        assert eng.retained == (0, 0) and code_of(eng.retain, [(0, 0)]) == FM_ENOMEM


def test_the_pool_counts_in_the_footprint():
    """Device memory grows by the entries -- each frame_bytes rounded up to its 256-byte alignment -- and by the call's
    table of copies, 16 bytes (two addresses) per entry; page-locked memory by that table's staging."""
    W, H, cap = 61, 7, 5
    fb = W * H * 3
    with engine(W, H, 1, 2) as eng:
        before = eng.footprint()
        eng.reserve_retained(cap)
        after = eng.footprint()
        grown = after["device_bytes"] - before["device_bytes"]
        assert cap * fb <= grown - cap * 16 <= cap * (fb + 255)
        assert grown - cap * 16 == cap * ((fb + 255) // 256 * 256)
        assert after["pinned_bytes"] - before["pinned_bytes"] == cap * 16
        eng.reserve_retained(0)
        assert eng.footprint() == before
