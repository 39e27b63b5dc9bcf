"""A refused fm_create gives back what it took, and so does closing each of the other device objects.

fm_create validates some of its parameters only after its first allocations (the 32-bit node-id limit
of the contour pass is known once the tile grid is).  The context's destructor releases the streams
and buffers taken by then; before it existed every such refusal leaked them.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from find_motion_amd import MotionEngine, _native
from find_motion_amd.synthetic import batch

pytestmark = pytest.mark.gpu

CALLS = 128
BOX = 512
# device memory a refused call holds when the refusal arrives: the two f64 background planes alone
BG_BYTES = 2 * BOX * BOX * 8


def test_refused_create_releases_device_memory():
    torch = pytest.importorskip("torch")
    L = _native.load()
    # 700 000 frames x 64 tiles x 49 node slots > 2^31: refused after six streams, the background
    # planes, the keep plane and the mask plane exist; nothing large is ever requested
    p = _native.FMParams(0, 1, BOX, BOX, BOX, 5, 12, 0.1, 700000, 16, 0)
    def refused():
        h = C.c_void_p()
        assert L.fm_create(C.byref(h), C.byref(p)) == _native.FM_ENOTSUP
        assert not h.value
        assert b"32-bit node ids" in L.fm_last_error(None)

    refused()  # (the library's first device call loads its code objects: some 160 MB, once per process)
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(CALLS):
        refused()
    lost = free0 - torch.cuda.mem_get_info()[0]
    leak = CALLS * BG_BYTES                      # 512 MiB at the least, were nothing released
    print(f"free device memory fell by {lost} bytes over {CALLS} refused calls (a leak loses >= {leak})")
    assert lost < leak // 2

    _engine_batch_is_exact()


def _engine_batch_is_exact():
    # the device is still usable: one small batch, bit-for-bit against the oracle
    W, H, k = 320, 240, 5
    eng = MotionEngine(n_streams=2, src_w=W, src_h=H, box_size=W, ksize=k, threshold=12, avg=0.1, max_batch=4)
    cfg = oracle.OracleConfig(H=H, W=W, box=W, ksize=k)
    orc = [oracle.OracleStream(cfg), oracle.OracleStream(cfg)]
    fr = batch(W, H, 2, 0, 4)
    eng.submit(fr)
    eng.wait()
    counts = eng.counts()
    for t in range(4):
        for s in range(2):
            ref = orc[s].step(fr[t, s])
            np.testing.assert_array_equal(eng.mask(t, s), ref["mask"])
            assert counts[t, s] == ref["count"]
            assert [c.bbox for c in eng.contours(t, s)] == ref["boxes"]
    eng.close()


CYCLES = 32


def _haar_cycle():
    """(one create -> detect_frames -> close of a CascadeClassifier at 640x360, the bytes it certainly allocates)"""
    from find_motion_amd import CascadeClassifier
    from haar_cases import make_cascade, make_image
    cs = make_cascade(1, tight=0.38, depth=2, tilted=True)
    W, H, n, rw = 640, 360, 3, 300
    small = make_image(0, w=300, h=169)
    raw = np.ascontiguousarray(small[(np.arange(H) * 169) // H][:, (np.arange(W) * 300) // W])
    raws = np.stack([raw] * n)
    rh = int(H * (rw / W))

    def cycle():
        det = CascadeClassifier(cs)
        got = det.detect_frames(raws, rw, 1.1, 3)
        det.close()
        return [g.tolist() for g in got]
    # the ROI frames, and the sum and squared-sum integrals of the first pyramid level alone (u32 each)
    return cycle, n * rh * rw * 3 + 2 * n * (rh + 1) * (rw + 1) * 4


def _jpeg_420_blocks(W, H):
    return -(-W // 16) * -(-H // 16) * 6


def _decoder_cycle():
    from find_motion_amd import MJpegDecoder, MJpegEncoder
    from find_motion_amd.synthetic import batch
    W, H, F = 640, 480, 8
    enc = MJpegEncoder(W, H, max_frames=1)  # (4:2:0, as the decoder's layout below)
    jpegs = enc.encode(batch(W, H, 1, 0, 1)[0, 0])
    enc.close()

    def cycle():
        dec = MJpegDecoder(W, H, max_frames=F)
        out = dec.decode(jpegs)
        dec.close()
        return out.tobytes()
    return cycle, 2 * F * _jpeg_420_blocks(W, H) * 64 * 2  # the two sets' s16 coefficients


def _encoder_cycle():
    from find_motion_amd import MJpegEncoder
    from find_motion_amd.synthetic import batch
    W, H, F = 640, 480, 8
    frame = batch(W, H, 1, 0, 1)[0, 0]

    def cycle():
        enc = MJpegEncoder(W, H, max_frames=F)
        out = enc.encode(frame)
        enc.close()
        return out
    return cycle, F * _jpeg_420_blocks(W, H) * 64 * 2  # the s16 coefficients


def _yolo_cycle():
    import yolo_ref as yr
    from find_motion_amd import YoloDetector
    from find_motion_amd import darknet as dk
    net, F = 64, 2
    _, layers = dk.parse_cfg(yr.net_cfg(3, [yr.conv_cfg(4, 1, 1, "linear", bn=0)], net, net))
    params = dk.load_weights(dk.write_weights(layers, yr.random_raw(layers, 0)), layers)
    frames = yr.make_frames(F, 640, 480, seed=1)

    def cycle():
        det = YoloDetector(layers, params, yr.MINI_CLASSES, net_w=net, net_h=net, max_frames=F)
        det.candidates(frames)
        out = det.layer_output(-1, F)
        det.close()
        return out.tobytes()
    return cycle, F * 3 * net * net * 4  # the f32 blob


@pytest.mark.parametrize("make", [_haar_cycle, _decoder_cycle, _encoder_cycle, _yolo_cycle],
                         ids=["haar", "mjpeg", "mjpeg_enc", "yolo"])
def test_create_call_close_releases_device_memory(make):
    """create -> one small call -> close, CYCLES times: every cycle computes what the first did, and free device
    memory falls by less than half of what the cycles' certain allocations add up to (the rule of the
    refused-create test above; an object that kept its buffers would lose all of it)."""
    torch = pytest.importorskip("torch")
    cycle, certain = make()
    first = cycle()  # (untimed: the library's first device call loads its code objects, once per process)
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(CYCLES):
        assert cycle() == first
    lost = free0 - torch.cuda.mem_get_info()[0]
    leak = CYCLES * certain
    print(f"free device memory fell by {lost} bytes over {CYCLES} cycles (a leak loses >= {leak})")
    assert lost < leak // 2
    _engine_batch_is_exact()
