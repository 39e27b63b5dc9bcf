"""A refused fm_create gives back what it took.

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
