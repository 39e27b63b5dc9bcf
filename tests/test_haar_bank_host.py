"""The cascade bank's C ABI and Python binding on the CPU: what fm_haar_bank_* and CascadeBank refuse
before any device call (null handles, member counts, inconsistent or oversized members, bad arguments).
The detections themselves are tests/test_gpu_haar_bank.py's.
"""
import ctypes as C

import numpy as np
import pytest

from find_motion_amd import CascadeBank, FMError, _native
from haar_cases import make_cascade


def _create(cascades):
    """fm_haar_bank_create on the descriptions -> (rc, message, size); the bank is destroyed again."""
    L = _native.load()
    descs, keep = (_native.FMHaarDesc * max(len(cascades), 1))(), []
    for i, cs in enumerate(cascades):
        descs[i], k = _native.haar_desc(cs)
        keep.append(k)
    h = C.c_void_p()
    rc = L.fm_haar_bank_create(0, descs, len(cascades), C.byref(h))
    msg, size = L.fm_haar_bank_last_error(h).decode(), L.fm_haar_bank_size(h)
    L.fm_haar_bank_destroy(h)
    return rc, msg, size


def _bad_cascades():
    """test_haar_host.py's inconsistent descriptions."""
    bad = []
    c = make_cascade(0)
    c.node_feature = c.node_feature.copy()
    c.node_feature[0] = len(c.feat_tilted)
    bad.append(c)
    c = make_cascade(0)
    c.feat_rects = c.feat_rects.copy()
    c.feat_rects[0, 0, 2] = c.win_w + 1
    bad.append(c)
    c = make_cascade(0)
    c.leaves = c.leaves[:-1]
    bad.append(c)
    c = make_cascade(0, depth=2)
    c.node_left = c.node_left.copy()
    c.node_left[1] = 5  # link out of the tree
    bad.append(c)
    c = make_cascade(0)
    c.feat_tilted = c.feat_tilted.copy()
    c.feat_tilted[0] = 1  # the full-window rect cannot be a tilted rect
    bad.append(c)
    return bad


def test_null_bank_is_refused_by_every_entry_point():
    L = _native.load()
    buf = np.zeros(64, np.int32)
    img = np.zeros((1, 40, 40, 3), np.uint8)
    p, ip = buf.ctypes.data, img.ctypes.data
    lst = (C.c_void_p * 1)(ip)
    E = _native.FM_EINVAL
    assert L.fm_haar_bank_detect(None, ip, 1, 40, 40, 3, 0, 1.1, 3, p, 1, p) == E
    assert L.fm_haar_bank_detect_frames(None, ip, 1, 40, 40, 0, 300, 1.1, 3, p, 1, p, None) == E
    assert L.fm_haar_bank_detect_frame_list(None, C.cast(lst, C.c_void_p), 1, 40, 40, 300, 1.1, 3, p, 1, p, None) == E
    assert L.fm_haar_bank_detect_frame_list_async(None, C.cast(lst, C.c_void_p), 1, 40, 40, 300, 1.1, 3, None) == E
    assert L.fm_haar_bank_collect(None, p, 1, p, 1) == E
    assert L.fm_haar_bank_candidates(None, 0, p, 1) == E
    assert L.fm_haar_bank_set_roi_upscale(None, 1) == E
    assert L.fm_haar_bank_size(None) == 0
    assert L.fm_haar_bank_last_ms(None) == 0.0
    assert L.fm_haar_bank_last_error(None)  # a fixed text, not a crash
    L.fm_haar_bank_destroy(None)
    assert L.fm_haar_bank_create(0, None, 1, None) == E


def test_a_valid_bank_passes_the_validation():
    # as fm_haar_create: on a host without a GPU a valid bank fails only at the first HIP call
    rc, msg, size = _create([make_cascade(0, tilted=True), make_cascade(1, win=(14, 28)), make_cascade(2, win=(64, 16))])
    assert rc in (_native.FM_OK, _native.FM_EHIP), msg
    assert size == (3 if rc == _native.FM_OK else 0)


@pytest.mark.parametrize("n", [0, 33])
def test_member_count_outside_1_to_32(n):
    rc, msg, size = _create([make_cascade(0)] * n)
    assert rc == _native.FM_EINVAL and "32" in msg and size == 0


def test_null_descriptions():
    L = _native.load()
    h = C.c_void_p()
    assert L.fm_haar_bank_create(0, None, 2, C.byref(h)) == _native.FM_EINVAL
    assert L.fm_haar_bank_last_error(h)
    L.fm_haar_bank_destroy(h)


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("at", [0, 2])
def test_inconsistent_member_is_named(k, at):
    members = [make_cascade(0), make_cascade(1, tilted=True), make_cascade(2)]
    members[at] = _bad_cascades()[k]
    rc, msg, size = _create(members)
    assert rc == _native.FM_EINVAL and msg.startswith(f"member {at}:") and size == 0, msg
    # the single detector's own words follow the member
    from test_haar_host import _create as create_one
    assert msg == f"member {at}: {create_one(members[at])[1]}"


def test_member_whose_patch_does_not_fit_the_tiled_sweep():
    # a 100x100 window: (30 + 101)^2 * 4 B = 68,644 B of LDS patch, beyond the tiled sweep's 56 KiB
    rc, msg, size = _create([make_cascade(0), make_cascade(1, win=(100, 100))])
    assert rc == _native.FM_ENOTSUP and msg.startswith("member 1:") and "100x100" in msg and size == 0, msg
    # 40x40 tilted: (30 + 41)^2 * 8 B = 40,328 B fits; 56x56 tilted: 60,552 B does not
    assert _create([make_cascade(1, win=(40, 40), tilted=True)])[0] in (_native.FM_OK, _native.FM_EHIP)
    rc, msg, _ = _create([make_cascade(1, win=(56, 56), tilted=True)])
    assert rc == _native.FM_ENOTSUP and msg.startswith("member 0:") and "tilted" in msg, msg
    # an inconsistent member is reported before an oversized one (validation first)
    rc, msg, _ = _create([make_cascade(1, win=(100, 100)), _bad_cascades()[0]])
    assert rc == _native.FM_EINVAL and msg.startswith("member 1:"), msg


def test_python_binding_refuses_before_any_call():
    with pytest.raises(FMError) as e:
        CascadeBank([])
    assert e.value.code == _native.FM_EINVAL
    with pytest.raises(FMError) as e:
        CascadeBank([make_cascade(0), make_cascade(1, win=(100, 100))])
    assert e.value.code == _native.FM_ENOTSUP and "member 1" in str(e.value)
    # argument checks of the methods come before the native call: a bank without a handle shows it
    bank = CascadeBank.__new__(CascadeBank)
    bank.cascades, bank._h, bank._keep = [make_cascade(0)], None, []
    with pytest.raises(ValueError):
        bank.detect_frames(np.zeros((1, 40, 40), np.uint8))  # not [n, H, W, 3]
    with pytest.raises(ValueError):
        bank.detect_batch(np.zeros((1, 40, 40, 4), np.uint8))
    with pytest.raises(IndexError):
        bank.candidates(1)

    class FakeDeviceTensor:  # what detect_frames reads of a torch tensor
        is_cuda, dtype, shape = True, None, (1, 40, 40, 3)

        def dim(self):
            return 4

        def is_contiguous(self):
            return False

    import torch
    t = FakeDeviceTensor()
    t.dtype = torch.uint8
    with pytest.raises(ValueError, match="contiguous"):
        bank.detect_frames(t)
