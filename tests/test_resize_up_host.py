"""INTER_AREA towards a larger image (a box wider than the frame) on a machine without a GPU: the numpy
restatement's known answers, the library's tap tables against it, and the opt-in (FM_FLAG_AREA_UPSCALE): without
the flag every entry point refuses such a box exactly as before.

The rule is restated from knowledge of OpenCV's resize.cpp (resize_up_ref.py); parity to cv2 itself is not pinned."""
import ctypes as C

import numpy as np
import pytest

import resize_up_ref as ru
from find_motion_amd import _native, work_height
from find_motion_amd._native import (FM_ENOTSUP, FM_FLAG_AREA_UPSCALE, FM_OK, RESIZE_FAST, RESIZE_GENERAL,
                                     RESIZE_IDENTITY, RESIZE_UP, FMError)

AXES = [(1920, 1921), (200, 300), (1280, 1920), (160, 300), (101, 300), (299, 300), (1, 5), (2, 3)]
# every (W, H, box) of test_gpu_resize_up.py
GEOMETRIES = [(1, 1, 5), (7, 5, 14), (64, 48, 128), (200, 113, 300), (101, 40, 300), (299, 168, 300),
              (1920, 1080, 1921), (1280, 720, 1920), (48, 36, 100), (640, 360, 1088), (160, 120, 300), (128, 96, 256)]
MSG = "INTER_AREA upscaling is bilinear in OpenCV, not supported"


def _params(W, H, box, k=5, flags=0):
    return _native.FMParams(0, 1, W, H, box, k, 12, 0.1, 1, 16, flags)


# --- the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3])
def test_integer_factor_replicates(n):
    img = np.random.default_rng(n).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    got = ru.resize_area_up_u8(img, 7 * n, 5 * n)
    assert np.array_equal(got, np.repeat(np.repeat(img, n, axis=0), n, axis=1))


def test_two_to_three_and_four_to_five():
    s0, s1, a0, a1 = ru.area_up_taps(2, 3)
    assert s0.tolist() == [0, 0, 1] and s1.tolist() == [1, 1, 1]
    assert a0.tolist() == [2048, 1024, 2048] and a1.tolist() == [0, 1024, 0]
    row = np.array([[[10], [20]]], np.uint8)
    assert ru.resize_area_up_u8(row, 3, 1)[0, :, 0].tolist() == [10, 15, 20]
    assert ru.area_up_taps(4, 5)[3].tolist() == [0, 1536, 1024, 512, 0]


@pytest.mark.parametrize("ssize,dsize", AXES[:7])
def test_taps_are_a_partition_and_monotone(ssize, dsize):
    s0, s1, a0, a1 = ru.area_up_taps(ssize, dsize)
    assert np.all(a0 + a1 == 2048) and np.all(a1 >= 0) and np.all(a0 >= 0)
    assert s0[0] == 0 and np.all(np.diff(s0) >= 0) and np.all(np.diff(s0) <= 1)
    assert np.array_equal(s1, np.minimum(s0 + 1, ssize - 1)) and s0.max() == ssize - 1
    for v in (0, 255, 77):
        img = np.full((1, ssize, 3), v, np.uint8)
        assert np.all(ru.resize_area_up_u8(img, dsize, 1 if dsize != ssize else 2) == v)


def test_equal_height_is_an_identity_axis():
    assert ru.up_height(1080, 1920, 1921) == 1080
    s0, s1, a0, a1 = ru.area_up_taps(1080, 1080)
    assert s0.tolist() == list(range(1080)) and not a1.any()
    img = np.random.default_rng(0).integers(0, 256, (6, 4, 3), dtype=np.uint8)
    got = ru.resize_area_up_u8(img, 8, 6)
    assert np.array_equal(got, np.repeat(img, 2, axis=1))


@pytest.mark.parametrize("W,H,box", GEOMETRIES)
def test_work_height_of_every_geometry(W, H, box):
    h = ru.up_height(H, W, box)
    assert h == int(H * box / W) == work_height(H, W, box) and h >= H
    out = _native.plan(src_w=W, src_h=H, box_size=box, ksize=5, area_upscale=True)
    assert out["work_shape"] == (h, box)


# --- the library's tables -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ssize,dsize", AXES)
def test_library_taps_equal_the_restatement(ssize, dsize):
    got = _native.area_up_taps(ssize, dsize)
    want = ru.area_up_taps(ssize, dsize)
    for g, w, name in zip(got, want, ("s0", "s1", "a0", "a1")):
        assert np.array_equal(g, w), name


def test_library_taps_refuse_a_shrinking_axis():
    with pytest.raises(FMError) as e:
        _native.area_up_taps(300, 200)
    assert e.value.code == _native.FM_EINVAL


# --- the opt-in ---------------------------------------------------------------------------------------------------

def test_resize_kind_is_up_only_with_the_flag():
    kw = dict(src_h=48, ksize=5)
    assert _native.resize_kind(src_w=64, box_size=128, area_upscale=True, **kw) == RESIZE_UP
    assert _native.resize_kind(src_w=64, box_size=64, area_upscale=True, **kw) == RESIZE_IDENTITY
    assert _native.resize_kind(src_w=64, box_size=64, **kw) == RESIZE_IDENTITY
    assert _native.resize_kind(src_w=64, box_size=32, area_upscale=True, **kw) == RESIZE_FAST
    assert _native.resize_kind(src_w=64, box_size=32, **kw) == RESIZE_FAST
    assert _native.resize_kind(src_w=64, box_size=50, area_upscale=True, **kw) == RESIZE_GENERAL
    assert _native.resize_kind(src_w=64, box_size=50, **kw) == RESIZE_GENERAL
    assert _native.resize_kind(src_w=1920, src_h=1080, box_size=1921, ksize=5, area_upscale=True) == RESIZE_UP
    assert _native.engine_flags(area_upscale=True) == FM_FLAG_AREA_UPSCALE == 0x20
    assert _native.engine_flags() == 0


def test_without_the_flag_the_refusal_stands():
    L = _native.load()
    p = _params(64, 48, 128)
    out, kind, h = _native.FMPlan(), C.c_int32(-7), C.c_void_p()
    assert L.fm_plan(C.byref(p), C.byref(out)) == FM_ENOTSUP
    assert MSG in L.fm_last_error(None).decode() and "box_size 128 > frame width 64" in L.fm_last_error(None).decode()
    assert (out.work_h, out.work_w, out.tiles, out.pixel_path) == (0, 0, 0, b"")
    assert L.fm_create(C.byref(h), C.byref(p)) == FM_ENOTSUP and not h.value
    assert MSG in L.fm_last_error(None).decode()
    assert L.fm_resize_kind(C.byref(p), C.byref(kind)) == FM_ENOTSUP and kind.value == -7
    assert MSG in L.fm_last_error(None).decode()
    for fn in (_native.plan, _native.resize_kind):
        with pytest.raises(FMError) as e:
            fn(src_w=64, src_h=48, box_size=128, ksize=5)
        assert e.value.code == FM_ENOTSUP and MSG in str(e.value)


def test_with_the_flag_the_plan_is_that_of_the_enlarged_frame():
    L = _native.load()
    p = _params(64, 48, 128, flags=FM_FLAG_AREA_UPSCALE)
    out = _native.FMPlan()
    assert L.fm_plan(C.byref(p), C.byref(out)) == FM_OK, L.fm_last_error(None)
    assert (out.work_h, out.work_w) == (96, 128)
    for k, keep in ((5, False), (5, True), (11, False), (51, False)):
        up = _native.plan(src_w=64, src_h=48, box_size=128, ksize=k, keep_planes=keep, area_upscale=True)
        same = _native.plan(src_w=128, src_h=96, box_size=128, ksize=k, keep_planes=keep)
        assert up == same and up["work_shape"] == (96, 128)
    wide = _native.plan(src_w=640, src_h=360, box_size=1088, ksize=51, area_upscale=True)
    assert wide["pixel_path"] == "wide" and wide["tiles"] > 16
    # the same validation as ever
    kind = C.c_int32()
    assert L.fm_resize_kind(None, C.byref(kind)) == _native.FM_EINVAL
    assert L.fm_resize_kind(C.byref(p), None) == _native.FM_EINVAL
    bad = _params(64, 48, 128, k=4, flags=FM_FLAG_AREA_UPSCALE)
    assert L.fm_resize_kind(C.byref(bad), C.byref(kind)) == _native.FM_EINVAL
