"""The Gaussian-size sweep of test_gpu_ksize_sweep.py, proven without a GPU.

  taps        the library's own gaussian_taps (fm_gaussian_taps; make_geo trims the wide path's geometry by it)
              equals the oracle's at every odd k from 1 to 255, sums to 256 and is symmetric; the refusals return
              their code and leave the output alone
  plan        fm_plan gives the path every sweep case stands for, among them both sides of the small path's LDS
              limit at 113 x 114 (k 27 | 29) and of its size limit at 100 x 56 (k 49 | 51)
  conditions  every case of both lists runs through ksize_sweep.run on the oracle alone and meets the conditions
              of its content: the GPU module's inputs reach what they are for
"""
import ctypes as C

import numpy as np
import pytest

import ksize_sweep as ks
import oracle
from find_motion_amd import _native
from find_motion_amd._native import FM_EINVAL, FM_OK, FMError

LIGHT, FULL = ks.light_cases(), ks.full_cases()


@pytest.mark.parametrize("k", range(1, 256, 2))
def test_library_taps_equal_the_oracles(k):
    got = _native.gaussian_taps(k)
    assert got.dtype == np.int32 and got.shape == (k,)
    np.testing.assert_array_equal(got, np.asarray(oracle.gauss_coeffs(k)).astype(np.int64))
    assert int(got.sum()) == 256
    np.testing.assert_array_equal(got, got[::-1])


@pytest.mark.parametrize("k", (0, -1, -3, 2, 4, 50, 254, 256, 257, 1 << 20))
def test_library_taps_refuse_other_sizes(k):
    L = _native.load()
    out = np.full(1024, -77, np.int32)
    assert L.fm_gaussian_taps(k, out.ctypes.data) == FM_EINVAL
    assert (out == -77).all()
    assert str(k) in L.fm_last_error(None).decode()
    with pytest.raises(FMError) as e:
        _native.gaussian_taps(k)
    assert e.value.code == FM_EINVAL


def test_library_taps_refuse_a_null_pointer_and_write_ksize_values_only():
    L = _native.load()
    assert L.fm_gaussian_taps(5, None) == FM_EINVAL
    assert "fm_gaussian_taps" in _native.EXPORTED and L.fm_abi_version() == 1
    out = np.full(300, -77, np.int32)
    assert L.fm_gaussian_taps(255, out.ctypes.data) == FM_OK
    assert (out[255:] == -77).all() and int(out[:255].sum()) == 256 and (out[:255] >= 0).all()


def test_case_lists_hold_what_they_name():
    assert len(LIGHT) == 25 + 25 + 103 + 14 and len(set(LIGHT)) == len(LIGHT)
    assert len(FULL) == 3 * (7 + 5 + 5 + 3 + 2 + 3 + 4 + 2) and len(set(FULL)) == len(FULL)
    by_path = {}
    for W, H, k, planes, path, launch in LIGHT:
        by_path.setdefault((path, W, H), []).append(k)
    assert by_path[("small", 100, 56)] == list(range(1, 50, 2))
    assert sorted(by_path[("fused", 200, 136)] + by_path[("pix", 200, 136)]) == list(range(1, 50, 2))
    assert by_path[("pix", 200, 136)] == [3, 5, 7, 21]
    assert by_path[("wide", 328, 136)] == list(range(51, 256, 2))
    assert by_path[("pixel", 256, 200)] == by_path[("pixel", 100, 56)] == [51, 53, 99, 155, 157, 253, 255]
    # a radius past the image: the kernel reaches over more than the whole short axis, so REFLECT_101 folds twice
    past = [c for c, content in FULL if content == "noise" and c[2] // 2 > min(c[0], c[1]) - 1]
    assert {(c[4], c[2]) for c in past} >= {("pix", 21), ("fused", 49), ("wide", 255), ("pixel", 255)}
    # ... and the shapes where it folds once but reaches most of the axis (r 3 on 8 columns, r 11 on 20)
    assert {(8, 2056, 7), (12, 1400, 21), (20, 900, 23), (900, 20, 23)} <= {c[:3] for c, _ in FULL}


def _plan(W, H, k, planes=False):
    return _native.plan(src_w=W, src_h=H, box_size=W, ksize=k, keep_planes=planes)["pixel_path"]


@pytest.mark.parametrize("case", sorted(set(LIGHT) | {c for c, _ in FULL}), ids=ks.case_id)
def test_plan_gives_the_path_of_every_case(case):
    W, H, k, planes, path, launch = case
    assert _plan(W, H, k, planes) == path
    assert launch == ks.LAUNCH[path]
    # profile="pix", which the GPU module sets to read the launch names, does not move the selection
    assert _native.plan(src_w=W, src_h=H, box_size=W, ksize=k, keep_planes=planes, profile="pix")["pixel_path"] == path


def test_plan_edges_in_k():
    assert (_plan(113, 114, 27), _plan(113, 114, 29)) == ("small", "fused")
    assert (_plan(100, 56, 49), _plan(100, 56, 51)) == ("small", "pixel")
    assert [_plan(100, 56, k) for k in range(51, 256, 2)] == ["pixel"] * 103  # the small path takes k <= 49 only
    for k in range(1, 50, 2):
        assert _plan(200, 136, k) == ("pix" if k in (3, 5, 7, 21) else "fused"), k
        assert _plan(200, 136, k, True) == ("pix" if k in (3, 5, 7, 21) else "fused"), k
    for k in range(51, 256, 2):
        assert _plan(200, 136, k) == "pixel" and _plan(328, 136, k) == "wide" and _plan(328, 136, k, True) == "pixel", k
        assert _plan(256, 200, k) == "pixel", k  # 16 tiles


@pytest.mark.parametrize("case", LIGHT, ids=ks.case_id)
def test_light_case_conditions(case):
    m = ks.run(case, "patches", light=True)
    print(f"\n{ks.case_id(case)}: fractions {m['fractions']} blur span {m['blur_span']}")


@pytest.mark.parametrize("item", FULL, ids=ks.full_id)
def test_full_case_conditions(item):
    m = ks.run(item[0], item[1], light=False)
    print(f"\n{ks.full_id(item)}: {m}")
