"""The content of test_gpu_pixel_content.py and test_gpu_resize_content.py, proven on the CPU oracle alone.

Every pixel case (path shape x content / threshold / alpha) runs through pixel_content.run_case without an
engine: the same frames, written backgrounds and oracle steps as on the GPU, with every condition of the case's
content asserted from the oracle's planes -- blur counts at 0 and 255, runs of 255 as long as the kernel, the four
gray residues, both sides of every tested threshold in the delta plane, .5 ties, negative and oversized background
values, and a steady frame whose mask is neither full nor empty (or exactly full / empty where that is the
design).  The resize cases' tap counts, launcher rule and .5 ties are asserted from oracle_np.area_tab and the
source sums.
"""
import numpy as np
import pytest

import oracle
import pixel_content as pc
import resize_content as rc


def test_case_table_holds_every_path():
    from test_gpu_engine_state import PATHS
    from test_gpu_pix5_loop import TALL

    assert all(pc.CASES[n] == v for n, v in PATHS.items()) and len(PATHS) == 8
    shapes = {(v[0], v[1], v[3]) for v in pc.CASES.values() if v[2] == v[0] and not v[4]}
    assert {(W, H, 5) for W, H in TALL} <= shapes          # every k_pix5 layout past the small-image path
    assert {(328, 136, 51), (200, 136, 3), (200, 136, 7)} <= shapes
    for name in pc.CASES:
        W, H, box, k, h = pc.geometry(name)
        assert pc.CASES[name][5] != "small_scan" or h * box <= 16384


def test_gray_edge_triples():
    """About a thousand triples per residue; the two rounding edges differ by one gray level."""
    tri = pc.gray_edge_triples()
    assert all(900 <= len(t) <= 1100 for t in tri), [len(t) for t in tri]
    for res, t in zip(pc.GRAY_RESIDUES, tri):
        v = (t.astype(np.int64) * [1868, 9617, 4899]).sum(-1)
        assert (v % 16384 == res).all()
        np.testing.assert_array_equal(oracle.bgr2gray(t[None])[0], (v + 8192) >> 14)


def test_dot_positions_cover_corners_edges_and_seams():
    pts = set(pc.dot_positions(136, 200))
    assert {(0, 0), (0, 199), (135, 0), (135, 199)} <= pts
    for x in (63, 64, 127, 128, 191, 192):
        assert {(0, x), (135, x), (63, x), (64, x), (127, x), (128, x)} <= pts
    for y in (63, 64, 127, 128):
        assert {(y, 0), (y, 199)} <= pts


def test_sweep_plane_values():
    p = pc.sweep_plane(72, 176, 3)
    assert set(np.unique(p[36:54])) == set(range(256)) and set(np.unique(p[18:36])) == set(pc.SWEEP_EDGE_VALUES)
    frac = p[:18] - np.floor(p[:18])
    assert (frac == 0.5).sum() >= 100 and (p < 0).any() and (p > 256).any()
    assert (p[54:, :88] == 0).all() and (p[54:, 88:] == 255).all()
    assert (pc.sweep_plane(72, 176, 3, white_second=False)[54:, :88] == 255).all()


@pytest.mark.parametrize("case", pc.pixel_cases(), ids=pc.case_id)
def test_pixel_case_conditions(case):
    m = pc.run_case(*case)
    print(f"\n{pc.case_id(case)}: {m}")


@pytest.mark.parametrize("case", rc.NT_CASES, ids=rc.case_id)
def test_resize_tap_counts(case):
    W, H, box, nt, taps = case
    assert rc.area_mode(W, H, box) == ("general", taps)
    assert (taps + 1) & ~1 == nt <= 32 and taps in (nt, nt - 1) and box >= 40


def test_resize_case_table():
    """Every instantiation NT = 2 .. 32 with NT and NT - 1 taps (NT = 2: a general-mode table has at least two
    taps), the two kernels past 32 taps, and the integer-scale shapes."""
    assert sorted({(c[3], c[4]) for c in rc.NT_CASES}) == \
        [(2, 2)] + [(nt, t) for nt in range(4, 33, 2) for t in (nt - 1, nt)]
    (W1, H1, b1), (W2, H2, b2) = rc.ROWS_CASE, rc.PLAIN_CASE
    assert rc.area_mode(W1, H1, b1)[0] == "general" and rc.area_mode(W1, H1, b1)[1] > 32 and 3 * W1 % 16 == 0
    assert rc.area_mode(W2, H2, b2)[0] == "general" and rc.area_mode(W2, H2, b2)[1] > 32 and 3 * W2 % 16 != 0
    assert [rc.area_mode(*c[:3]) for c in rc.FAST_CASES] == [("fast", c[3], c[4]) for c in rc.FAST_CASES]
    assert {(c[3], c[4]) for c in rc.FAST_CASES} == {(3, 3), (5, 5), (2, 3), (4, 4)}
    assert oracle.work_height(3, 200, 100) == 1 and (200, 3, 100, 2, 3) in rc.FAST_CASES


def test_resize_4x_noise_ties():
    W, H, box = rc.TIE_CASE
    fr = rc.frames(W, H, 0)
    assert min(rc.tie_count(fr[t, s], 4) for t in range(fr.shape[0]) for s in range(fr.shape[1])) >= 100
