"""GPU: every INTER_AREA kernel variant on noise, white and checkerboard frames, byte for byte against the oracle.

The PLANE_SMALL bytes of every frame of every stream are compared with oracle.resize_area_bgr: S = 2, T = 2, two
batches, so the batch's last frame ends the input buffer and the last columns' windows run past it.  The shapes
and their tap counts come from resize_content.py; test_pixel_content_host.py asserts them from
oracle_np.area_tab without a GPU.

k_resize_area_nt<NT> is instantiated for NT = 2, 4, ..., 32 and loads 3 NT tap bytes per row as b128 loads plus
a tail chosen by NR = ((3 NT + 3) / 4 + 1) % 4.  NT = 10, 16, 26 and 32 are the NR == 1 cases (one
raw_buffer_load_b32), which no earlier test ran; earlier tests ran NT = 2, 6, 8, 14 and 22 only.  Here every NT
runs with NT taps and with NT - 1 (the zero-padded weight in use), at a destination 40 px wide, so a row of
threads meets every byte misalignment and the window-past-the-frame branch.  The tail dword holds bytes of the
last of NT taps only (and only at a 3-byte misalignment), so the source widths are odd (every row shifts the
alignment) and chosen so that the end taps cover half a source pixel: with that tail load moved by one dword
all four NR == 1 cases fail, where at the narrowest width with the same tap count (end taps of 0.025 px) NT = 26
still passed.
"""
import numpy as np
import pytest

import oracle
import resize_content as rc
from find_motion_amd import MotionEngine
from find_motion_amd._native import PLANE_SMALL

pytestmark = pytest.mark.gpu


def _compare(W, H, box):
    eng = MotionEngine(n_streams=rc.S, src_w=W, src_h=H, box_size=box, ksize=5, threshold=12, avg=0.1,
                       max_batch=rc.T)
    try:
        assert eng.work_shape == (oracle.work_height(H, W, box), box)
        for b in range(rc.NB):
            fr = rc.frames(W, H, b)
            eng.submit(fr)
            eng.wait()
            for t in range(rc.T):
                for s in range(rc.S):
                    got, ref = eng.plane(PLANE_SMALL, t, s), oracle.resize_area_bgr(fr[t, s], box)
                    bad = np.argwhere(got != ref)
                    assert len(bad) == 0, f"{W} x {H} -> {box}: batch {b} frame {t} stream {s}: {len(bad)} bytes " \
                                          f"differ, first (y, x, c) {bad[:8].tolist()}"
    finally:
        eng.close()


@pytest.mark.parametrize("case", rc.NT_CASES, ids=rc.case_id)
def test_register_kernel_every_instantiation(case):
    """k_resize_area_nt<NT> with NT and NT - 1 taps.  NT = 10, 16, 26, 32: the NR == 1 tail."""
    W, H, box, nt, taps = case
    assert rc.area_mode(W, H, box) == ("general", taps) and (taps + 1) & ~1 == nt <= 32
    _compare(W, H, box)


@pytest.mark.parametrize("case", [rc.ROWS_CASE, rc.PLAIN_CASE], ids=["rows", "plain"])
def test_past_32_taps(case):
    """k_resize_area_rows (3 W % 16 == 0) and k_resize_area (3 W % 16 != 0)."""
    W, H, box = case
    mode = rc.area_mode(W, H, box)
    assert mode[0] == "general" and mode[1] > 32 and (3 * W % 16 == 0) == (case == rc.ROWS_CASE)
    _compare(W, H, box)


@pytest.mark.parametrize("case", rc.FAST_CASES, ids=rc.case_id)
def test_integer_scale_kernel(case):
    """k_resize_area_fast at 3 x 3, 5 x 5, the non-square 2 x 3 (the float branch, not (sum + 2) >> 2) and 4 x 4
    on noise, where at least 100 outputs per frame sit on an exact .5 tie (rounded to even)."""
    W, H, box, sx, sy = case
    assert rc.area_mode(W, H, box) == ("fast", sx, sy)
    if case[:3] == rc.TIE_CASE:
        fr = rc.frames(W, H, 0)
        assert min(rc.tie_count(fr[t, s], 4) for t in range(rc.T) for s in range(rc.S)) >= 100
    _compare(W, H, box)
