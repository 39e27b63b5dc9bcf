"""GPU parity of the object-ROI stage on full-range content and at every tie (tests/haar_content.py) against
oracle/haar.py: candidates exactly and in order at minNeighbors 0, grouped rectangles exactly at minNeighbors 3
for every list of at most haar_content.GROUP_CAP candidates (groupRectangles' partition is quadratic; the probes'
lists of 3,000 to 26,000 candidates are compared ungrouped only),
through the tiled sweep (k_hdetect), the global-memory sweep (k_heval / k_heval_tail) and the cascade bank
(k_bdetect), which each carry their own copy of setWindow and of the stage loop.

test_haar_content_host.py proves without a GPU that every case sits on its edge and that a kernel which keeps
1 / sqrt(nf) in double, reads the squared sum as signed, saturates the integrals, compares with `<=` at a node or at
a stage, drops a rounding term of the gray conversion or of the resize, or contracts the feature sum would give
other candidates on a case run here.
"""
import numpy as np
import pytest

import haar_content as hc
import oracle
import pixel_content
from find_motion_amd import CascadeBank, CascadeClassifier
from oracle import haar

pytestmark = pytest.mark.gpu


def _rects(a):
    return [tuple(r) for r in np.asarray(a).reshape(-1, 4).tolist()]


def _stack(names, channels):
    return np.stack([hc.image(n) if channels == 3 else hc.gray(n) for n in names])


def _check_detector(key, names, sweep, channels=3):
    """One detect_batch call over all the images at minNeighbors 0 (every candidate of every image, in order),
    then one at minNeighbors 3 over the images whose lists groupRectangles can take (hc.GROUP_CAP)."""
    want = [hc.oracle_candidates(key, n, channels) for n in names]
    det = CascadeClassifier(hc.cascade(key))
    try:
        got = det.detect_batch(_stack(names, channels), 1.1, 0, cap=max(len(w) for w in want) + 16)
        assert det.last_sweep() == sweep
        assert _rects(det.candidates()) == want[0], (key, names[0])
        for n, g, w in zip(names, got, want):
            assert _rects(g) == w, (key, n)
        few = [n for n, w in zip(names, want) if len(w) <= hc.GROUP_CAP]
        got = det.detect_batch(_stack(few, channels), 1.1, 3)
        for n, g in zip(few, got):
            assert _rects(g) == hc.oracle_groups(key, n, channels), (key, n)
    finally:
        det.close()
    return want


@pytest.mark.parametrize("key", hc.TILED)
def test_tiled_sweep_on_every_class(key):
    want = _check_detector(key, hc.SMALL, 1)
    assert want[0] == want[1] == []  # white and black: every window flat
    assert sum(len(w) for w in want) >= 50


@pytest.mark.parametrize("key", hc.GLOBAL)
def test_global_memory_sweep_on_every_class(key):
    want = _check_detector(key, hc.LARGE, 2)
    assert want[0] == want[1] == []
    assert sum(len(w) for w in want) >= 50


@pytest.mark.parametrize("key,sweep", [(k, 1) for k in hc.WRAP_TILED] + [(k, 2) for k in hc.WRAP_GLOBAL])
def test_squared_sum_past_two_to_the_32(key, sweep):
    """360 x 270 near white: the squared-sum integral wraps past 2^32, the 200 x 200 window's
    own squared sum passes 2^31, and the all-white and all-black images have no candidate."""
    want = _check_detector(key, hc.WRAP, sweep)
    assert want[0] == want[1] == [] and len(want[2]) >= 50


def test_the_tie_table_on_the_device():
    """pass_all on the a | a + 20 edges: per window size the candidates of scale 0 are none where the table says
    flat and one per window row (column) where it says not flat -- read from the GPU's lists alone."""
    for key, names, sweep in [("pass20", hc.TIES, 1), ("pass24", hc.TIES, 1), ("pass14x28", hc.HTIES, 1),
                              ("pass100", [n + "@L" for n in hc.TIES], 2), ("pass60t", [n + "@L" for n in hc.TIES], 2)]:
        cs = hc.cascade(key)
        det = CascadeClassifier(cs)
        try:
            got = det.detect_batch(_stack(names, 3), 1.1, 0, cap=4096)
            assert det.last_sweep() == sweep
        finally:
            det.close()
        for n, g in zip(names, got):
            at0 = [r for r in _rects(g) if r[2:] == (cs.win_w, cs.win_h)]
            step = int(n.split(",")[1].split("@")[0])
            if step == 19 or (step == 20 and hc.TIE_FLAT[(cs.win_w, cs.win_h)]):
                assert at0 == [], (key, n)
            elif step == 20:
                axis = 1 if n.startswith("htie") else 0  # one tie window per window row (per column: htie)
                assert len(at0) == len({r[1 - axis] for r in at0}) >= 10, (key, n)
                assert len({r[axis] for r in at0}) == 1, (key, n)
            else:
                assert len(at0) >= 10, (key, n)


def _check_bank(keys, names, channels=3):
    want = {k: [hc.oracle_candidates(k, n, channels) for n in names] for k in keys}
    imgs = _stack(names, channels)
    cap = max(len(w) for ws in want.values() for w in ws) + 16
    bank = CascadeBank([hc.cascade(k) for k in keys])
    try:
        got = bank.detect_batch(imgs, 1.1, 0, cap=cap)
        for m, k in enumerate(keys):
            assert _rects(bank.candidates(m)) == want[k][0], (k, names[0])
            for i, n in enumerate(names):
                assert _rects(got[m][i]) == want[k][i], (k, n)
            det = CascadeClassifier(hc.cascade(k))  # the member alone
            try:
                alone = det.detect_batch(imgs, 1.1, 0, cap=cap)
            finally:
                det.close()
            for i, n in enumerate(names):
                assert np.array_equal(alone[i], got[m][i]), (k, n)
        few = [n for i, n in enumerate(names) if all(len(want[k][i]) <= hc.GROUP_CAP for k in keys)]
        got = bank.detect_batch(_stack(few, channels), 1.1, 3)
        for m, k in enumerate(keys):
            for i, n in enumerate(few):
                assert _rects(got[m][i]) == hc.oracle_groups(k, n, channels), (k, n)
        assert len(few) >= 2
    finally:
        bank.close()
    return want


def test_bank_of_probes_and_a_tilted_member():
    want = _check_bank(hc.BANK, hc.SMALL)  # every 173 x 97 class, the batch of the tiled sweep
    assert hc.cascade("gen24").has_tilted and not hc.cascade("pass20").has_tilted
    for k in hc.BANK:
        assert sum(len(w) for w in want[k]) >= 50, k


def test_bank_past_two_to_the_32():
    want = _check_bank(hc.WRAP_BANK, hc.WRAP)
    for k in hc.WRAP_BANK:
        assert want[k][0] == want[k][1] == [] and len(want[k][2]) >= 50, k


@pytest.mark.parametrize("key,sweep", [("pass20", 1), ("gen20", 1), ("pass14x28", 1), ("pass60t", 2), ("gen100", 2)])
def test_one_channel_input(key, sweep):
    names = hc.GRAY_TWINS if sweep == 1 else [n + "@L" for n in hc.GRAY_TWINS if not n.startswith("htie")]
    want = _check_detector(key, names, sweep, channels=1)
    assert sum(len(w) for w in want) >= 50


def test_bank_one_channel_input():
    _check_bank(["pass20", "pass14x28", "gen24"], hc.GRAY_TWINS, channels=1)


@pytest.mark.parametrize("W,H", [(640, 360), (600, 338), (300, 169)])  # general INTER_AREA, exact 2x, identity
def test_detect_frames_on_noise(W, H):
    """find_objects on full-range frames: INTER_AREA to width 300 on the device, then the stage-tie probe (about
    half of the windows sum to exactly the stage threshold) and a general readout calibrated on the first ROI."""
    raws = np.ascontiguousarray(pixel_content.noise(W, H, 1, 2, 17 + W)[:, 0])
    rois = [oracle.resize_area_bgr(r, 300) if W != 300 else r for r in raws]
    gen = hc.general(haar.bgr2gray(rois[0]), 1, 0.38, depth=2, tilted=True)
    for key, cs, neighbors in [("stage20", hc.cascade("stage20"), (0,)), ("gen", gen, (0, 3))]:
        cand = [[tuple(r) for r in haar.detect_candidates(cs, roi, 1.1)] for roi in rois]
        assert min(len(c) for c in cand) >= 50, key
        assert neighbors == (0,) or max(len(c) for c in cand) <= hc.GROUP_CAP, key
        det = CascadeClassifier(cs)
        try:
            for mn in neighbors:
                got = det.detect_frames(raws, 300, 1.1, mn, cap=max(len(c) for c in cand) + 16)
                assert _rects(det.candidates()) == cand[0], key
                for i, c in enumerate(cand):
                    assert _rects(got[i]) == (haar.group_rectangles(c, 3) if mn else c), (key, i)
        finally:
            det.close()
