"""The cases of test_gpu_haar_content.py reach their edges, proven on oracle/haar.py alone (no GPU).

Each content class of tests/haar_content.py exists for one place where the Haar stage could be wrong unseen: the
mod-2^32 squared-sum integral, the float rounding of 1 / sqrt(nf) at the sigma = 10 cut, `<` at a node and at a
stage threshold, the two fixed-point roundings in front of the integrals and the uncontracted float32 feature sum.
This module asserts that the committed images and probes sit on those edges, and that each named wrong
restatement of the oracle changes the candidate list of a committed case, so the GPU comparison cannot pass a
kernel that makes that mistake.
"""
import contextlib

import numpy as np
import pytest

import haar_content as hc
from haar_cases import candidates_and_results
from oracle import haar


@contextlib.contextmanager
def patched(**attrs):
    old = {k: getattr(haar, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(haar, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(haar, k, v)


def _candidates(key, name, **attrs):
    with patched(**attrs):
        return [tuple(r) for r in haar.detect_candidates(hc.cascade(key), hc.image(name), 1.1)]


def _eval(**sw):
    return lambda *a: hc.eval_windows_variant(*a, **sw)


# --- the restatements with no switch on are the oracle ---------------------------------------------------------

@pytest.mark.parametrize("key,name", [("gen20", "noise"), ("gen24", "gray_edges"), ("stage20", "checker"),
                                      ("frac20t", "stripes2"), ("gen100", "noise@L"), ("pass60t", "vtie:100,20@L")])
def test_variants_without_a_switch_restate_the_oracle(key, name):
    want = hc.oracle_candidates(key, name)
    assert _candidates(key, name, eval_windows=_eval(), resize_linear_exact=hc.resize_variant) == want
    g = hc.gray(name)
    for dw, dh in [(157, 88), (86, 48), (31, 17)]:
        assert np.array_equal(hc.resize_variant(g, dw, dh), haar.resize_linear_exact(g, dw, dh))


# --- white_wrap -----------------------------------------------------------------------------------------------

def test_wrap_images_pass_two_to_the_32_and_windows_straddle_a_wrap():
    g = hc.gray("wrap").astype(np.int64)
    assert int((g * g).sum()) > 1 << 32
    assert int((hc.gray("wrap_white").astype(np.int64) ** 2).sum()) > 1 << 32
    assert int((hc.gray("wrap_dots").astype(np.int64) ** 2).sum()) > 1 << 32
    assert 1 << 31 < int((hc.gray("white300").astype(np.int64) ** 2).sum()) < 1 << 32
    assert g.min() == 215 and g.max() == 255
    for key in ("pass20", "pass100", "pass200"):
        cs = hc.cascade(key)
        S, Q, T, xs, ys = hc.scale0(cs, hc.gray("wrap"))
        q = Q.astype(np.int64) & 0xFFFFFFFF
        p0 = q[ys + 1, xs + 1]
        p3 = q[ys + cs.win_h - 1, xs + cs.win_w - 1]
        assert int((p3 < p0).sum()) >= 1, key  # the far corner wrapped, the near one not yet
    # the window's own squared sum passes 2^31 only for the 200 x 200 window (198^2 * 215^2 < 2^31 < 198^2 * 245^2);
    # a window of the tiled sweep holds at most 86^2 * 255^2 < 2^31, so (uint32_t) there cannot differ from int32
    cs = hc.cascade("pass200")
    S, Q, T, xs, ys = hc.scale0(cs, hc.gray("wrap"))
    vq = haar._rect_sum(Q, xs, ys, (1, 1, 198, 198), False).astype(np.int64)
    assert (vq < 0).all()
    assert 86 * 86 * 255 * 255 < 1 << 31


def test_flat_images_have_no_candidate():
    for key, name in [("pass20", "white"), ("pass20", "black"), ("pass20", "wrap_white"), ("pass20", "wrap_black"),
                      ("pass100", "white@L"), ("pass100", "wrap_black")]:
        assert hc.oracle_candidates(key, name) == [], (key, name)
    # the dotted white is flat except where a window's norm rect reaches a dot of the second-outermost ring
    # (one black pixel among the 98 x 98 of a 100 x 100 window's norm rect leaves sigma at 2.6: flat)
    assert hc.oracle_candidates("pass100", "dots@L") == []
    for key, name in [("pass20", "dots"), ("pass20", "wrap_dots")]:
        n = len(hc.oracle_candidates(key, name))
        print(key, name, n)
        assert n >= 10, (key, name)


# --- sigma_tie ------------------------------------------------------------------------------------------------

TIE_CASES = [(win, f"vtie:{a},{{}}" + size) for win, size in [((20, 20), ""), ((24, 24), ""), ((100, 100), "@L"),
                                                              ((60, 60), "@L")] for a in (0, 100, 235)]
TIE_CASES += [((14, 28), "htie:100,{}")]


@pytest.mark.parametrize("win,name", TIE_CASES)
def test_sigma_tie_windows_sit_on_the_cut(win, name):
    cs = hc.pass_all(win)
    area = (win[0] - 2) * (win[1] - 2)
    verdicts = {}
    for step in (19, 20, 21):
        S, Q, T, xs, ys = hc.scale0(cs, hc.gray(name.format(step)))
        nr = (1, 1, win[0] - 2, win[1] - 2)
        vs = haar._rect_sum(S, xs, ys, nr, False).astype(np.int64)
        vq = haar._rect_sum(Q, xs, ys, nr, False).astype(np.int64) & 0xFFFFFFFF
        nf = area * vq - vs * vs  # exact in int64
        half = 2 * vs == area * sum(hc.tie_levels(int(name.split(":")[1].split(",")[0]), step))  # split in half
        if step == 20:
            rows = len(np.unique(ys))
            tie = nf == 100 * area * area
            assert np.array_equal(tie, half) and int(tie.sum()) >= rows
        ok, _ = hc.feature_values(cs, S, Q, T, xs, ys)
        assert len(set(ok[half].tolist())) == 1
        verdicts[step] = not ok[half][0]  # flat?
        if step == 20:
            assert not ok[~half].any()  # every other scale-0 window is flat: sigma < 10
            # 1 / sqrt(nf) kept in double: 0.0999...9 (kept) for 20 x 20 and 24 x 24, exactly 0.1 (flat) for the others,
            # so the float cast shows on 20 x 20, 24 x 24 (flat only in float) and 60 x 60 (flat only in double)
            ok_d, _ = hc.feature_values(cs, S, Q, T, xs, ys, vnf_double=True)
            assert (~ok_d[half]).all() == hc.TIE_FLAT_DOUBLE[win] and len(set(ok_d[half].tolist())) == 1
    assert verdicts == {19: True, 20: hc.TIE_FLAT[win], 21: False}


# --- node and stage ties --------------------------------------------------------------------------------------

def _spied(key, name):
    cs = hc.cascade(key)
    S, Q, T, xs, ys = hc.scale0(cs, hc.gray(name))
    spy = {}
    res = hc.eval_windows_variant(cs, S, Q, T, xs, ys, spy=spy)
    assert np.array_equal(res, haar.eval_windows(cs, S, Q, T, xs, ys))
    return res, spy


@pytest.mark.parametrize("key,name", [("node20", "stripes2"), ("node100", "stripes2@L")])
def test_node_tie_windows_have_a_feature_of_exactly_zero(key, name):
    res, spy = _spied(key, name)
    tie = spy["ok"] & (spy["vals"][0] == 0.0)
    assert int(tie.sum()) >= 50 and (res[tie] == 1).all()


@pytest.mark.parametrize("key,name", [("stage20", "noise"), ("stage20", "gray_edges"), ("stage60t", "noise@L")])
def test_stage_tie_windows_sum_to_exactly_the_threshold(key, name):
    res, spy = _spied(key, name)
    alive, tot = spy["sums"][0]
    assert float(hc.cascade(key).stage_threshold[0]) == 0.75
    tie = tot == 0.75
    assert int(tie.sum()) >= 50 and (res[alive[tie]] == 1).all()
    assert (tot == 0.5).any() and (tot == 1.0).any()


@pytest.mark.parametrize("key,name", [("frac20", "stripes2"), ("frac20t", "stripes2"), ("frac100", "stripes2@L")])
def test_snapped_windows_tie_at_every_node(key, name):
    cs = hc.cascade(key)
    res, spy = _spied(key, name)
    assert (res == 1).all() and len(res) >= 50
    assert (spy["vals"][cs.node_feature] == cs.node_threshold[:, None]).all()
    w = cs.feat_weights[1:][cs.feat_weights[1:] != 0]  # (feature 0 is stage 0's centre-surround: -1 and 4)
    assert ((np.abs(w) >= 0.3) & (np.abs(w) <= 3)).all() and (cs.feat_weights[:, 2] != 0).any()
    m, e = np.frexp(w)  # no weight is dyadic within 12 bits
    assert (m * 4096 != np.round(m * 4096)).all()


# --- the general readouts are not vacuous ---------------------------------------------------------------------

@pytest.mark.parametrize("key,name", [("gen20", "noise"), ("gen20", "gray_edges"), ("gen20", "checker"),
                                      ("gen24", "noise"), ("gen24", "gray_edges"), ("gen20w", "wrap"),
                                      ("gen100", "noise@L"), ("gen100", "gray_edges@L"), ("gen60t", "noise@L"),
                                      ("gen60t", "gray_edges@L"), ("gen60tw", "wrap")])
def test_general_readouts_accept_and_reject_early_and_late(key, name):
    """The rule of test_gpu_haar._check_against_live_oracle: accepted windows at least 50 and at most half of
    all, stage-0 rejections and later ones both present, flat windows not counted as later rejections."""
    cs = hc.cascade(key)
    _, flat = candidates_and_results(hc.pass_all((cs.win_w, cs.win_h)), hc.image(name), 1.1)
    cand, res = candidates_and_results(cs, hc.image(name), 1.1)
    acc, zero = int((res == 1).sum()), int((res == 0).sum())
    later = int((res < 0).sum()) - int((flat == -1).sum())
    print(f"{key} {name}: windows {len(res)}, accepted {acc}, stage 0 {zero}, later {later}, candidates {len(cand)}")
    assert 50 <= acc <= len(res) // 2 and zero > 0 and later > 0
    assert len(cand) <= hc.GROUP_CAP  # grouped at minNeighbors 3 on the GPU as well


# --- sensitivity: each wrong restatement changes a committed case ----------------------------------------------

MISTAKES = {
    "vnf_double": (dict(eval_windows=_eval(vnf_double=True)),
                   [("pass20", "vtie:0,20"), ("pass20", "vtie:100,20"), ("pass20", "vtie:235,20"),
                    ("pass24", "vtie:100,20"), ("pass60t", "vtie:0,20@L"), ("pass60t", "vtie:100,20@L"),
                    ("pass60t", "vtie:235,20@L")]),
    "vq_signed": (dict(eval_windows=_eval(vq_signed=True)), [("pass200", "wrap")]),
    "saturating_integrals": (dict(integrals=hc.integrals_saturating),
                             [("pass20", "wrap"), ("pass100", "wrap"), ("pass20", "wrap_dots"), ("gen20w", "wrap")]),
    "node_le": (dict(eval_windows=_eval(node_le=True)),
                [("node20", "stripes2"), ("node100", "stripes2@L"), ("frac20", "stripes2")]),
    "stage_le": (dict(eval_windows=_eval(stage_le=True)),
                 [("stage20", "noise"), ("stage20", "gray_edges"), ("stage60t", "noise@L")]),
    "gray_without_8192": (dict(bgr2gray=hc.gray_truncating),
                          [("gen20", "gray_edges"), ("gen20", "noise"), ("gen100", "gray_edges@L")]),
    "resize_without_2_15": (dict(resize_linear_exact=lambda g, w, h: hc.resize_variant(g, w, h, no_round=True)),
                            [("gen20", "gray_edges"), ("gen20", "checker"), ("gen24", "gray_edges"),
                             ("gen60t", "gray_edges@L"), ("stage20", "checker"), ("node20", "checker"),
                             ("stage20", "noise")]),
    "contracted_sum": (dict(eval_windows=_eval(contracted=True)),
                       [("frac20", "stripes2"), ("frac20t", "stripes2"), ("frac100", "stripes2@L")]),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_each_mistake_changes_the_candidates_of_its_cases(mistake):
    attrs, cases = MISTAKES[mistake]
    for key, name in cases:
        want = hc.oracle_candidates(key, name)
        got = _candidates(key, name, **attrs)
        moved = len(set(want) ^ set(got))
        print(f"{mistake}: {key} on {name}: {len(want)} candidates, {moved} moved")
        assert got != want, (key, name)
        if mistake == "contracted_sum":
            assert moved >= 10, (key, name)


def test_the_resize_clamp_cannot_bind():
    """min(v, 255) behind (h0 * (256 - c) + h1 * c + 2^15) >> 16: the horizontal values are at most 255 * 256 and
    the vertical taps sum to 256, so v <= (255 * 65536 + 32768) >> 16 = 255: no input reaches the clamp, a kernel
    without it computes the same, and no case is asked to tell the two apart.  On the committed content the
    unclamped restatement gives the same pixels."""
    assert (255 * 256 * 256 + (1 << 15)) >> 16 == 255
    for name in ("white", "checker", "noise", "dots"):
        g = hc.gray(name)
        for dw, dh in [(157, 88), (143, 80), (86, 48)]:
            assert np.array_equal(hc.resize_variant(g, dw, dh, no_clamp=True), haar.resize_linear_exact(g, dw, dh))


def test_batches_put_the_extremes_side_by_side():
    assert hc.SMALL[:3] == ["white", "black", "noise"] and hc.LARGE[:3] == ["white@L", "black@L", "noise@L"]
    for names in (hc.SMALL, hc.LARGE, hc.WRAP):
        assert len({hc.image(n).shape for n in names}) == 1
    assert hc.image("noise").shape == (97, 173, 3) and hc.image("wrap").shape == (270, 360, 3)
    assert len(np.unique(hc.image("noise"))) == 256
    res = (hc.image("gray_edges").astype(np.int64) * [1868, 9617, 4899]).sum(-1) % 16384
    for r in (8191, 8192, 16383, 0):
        assert int((res == r).sum()) >= 100, r
