"""GPU parity of the cascade bank (fm_haar_bank_*, CascadeBank): several cascades over the same images in
one pass.  Every member's ungrouped candidates and grouped detections must be the ones the cascade gives
alone: the fixture's for the reference's nine cascades (tests/golden/cascades_loosened.npz), oracle/haar.py's
for synthetic cascades of different window shapes, CascadeClassifier's wherever both run.
"""
import functools

import numpy as np
import pytest

import oracle
from find_motion_amd import CascadeBank, CascadeClassifier, FMError, _native
from find_motion_amd.cascade import CASCADE_LOOKUP, parse, to_xml
from haar_cases import candidates_and_results, loosen, make_cascade, make_image
from oracle import haar

pytestmark = pytest.mark.gpu

CAND_CAP = 1024  # the device candidate lists' capacity (kCandCap): a longer list makes the host walk the grid

MEMBERS = {
    "A": (1, dict(tight=0.41, depth=2)),
    "B": (1, dict(tight=0.38, win=(24, 24), depth=2, tilted=True)),
    "C": (2, dict(tight=0.38, win=(14, 28), stages=5)),
    "D": (3, dict(tight=0.41, win=(33, 17), tilted=True)),
    "E": (2, dict(tight=0.38, win=(64, 16), stages=3)),
    "F": (1, dict(tight=0.50)),
}


@functools.lru_cache(maxsize=None)
def _member(key):
    seed, kw = MEMBERS[key]
    return make_cascade(seed, **kw)


def _raw_frame(seed, W, H):
    small = make_image(seed, w=300, h=169)
    ys = (np.arange(H) * 169) // H
    xs = (np.arange(W) * 300) // W
    return np.ascontiguousarray(small[ys][:, xs])


@functools.lru_cache(maxsize=None)
def _image(key):
    if key == "roi":
        return make_image(2)
    if key == "roi_flipped":
        return np.ascontiguousarray(make_image(2)[::-1])
    if key == "mid":
        return make_image(2, w=173, h=97)
    if key == "small":
        return make_image(2, w=128, h=80)
    if key == "tiny":
        return np.ascontiguousarray(make_image(2, w=60, h=40)[:30, :60])
    if key == "speck":
        return np.ascontiguousarray(make_image(2, w=60, h=40)[:13, :13])
    kind, seed = key
    assert kind == "frame640"  # the ROI frame of a raw 640x360 frame
    return oracle.resize_area_bgr(_raw_frame(seed, 640, 360), 300)


@functools.lru_cache(maxsize=None)
def _oracle(member, image):
    """(candidates, per-window results) of oracle/haar.py, computed once per (member, image) for the module."""
    cand, res = candidates_and_results(_member(member), _image(image), 1.1)
    return [tuple(r) for r in cand], res


def _rects(a):
    return [tuple(r) for r in np.asarray(a).reshape(-1, 4).tolist()]


def _bank(keys, **kw):
    return CascadeBank([_member(k) for k in keys], **kw)


def _check_against_oracle(bank, keys, image_keys, got, min_neighbors):
    """got[m][i] against the oracle's grouped candidates; candidates(m) against image 0's."""
    for m, k in enumerate(keys):
        assert _rects(bank.candidates(m)) == _oracle(k, image_keys[0])[0], (k, image_keys[0])
        for i, ik in enumerate(image_keys):
            cand = _oracle(k, ik)[0]
            want = haar.group_rectangles(cand, min_neighbors) if min_neighbors > 0 else cand
            assert _rects(got[m][i]) == want, (k, ik)


# --- 1. the reference's nine cascades: fixture parity -------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loosened():
    from golden_cases import cascade_xml, load_loosened

    fx = load_loosened()
    return {name: (loosen(parse(cascade_xml(name)), fx[name]["lam"]), fx[name]) for name in CASCADE_LOOKUP}


@pytest.mark.parametrize("order", ["lookup", "reversed"])
def test_reference_cascades_in_one_bank(order):
    """The nine cascades of CASCADE_LOOKUP with the fixture's loosened thresholds (tilted features, multi-node
    trees, 14x28 and 19x23 windows and the 47-stage cascade among them) in one bank: every member's candidates
    and detections on the 300x169 and the 128x80 image are the fixture's, in either member order.  The
    fixture's lists hold 43-330 candidates per cascade at 300x169, so these come from the device lists."""
    names = list(CASCADE_LOOKUP)[::-1] if order == "reversed" else list(CASCADE_LOOKUP)
    fx = _loosened()
    bank = CascadeBank([fx[n][0] for n in names])
    assert len(bank) == 9
    for key in ("roi", "small"):
        got = bank.detect_batch(_image(key)[None], 1.1, 3)
        for m, n in enumerate(names):
            cand, dets = fx[n][1][key]
            assert len(cand) <= CAND_CAP
            assert _rects(bank.candidates(m)) == cand, (n, key)
            assert _rects(got[m][0]) == dets, (n, key)
    assert min(len(fx[n][1]["roi"][0]) for n in names) >= 20
    bank.close()


def test_reference_cascades_batch_of_three():
    """Image index > 0 with member index > 0 and the reference's stage sizes: three copies of the 300x169 image
    give each copy the fixture's detections."""
    names = list(CASCADE_LOOKUP)
    fx = _loosened()
    bank = CascadeBank([fx[n][0] for n in names])
    got = bank.detect_batch(np.stack([_image("roi")] * 3), 1.1, 3)
    for m, n in enumerate(names):
        for i in range(3):
            assert _rects(got[m][i]) == fx[n][1]["roi"][1], (n, i)
        assert _rects(bank.candidates(m)) == fx[n][1]["roi"][0], n
    bank.close()


# --- 2. synthetic windows of different shapes against the live oracle ---------------------------------

def test_mid_image_every_member_rejects_early_and_late_and_scale_lists_differ():
    # what makes the comparisons below say something, from the oracle alone
    nsc = {}
    for k in MEMBERS:
        res = _oracle(k, "mid")[1]
        assert (res == 0).any() and (res < 0).any(), k  # stage-0 rejections (the row walk's skip) and later ones
        cs, n, f = _member(k), 0, 1.0
        while round(cs.win_w * f) <= 173 and round(cs.win_h * f) <= 97:
            n, f = n + 1, f * 1.1
        nsc[k] = n
    assert len(set(nsc.values())) >= 4, nsc  # the members' prefixes of the shared scale list end in different places


def test_mid_image_device_lists():
    """{A, B, C, F} on 173x97: no list is longer than the device lists hold, so the candidates come from
    k_bwalk's lists; F (a cascade that rejects everything) stays empty beside the others."""
    keys = ["A", "B", "C", "F"]
    for k in "ABC":
        assert 40 <= len(_oracle(k, "mid")[0]) <= CAND_CAP, k
    assert _oracle("F", "mid")[0] == []
    bank = _bank(keys)
    got = bank.detect_batch(_image("mid")[None], 1.1, 3)
    _check_against_oracle(bank, keys, ["mid"], got, 3)
    bank.close()


def test_mid_image_overflowing_lists_walk_the_grid_on_the_host():
    """{A..F} on 173x97: D and E overflow their lists, so every member's candidates (A's short list too)
    come from the host's walk of the whole result grid."""
    keys = list(MEMBERS)
    assert len(_oracle("D", "mid")[0]) > CAND_CAP and len(_oracle("E", "mid")[0]) > CAND_CAP
    assert 0 < len(_oracle("A", "mid")[0]) < CAND_CAP
    bank = _bank(keys)
    got = bank.detect_batch(_image("mid")[None], 1.1, 3)
    _check_against_oracle(bank, keys, ["mid"], got, 3)
    bank.close()


def test_roi_image_batch_of_two_ungrouped():
    """{A..F} on the 300x169 image upside down and upright, minNeighbors 0 (the raw candidates of both images,
    thousands for D and E)."""
    keys = list(MEMBERS)
    imgs = ["roi_flipped", "roi"]
    assert any(_oracle(k, imgs[0])[0] != _oracle(k, imgs[1])[0] for k in keys)
    for k in "ABCDE":
        assert _oracle(k, imgs[0])[0] != _oracle(k, imgs[1])[0], k
    bank = _bank(keys)
    got = bank.detect_batch(np.stack([_image(i) for i in imgs]), 1.1, 0)
    _check_against_oracle(bank, keys, imgs, got, 0)
    bank.close()


def test_member_without_a_scale_and_image_without_a_window():
    # 60x30: the 64x16 window of E fits nowhere (no scale at all) while C and D find candidates
    keys = list(MEMBERS)
    assert _oracle("E", "tiny")[0] == [] and len(_oracle("D", "tiny")[0]) >= 20 and len(_oracle("C", "tiny")[0]) >= 1
    bank = _bank(keys)
    got = bank.detect_batch(_image("tiny")[None], 1.1, 3)
    _check_against_oracle(bank, keys, ["tiny"], got, 3)
    assert len(got[keys.index("E")][0]) == 0 and len(bank.candidates(keys.index("E"))) == 0
    # 13x13: smaller than every window; no error, nothing found, and the bank works afterwards
    got = bank.detect_batch(np.stack([_image("speck")] * 2), 1.1, 3)
    assert [[len(r) for r in per] for per in got] == [[0, 0]] * len(keys)
    assert all(len(bank.candidates(m)) == 0 for m in range(len(keys)))
    got = bank.detect_batch(_image("tiny")[None], 1.1, 3)
    _check_against_oracle(bank, keys, ["tiny"], got, 3)
    bank.close()


# --- 3. a bank of one -------------------------------------------------------------------------------

def test_bank_of_one_equals_the_detector():
    cs = _member("B")
    bank, det = CascadeBank([cs]), CascadeClassifier(cs)
    img = _image("roi")
    got = bank.detect_batch(img[None], 1.1, 3)
    want = det.detect_batch(img[None], 1.1, 3)
    assert len(got) == 1 and _rects(got[0][0]) == _rects(want[0]) and len(want[0]) >= 1
    assert _rects(bank.candidates(0)) == _rects(det.candidates()) and len(det.candidates()) > CAND_CAP
    g = haar.bgr2gray(_image("mid"))  # gray input, device lists
    assert _rects(bank.detect_batch(g[None], 1.1, 3)[0][0]) == _rects(det.detect_batch(g[None], 1.1, 3)[0])
    assert _rects(bank.candidates(0)) == _rects(det.candidates())
    bank.close()
    det.close()


# --- 4. frames and the ROI stage -------------------------------------------------------------------

def test_frame_routes_agree_with_the_detectors_and_the_oracle():
    """Raw 640x360 frames through the five routes (host array, CUDA tensor, (ptr, n, H, W), a list of
    separate device frames, the asynchronous list): all equal the single detectors' detect_frames and the
    oracle on the INTER_AREA ROI frame."""
    import torch

    keys = ["A", "B", "C"]
    seeds = [2, 0]
    raws = np.stack([_raw_frame(s, 640, 360) for s in seeds])
    bank = _bank(keys)
    dev = torch.from_numpy(raws).to("cuda:0")
    ring = torch.zeros((5, 360, 640, 3), dtype=torch.uint8, device="cuda:0")
    slots = [3, 1]
    for i, k in enumerate(slots):
        ring[k].copy_(dev[i])
    torch.cuda.synchronize()
    ptrs = [ring[k].data_ptr() for k in slots]
    routes = {
        "host": bank.detect_frames(raws, 300, 1.1, 3),
        "tensor": bank.detect_frames(dev, 300, 1.1, 3),
        "pointer": bank.detect_frames((dev.data_ptr(), 2, 360, 640), 300, 1.1, 3),
        "list": bank.detect_frame_list(ptrs, 360, 640, 300, 1.1, 3),
    }
    assert bank.detect_frame_list_async(ptrs, 360, 640, 300, 1.1, 3) == 2
    with pytest.raises(FMError) as e:  # one detection in flight per bank
        bank.detect_frame_list_async(ptrs, 360, 640, 300, 1.1, 3)
    assert e.value.code == _native.FM_ESTATE
    with pytest.raises(FMError) as e:  # (this collects the queued detection; its results stay)
        bank.collect(3)
    assert e.value.code == _native.FM_ESTATE
    routes["async"] = bank.collect(2, cap=1)  # grows the cap and collects again
    image_keys = [("frame640", s) for s in seeds]
    for name, got in routes.items():
        for m, k in enumerate(keys):
            for i, ik in enumerate(image_keys):
                assert _rects(got[m][i]) == haar.group_rectangles(_oracle(k, ik)[0], 3), (name, k, i)
    assert any(len(r) for per in routes["host"] for r in per)
    with pytest.raises(ValueError):
        bank.detect_frames(dev[:, :, ::2], 300)  # not contiguous
    for m, k in enumerate(keys):
        det = CascadeClassifier(_member(k))
        one = det.detect_frames(raws, 300, 1.1, 3)
        assert [_rects(r) for r in one] == [_rects(r) for r in routes["host"][m]], k
        det.close()
    bank.close()


def test_identity_size_and_roi_upscale():
    keys = ["A", "B", "C"]
    bank = _bank(keys)
    frame = _raw_frame(2, 300, 169)  # already 300 wide: the ROI stage passes it through
    assert np.array_equal(frame, _image("roi"))
    got = bank.detect_frames(frame[None], 300, 1.1, 3)
    _check_against_oracle(bank, keys, ["roi"], got, 3)
    narrow = np.ascontiguousarray(_raw_frame(0, 640, 360)[:120, :200])
    with pytest.raises(FMError) as e:  # narrower than the ROI: refused unless the switch is on
        bank.detect_frames(narrow[None], 300, 1.1, 3)
    assert e.value.code == _native.FM_ENOTSUP
    bank.set_roi_upscale(True)
    up = bank.detect_frames(narrow[None], 300, 1.1, 3)
    for m, k in enumerate(keys):
        det = CascadeClassifier(_member(k), roi_upscale=True)
        assert _rects(det.detect_frames(narrow[None], 300, 1.1, 3)[0]) == _rects(up[m][0]), k
        det.close()
    assert any(len(per[0]) for per in up)
    bank.close()
    again = CascadeBank([_member(k) for k in keys], roi_upscale=True)  # the constructor's switch
    assert [_rects(per[0]) for per in again.detect_frames(narrow[None], 300, 1.1, 3)] == [_rects(per[0]) for per in up]
    again.close()


# --- 5. one bank across changing geometry -----------------------------------------------------------

def test_one_bank_across_changing_sizes_and_batches():
    """300x169 x1, 128x80 x3, 300x169 x1, 173x97 x2 on one bank (grow-only buffers, the geometry table of the
    call before): each call gives what a fresh bank gives."""
    keys = list(MEMBERS)
    calls = [((300, 169), [2]), ((128, 80), [2, 5, 7]), ((300, 169), [3]), ((173, 97), [2, 4])]
    bank = _bank(keys)
    for (w, h), seeds in calls:
        imgs = np.stack([make_image(s, w=w, h=h) for s in seeds])
        got = bank.detect_batch(imgs, 1.1, 3)
        cand = [_rects(bank.candidates(m)) for m in range(len(keys))]
        fresh = _bank(keys)
        want = fresh.detect_batch(imgs, 1.1, 3)
        assert [[_rects(r) for r in per] for per in got] == [[_rects(r) for r in per] for per in want], (w, h)
        assert cand == [_rects(fresh.candidates(m)) for m in range(len(keys))], (w, h)
        assert any(cand), (w, h)
        fresh.close()
    bank.close()


# --- 6. the drop-in ---------------------------------------------------------------------------------

def test_video_motion_find_objects_with_two_cascades(tmp_path, monkeypatch):
    from types import SimpleNamespace

    from find_motion_amd import motion, videoio

    (tmp_path / "haarcascade_frontalface_default.xml").write_text(to_xml(_member("A")))
    (tmp_path / "haarcascade_fullbody.xml").write_text(to_xml(_member("C")))
    calls = []
    real = CascadeClassifier.detect_frames
    monkeypatch.setattr(CascadeClassifier, "detect_frames", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))

    def vm_of(names):
        return motion.VideoMotion(filename=str(tmp_path / "v"), capture=videoio.SyntheticCapture(640, 360, 4, 0),
                                  box_size=100, cascades=names, cascade_dir=str(tmp_path), outdir=str(tmp_path))

    vm = vm_of(["fullbody", "frontalface_default"])
    assert list(vm.cascades) == ["Person", "Face 4"]
    fr = SimpleNamespace(raw=_raw_frame(2, 640, 360))
    for _ in range(14):
        assert vm.find_objects(fr, minNeighbours=2) == set()
    seen = vm.find_objects(fr, minNeighbours=2)
    want = {}
    for title, k in (("Person", "C"), ("Face 4", "A")):
        rects = haar.group_rectangles(_oracle(k, ("frame640", 2))[0], 2)
        if rects:
            want[title] = [((x, y), (x + w, y + h)) for x, y, w, h in rects]
    assert want, "the oracle finds nothing: the comparison would be empty"
    assert seen == set(want)
    assert vm.last_objects == want and list(vm.last_objects) == [t for t in vm.cascades if t in want]
    if motion.FIND_OBJECTS_USES_BANK:
        assert vm.cascade_bank is not None and len(vm.cascade_bank) == 2 and calls == []
    else:
        assert vm.cascade_bank is None and len(calls) == 2
    assert vm_of(["frontalface_default"]).cascade_bank is None
