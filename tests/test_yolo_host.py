"""The host side of the YOLOv3 object stage on a machine without a GPU: the Darknet cfg parser and weights
loader (find_motion_amd/darknet.py), the restated 8-bit INTER_LINEAR and blob table, cvlib's box loop and
NMSBoxes (the product's host tail and tests/yolo_ref.py's restatement alike), fm_yolo_create's refusals (host
code of the built library), the drop-in's wiring with a fake detector, known answers for the yolov3 and
yolov3-tiny generators, and the exact integer convolution reference."""
import ctypes as C
import logging
import struct
from argparse import ArgumentParser
from types import SimpleNamespace

import numpy as np
import pytest

import yolo_ref as yr
from fake_engine import OracleEngine
from find_motion_amd import _native, cli, motion, videoio
from find_motion_amd import darknet as dk

CFG = """
# a miniature with every layer kind
[net]
width=32
height = 32
channels=3
momentum=0.9

[convolutional]
batch_normalize=1
filters=8
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
batch_normalize=1
filters = 8
size=1
stride=1
pad=1
activation=leaky

[shortcut]
from=-2
activation=linear

[maxpool]
size=2
stride=1

[convolutional]
filters=16
size=3
stride=2
pad=1
activation=linear

[yolo]
mask = 0,1
anchors = 1,2, 3,4, 5,6
classes=3
num=3
jitter=.3
ignore_thresh = .7
truth_thresh = 1
random=1

[route]
layers = -3

[upsample]
stride=2

[route]
layers = -1, 0

[convolutional]
filters=8
size=1
stride=1
pad=1
activation=linear

[yolo]
mask = 2
anchors = 1,2, 3,4, 5,6
classes=3
num=3
"""


def test_cfg_known_answers():
    net, layers = dk.parse_cfg(CFG)
    assert net["width"] == "32" and net["height"] == "32" and net["channels"] == "3"
    assert [ly["kind"] for ly in layers] == [dk.CONV, dk.MAXPOOL, dk.CONV, dk.SHORTCUT, dk.MAXPOOL, dk.CONV, dk.YOLO,
                                             dk.ROUTE, dk.UPSAMPLE, dk.ROUTE, dk.CONV, dk.YOLO]
    assert [ly["index"] for ly in layers] == list(range(12))
    assert [ly["out_c"] for ly in layers] == [8, 8, 8, 8, 8, 16, 16, 8, 8, 16, 8, 8]
    assert [ly["in_c"] for ly in layers] == [3, 8, 8, 8, 8, 8, 16, 16, 8, 8, 16, 8]
    c0, c2, c5 = layers[0], layers[2], layers[5]
    assert (c0["filters"], c0["size"], c0["stride"], c0["pad"], c0["batch_normalize"], c0["activation"]) == \
        (8, 3, 1, 1, 1, "leaky")
    assert (c2["size"], c2["pad"]) == (1, 0)  # pad=1 means size // 2
    assert (c5["filters"], c5["stride"], c5["batch_normalize"], c5["activation"]) == (16, 2, 0, "linear")
    assert (layers[1]["size"], layers[1]["stride"]) == (2, 2) and (layers[4]["size"], layers[4]["stride"]) == (2, 1)
    assert layers[3]["from"] == 1
    assert layers[7]["layers"] == [4]      # -3 from layer 7
    assert layers[9]["layers"] == [8, 0]   # -1 and the absolute 0, in the order given
    assert layers[8]["stride"] == 2
    y = layers[6]
    assert y["mask"] == [0, 1] and y["classes"] == 3 and y["num"] == 3 and y["anchors"] == [(1, 2), (3, 4), (5, 6)]
    assert "jitter" not in y and "random" not in y
    assert layers[11]["mask"] == [2]
    # the project's own generator parses too
    _, mini = dk.parse_cfg(yr.mini_cfg())
    assert len(mini) == 17 and sum(ly["kind"] == dk.YOLO for ly in mini) == 2


def _with(section_text, replace=None):
    """CFG with one more section at the end, or with `replace` = (old, new) applied."""
    return CFG.replace(*replace) if replace else CFG + "\n" + section_text


@pytest.mark.parametrize("text, where", [
    (_with("[dropout]\nprobability=.5\n"), r"\[dropout\] \(section 13"),
    (_with("[convolutional]\nfilters=4\nsize=1\nstride=1\ngroups=2\nactivation=linear\n"), r"section 13.*groups"),
    (_with("[convolutional]\nfilters=4\nsize=1\nstride=1\nactivation=mish\n"), r"section 13.*activation=mish"),
    (_with("[convolutional]\nfilters=4\nsize=5\nstride=1\nactivation=linear\n"), r"section 13.*size=5"),
    (_with("[convolutional]\nfilters=4\nsize=3\nstride=3\nactivation=linear\n"), r"section 13.*stride=3"),
    (_with("[maxpool]\nsize=3\nstride=2\n"), r"\[maxpool\] \(section 13.*size=3"),
    (_with("[maxpool]\nsize=2\nstride=3\n"), r"\[maxpool\] \(section 13.*stride=3"),
    (_with("[upsample]\nstride=4\n"), r"\[upsample\] \(section 13.*stride=4"),
    (_with("[route]\nlayers=12\n"), r"\[route\] \(section 13.*outside"),
    (_with("[route]\nlayers=-1,-2,-3\n"), r"\[route\] \(section 13.*one or two"),
    (_with("[shortcut]\nfrom=-3\nactivation=leaky\n"), r"\[shortcut\] \(section 13.*activation=leaky"),
    (_with("[shortcut]\nfrom=5\nactivation=linear\n"), r"\[shortcut\] \(section 13.*adds 16 channels to 8"),
    (_with("[yolo]\nmask=0,1\nanchors=1,2, 3,4, 5,6\nclasses=3\nnum=3\n"), r"\[yolo\] \(section 13.*8 input channels"),
    (_with(None, ("mask = 2\n", "mask = 2\nscale_x_y=1.05\n")), r"\[yolo\] \(section 12.*scale_x_y"),
    (_with(None, ("mask = 2\n", "mask = 3\n")), r"\[yolo\] \(section 12.*mask"),
    (_with(None, ("size=2\nstride=1", "size=2\nstride=1\n[avgpool]")), r"\[avgpool\] \(section 6"),
    ("[convolutional]\nfilters=1\n", r"starts with \[net\]"),
])
def test_cfg_refusals_name_the_section(text, where):
    with pytest.raises(ValueError, match=where):
        dk.parse_cfg(text)


def _raw_for(layers, seed=3):
    return yr.random_raw(layers, seed)


@pytest.mark.parametrize("major, minor, seen_bytes", [(0, 1, 4), (0, 2, 8), (1, 0, 8)])
def test_weights_loader_both_seen_widths_and_the_fold(major, minor, seen_bytes):
    _, layers = dk.parse_cfg(CFG)
    raw = _raw_for(layers)
    data = dk.write_weights(layers, raw, major, minor, seen=12345)
    n_floats = sum(a.size for i in raw for a in raw[i])
    assert len(data) == 12 + seen_bytes + 4 * n_floats
    assert struct.unpack_from("<iii", data) == (major, minor, 0)
    params = dk.load_weights(data, layers)
    assert [p is not None for p in params] == [ly["kind"] == dk.CONV for ly in layers]
    for ly in layers:
        if ly["kind"] != dk.CONV:
            continue
        w, b = params[ly["index"]]
        assert w.dtype == np.float32 and b.dtype == np.float32
        assert w.shape == (ly["filters"], ly["in_c"], ly["size"], ly["size"]) and b.shape == (ly["filters"],)
        if ly["batch_normalize"]:
            beta, gamma, mean, var, w0 = (a.astype(np.float64) for a in raw[ly["index"]])
            for m in range(ly["filters"]):  # the definition, one filter at a time, rounded once
                s = gamma[m] / np.sqrt(var[m] + 1e-6)
                assert np.array_equal(w[m], (w0[m] * s).astype(np.float32))
                assert b[m] == np.float32(beta[m] - mean[m] * s)
        else:
            assert np.array_equal(b, raw[ly["index"]][0]) and np.array_equal(w, raw[ly["index"]][1])


def test_weights_loader_from_a_path_and_wrong_lengths(tmp_path):
    _, layers = dk.parse_cfg(CFG)
    data = dk.write_weights(layers, _raw_for(layers))
    p = tmp_path / "m.weights"
    p.write_bytes(data)
    a, b = dk.load_weights(str(p), layers), dk.load_weights(data, layers)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b) if x is not None)
    for cut in (4, 1, len(data) - 20, len(data) - 8):
        with pytest.raises(ValueError, match="too short"):
            dk.load_weights(data[:-cut], layers)
    with pytest.raises(ValueError, match="4 bytes left over"):
        dk.load_weights(data + b"\0\0\0\0", layers)
    with pytest.raises(ValueError, match="1 bytes left over"):
        dk.load_weights(data + b"\0", layers)
    (tmp_path / "names.txt").write_text("person\nbicycle\n\ntraffic light\n")
    assert dk.load_classes(str(tmp_path / "names.txt")) == ["person", "bicycle", "traffic light"]


# ---- the restated INTER_LINEAR and the blob table -------------------------------------------------------------
def test_inter_linear_identity_ramp_and_clamps():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    assert np.array_equal(yr.resize_linear_u8(img, 9, 7), img)
    # equal sizes through the arithmetic as well: coefficient 2048 on the pixel itself
    s0, s1, a0, a1 = yr.linear_taps(9, 9)
    assert s0.tolist() == list(range(9)) and a0.tolist() == [2048] * 9 and a1.tolist() == [0] * 9
    # an exact 2x upscale of a ramp: taps at 1/4 and 3/4 between neighbours, both borders clamped
    ramp = np.array([[0, 8, 16, 24]], np.uint8).reshape(1, 4, 1)
    assert yr.resize_linear_u8(ramp, 8, 1)[0, :, 0].tolist() == [0, 2, 6, 10, 14, 18, 22, 24]
    col = ramp.transpose(1, 0, 2)
    assert yr.resize_linear_u8(col, 1, 8)[:, 0, 0].tolist() == [0, 2, 6, 10, 14, 18, 22, 24]
    s0, s1, a0, a1 = yr.linear_taps(4, 8)
    assert (s0[0], s1[0], a0[0], a1[0]) == (0, 1, 2048, 0)      # fx < 0: the first pixel alone
    assert (s0[7], s1[7], a0[7], a1[7]) == (3, 3, 2048, 0)      # sx >= w - 1: the last pixel, second tap clamped
    assert (s0[1], s1[1], a0[1], a1[1]) == (0, 1, 1536, 512)
    assert (s0[6], s1[6], a0[6], a1[6]) == (2, 3, 512, 1536)
    # a shrink: 533 -> 416 keeps every tap inside the image
    s0, s1, a0, a1 = yr.linear_taps(533, 416)
    assert s0.min() == 0 and s1.max() == 532 and np.all(a0 + a1 == 2048) and np.all(s1 - s0 <= 1)


def test_blob_table():
    t = dk.blob_table()
    assert t.dtype == np.float32 and t.shape == (256,)
    for v in range(256):
        want = struct.unpack("<f", struct.pack("<f", float(v) * 0.00392))[0]  # (float)((double)v * 0.00392)
        assert float(t[v]) == want and float(yr.blob_value(v)) == want
    assert float(t[255]) != float(np.float32(1.0))  # cvlib's scale is not 1 / 255


# ---- cvlib's loop and NMSBoxes: the product's host tail and the restatement -------------------------------------
def _row(bx, by, bw, bh, cls, p, head=0, idx=0):
    return [head, idx, bx, by, bw, bh, 0.9, cls, p]


TAILS = [pytest.param(dk.nms_boxes, dk.cvlib_boxes, dk.detections, id="product"),
         pytest.param(yr.nms, yr.cvlib_loop, yr.detect, id="restatement")]


@pytest.mark.parametrize("nms, loop, detect", TAILS)
def test_nms_and_cvlib_loop(nms, loop, detect):
    # ties: equal scores stay in input order, and the earlier one wins an overlap
    far = [[0, 0, 10, 10], [100, 0, 10, 10], [200, 0, 10, 10]]
    assert nms(far, [0.5, 0.9, 0.5], 0.25, 0.3) == [1, 0, 2]
    assert nms([[0, 0, 10, 10], [1, 0, 10, 10]], [0.5, 0.5], 0.25, 0.3) == [0]
    assert nms([[1, 0, 10, 10], [0, 0, 10, 10]], [0.5, 0.5], 0.25, 0.3) == [0]
    # IoU exactly 0.3 (30 / (65 + 65 - 30)) is kept; one more column of overlap is not
    assert nms([[0, 0, 13, 5], [7, 0, 13, 5]], [0.9, 0.8], 0.25, 0.3) == [0, 1]
    assert nms([[0, 0, 13, 5], [6, 0, 13, 5]], [0.9, 0.8], 0.25, 0.3) == [0]
    # a score exactly at the confidence is dropped
    assert nms(far, [0.25, 0.2500001, 0.1], 0.25, 0.3) == [1]
    # int() truncates the products; x = cx - w / 2 keeps the half of an odd w
    rows = [_row(10.9 / 300, 20.99 / 168, 9.7 / 300, 4.2 / 168, 1, 0.8)]
    boxes, ids, scores = loop(rows, 300, 168)
    assert boxes == [[10 - 4.5, 20 - 2.0, 9, 4]] and ids == [1] and scores == [0.8]
    bbox, label, conf = detect(rows, 300, 168, ["a", "b"], 0.25, 0.3)
    assert bbox == [[5, 18, 14, 22]] and label == ["b"] and conf == [0.8]  # int(5.5), int(18.0), int(14.5), int(22.0)
    # a box hanging over the left edge: int() truncates towards zero
    rows = [_row(3.5 / 300, 2.5 / 168, 9.5 / 300, 7.5 / 168, 0, 0.6)]
    assert detect(rows, 300, 168, ["a", "b"], 0.25, 0.3)[0] == [[int(-1.5), int(-1.5), 7, 5]]
    assert int(-1.5) == -1
    assert detect([], 300, 168, ["a"], 0.25, 0.3) == ([], [], [])


def test_product_tail_equals_the_restatement_on_random_rows():
    rng = np.random.default_rng(5)
    for _ in range(20):
        k = int(rng.integers(1, 40))
        rows = np.column_stack([np.zeros(k), np.arange(k), rng.random(k), rng.random(k), rng.random(k) * 0.4,
                                rng.random(k) * 0.4, rng.random(k), rng.integers(0, 3, k),
                                np.round(rng.random(k), 2)]).astype(np.float32)
        assert dk.detections(rows, 300, 168, yr.MINI_CLASSES, 0.25, 0.3) == \
            yr.detect(rows.astype(np.float64), 300, 168, yr.MINI_CLASSES, 0.25, 0.3)


# ---- fm_yolo_create's refusals: host code, no device ------------------------------------------------------------
def _create(layers, params, **kw):
    L = _native.load()
    d, keep = _native.yolo_desc(layers, params, **{"net_w": 32, "net_h": 32, **kw})
    h = C.c_void_p()
    rc = L.fm_yolo_create(0, C.byref(d), C.byref(h))
    msg = L.fm_yolo_last_error(h).decode()
    assert h.value, "*out is set even on failure"
    L.fm_yolo_destroy(h)
    return rc, msg, (d, keep)


def _parsed():
    _, layers = dk.parse_cfg(CFG)
    return layers, dk.load_weights(dk.write_weights(layers, _raw_for(layers)), layers)


def test_create_refuses_inconsistent_descriptions_before_any_device_call():
    EINVAL = _native.FM_EINVAL
    layers, params = _parsed()
    # a route to a later layer, and to itself
    for src in ([9], [7], [1, 11]):
        bad = [dict(ly) for ly in layers]
        bad[7]["layers"] = src
        rc, msg, _ = _create(bad, params)
        assert rc == EINVAL and "layer 7: route" in msg, msg
    # a route joining two image sizes
    bad = [dict(ly) for ly in layers]
    bad[9]["layers"] = [8, 4]
    rc, msg, _ = _create(bad, params)
    assert rc == EINVAL and "layer 9: route joins" in msg, msg
    # channel counts that do not chain: a shortcut across 8 and 16 channels; weights cut for another Cin
    bad = [dict(ly) for ly in layers]
    bad[8] = {"kind": dk.SHORTCUT, "index": 8, "from": 5, "in_c": 16, "out_c": 16}
    rc, msg, _ = _create(bad, params)
    assert rc == EINVAL and "layer 8: shortcut adds" in msg, msg
    bad = [dict(ly) for ly in layers]
    bad[2]["filters"] = 9  # one more filter than its weights hold and than the shortcut after it takes
    rc, msg, _ = _create(bad, params)
    assert rc == EINVAL and ("layer 3: shortcut adds" in msg or "weights do not lie inside" in msg), msg
    short = list(params)
    short[10] = (params[10][0][:, :8], params[10][1])  # the last convolution's weights for 8 of its 16 inputs
    rc, msg, _ = _create(layers, short)
    assert rc == EINVAL and "layer 10" in msg and "weights do not lie inside" in msg, msg
    # a head whose filters != len(mask) * (classes + 5)
    bad = [dict(ly) for ly in layers]
    bad[11] = dict(layers[11], mask=[1, 2])
    rc, msg, _ = _create(bad, params)
    assert rc == EINVAL and "layer 11: head with 8 input channels" in msg and "= 16" in msg, msg
    # layer parameters outside the supported set
    for i, key, val, what in ((0, "size", 5, "layer 0: convolution"), (0, "stride", 3, "layer 0: convolution"),
                              (1, "size", 3, "layer 1: maxpool"), (4, "stride", 4, "layer 4: maxpool"),
                              (8, "stride", 3, "layer 8: upsample"), (0, "pad", 2, "layer 0: convolution")):
        bad = [dict(ly) for ly in layers]
        bad[i][key] = val
        rc, msg, _ = _create(bad, params)
        assert rc == EINVAL and what in msg, (i, key, msg)
    bad = [dict(ly) for ly in layers]
    bad[4]["kind"] = "dropout"
    rc, msg, _ = _create(bad, params)
    assert rc == EINVAL and "layer 4: unknown kind" in msg, msg
    # the scalars
    for kw in ({"net_w": 0}, {"max_frames": 0}, {"zero_thresh": 1.5}, {"zero_thresh": float("nan")}, {"channels": 0}):
        rc, msg, _ = _create(layers, params, **kw)
        assert rc == EINVAL and msg, (kw, msg)
    # activations past 2^31 elements
    rc, msg, _ = _create(layers[:1], [(params[0][0], params[0][1])], net_w=1 << 15, net_h=1 << 15, max_frames=4)
    assert rc == EINVAL and "2^31" in msg, msg
    L = _native.load()
    h = C.c_void_p(1)
    assert L.fm_yolo_create(0, None, C.byref(h)) == EINVAL and h.value
    assert b"null description" in L.fm_yolo_last_error(h)
    L.fm_yolo_destroy(h)
    assert L.fm_yolo_create(0, None, None) == EINVAL
    assert L.fm_yolo_last_error(None) == b"null detector"
    L.fm_yolo_destroy(None)
    for fn, args in ((L.fm_yolo_forward, (None, None, 1)), (L.fm_yolo_layer_output, (None, 0, None, 0)),
                     (L.fm_yolo_decode, (None, 1, 0.25, None, 0, None)), (L.fm_yolo_route_in_place, (None, 0)),
                     (L.fm_yolo_detect_frames, (None, None, 1, 8, 8, 0, 300, 0.25, None, 0, None, None)),
                     (L.fm_yolo_detect_frame_list, (None, None, 1, 8, 8, 300, 0.25, None, 0, None, None))):
        assert fn(*args) == EINVAL, fn


def test_description_matches_the_header_layout():
    layers, params = _parsed()
    d, keep = _native.yolo_desc(layers, params, net_w=32, net_h=32, max_frames=2)
    assert C.sizeof(_native.FMYoloLayer) == 56
    assert d.n_layers == 12 and d.classes == 3 and d.channels == 3 and d.n_anchors == 3 and d.max_frames == 2
    arr = keep[0]
    assert [arr[i].kind for i in range(12)] == [0, 1, 0, 4, 1, 0, 5, 3, 2, 3, 0, 5]
    assert (arr[9].src[0], arr[9].src[1]) == (8, 0) and (arr[7].src[0], arr[7].src[1]) == (4, -1)
    assert arr[3].src[0] == 1
    assert (arr[6].n_mask, arr[6].anchor_ofs, arr[11].n_mask, arr[11].anchor_ofs) == (2, 0, 1, 2)
    assert keep[3].tolist() == [[1, 2], [3, 4], [5, 6]]  # the masks applied, head by head
    assert arr[2].weight_ofs == 8 * 3 * 9 and arr[2].bias_ofs == 8 and arr[5].leaky == 0 and arr[0].leaky == 1
    assert d.n_weights == sum(p[0].size for p in params if p is not None)


# ---- the drop-in's wiring ------------------------------------------------------------------------------------
class FakeDetector:
    made = []

    def __init__(self, directory=None, tiny=False, device=0):
        self.directory, self.tiny, self.device = directory, tiny, device
        self.calls = []

    @classmethod
    def from_dir(cls, directory, tiny=False, device=0):
        d = cls(directory, tiny, device)
        cls.made.append(d)
        return d

    def detect_frames(self, src, width=300, confidence=0.25, nms=0.3):
        self.calls.append((np.asarray(src).shape, width, confidence))
        return [([[1, 2, 30, 40], [5, 6, 7, 8]], ["dog", "dog"], [0.9, 0.5])]


def _vm(tmp_path, n=40, **kw):
    W, H = 192, 108
    eng = OracleEngine(n_streams=1, src_w=W, src_h=H, box_size=100, ksize=5, threshold=12, avg=0.1, max_batch=4)
    return motion.VideoMotion(filename=str(tmp_path / "v"), capture=videoio.SyntheticCapture(W, H, n, 0), engine=eng,
                              batch=4, box_size=100, threshold=12, cache_time=0.3, min_time=0.1,
                              outdir=str(tmp_path), **kw)


def _cvlib_files(d, tiny):
    stem = "yolov3-tiny" if tiny else "yolov3"
    (d / f"{stem}.cfg").write_text("x")
    (d / f"{stem}.weights").write_bytes(b"x")
    (d / "yolov3_classes.txt").write_text("dog\n")


def test_find_objects_merges_yolo_labels_on_the_fifteenth_call_only(tmp_path, monkeypatch):
    monkeypatch.delenv("FM_YOLO_DIR", raising=False)
    monkeypatch.setattr(motion, "YoloDetector", FakeDetector)
    monkeypatch.setattr(motion, "_YOLOS", {})
    FakeDetector.made.clear()
    _cvlib_files(tmp_path, tiny=False)
    vm = _vm(tmp_path, yolo_dir=str(tmp_path))
    assert len(FakeDetector.made) == 1 and vm.yolo is FakeDetector.made[0]
    assert (vm.yolo.directory, vm.yolo.tiny, vm.yolo.device) == (str(tmp_path), False, 0)
    fr = SimpleNamespace(raw=np.zeros((108, 192, 3), np.uint8))
    for _ in range(14):
        assert vm.find_objects(fr) == set() and vm.yolo.calls == []
    assert vm.find_objects(fr) == {"dog"}
    assert vm.yolo.calls == [((1, 108, 192, 3), 300, 0.25)]
    assert vm.last_objects == {"dog": [((1, 2), (30, 40)), ((5, 6), (7, 8))]}  # make_area_from_box
    assert vm.find_objects(fr) == set() and len(vm.yolo.calls) == 1
    # a second stream on the same files shares the detector; the whole run collects the label
    vm2 = _vm(tmp_path, n=80, yolo_dir=str(tmp_path))
    assert vm2.yolo is vm.yolo and len(FakeDetector.made) == 1
    asked, inner = [], vm2.find_objects
    vm2.find_objects = lambda *a, **k: (asked.append(1), inner(*a, **k))[1]
    wrote, err, seen = vm2.find_motion()
    assert wrote and len(asked) >= 15 and seen == ("dog",)
    assert len(vm.yolo.calls) == 1 + len(asked) // 15


def test_without_a_directory_no_detector_is_touched(tmp_path, monkeypatch, caplog):
    class Untouchable:
        @classmethod
        def from_dir(cls, *a, **k):
            raise AssertionError("a detector was loaded without a yolo_dir")

    monkeypatch.delenv("FM_YOLO_DIR", raising=False)
    monkeypatch.setattr(motion, "YoloDetector", Untouchable)
    monkeypatch.setattr(motion, "_YOLOS", {})
    with caplog.at_level(logging.WARNING):
        vm = _vm(tmp_path)
        assert vm.yolo is None and vm.yolo_dir is None
        wrote, err, seen = vm.find_motion()
    assert wrote and seen == () and not [r for r in caplog.records if "YOLO" in r.getMessage()]
    # the environment supplies the default; an argument wins over it
    monkeypatch.setattr(motion, "YoloDetector", FakeDetector)
    FakeDetector.made.clear()
    d = tmp_path / "env"
    d.mkdir()
    _cvlib_files(d, tiny=False)
    monkeypatch.setenv("FM_YOLO_DIR", str(d))
    vm = _vm(tmp_path)
    assert vm.yolo_dir == str(d) and vm.yolo is FakeDetector.made[-1] and vm.yolo.directory == str(d)
    assert _vm(tmp_path, yolo_dir=str(tmp_path / "nowhere")).yolo is None
    assert inspect_default("yolo_dir") is None


def inspect_default(name):
    import inspect
    p = inspect.signature(motion.VideoMotion.__init__).parameters[name]
    assert p.kind is p.KEYWORD_ONLY
    return p.default


def test_tiny_flag_selects_the_tiny_pair_and_missing_or_refused_files_leave_the_stage_off(tmp_path, monkeypatch, caplog):
    monkeypatch.delenv("FM_YOLO_DIR", raising=False)
    monkeypatch.setattr(motion, "YoloDetector", FakeDetector)
    monkeypatch.setattr(motion, "_YOLOS", {})
    FakeDetector.made.clear()
    _cvlib_files(tmp_path, tiny=True)  # only yolov3-tiny.cfg / .weights
    with caplog.at_level(logging.WARNING):
        vm = _vm(tmp_path, yolo_dir=str(tmp_path))
    assert vm.yolo is None and FakeDetector.made == []
    assert any("yolov3.cfg" in r.getMessage() and "skipped" in r.getMessage() for r in caplog.records)
    vm = _vm(tmp_path, yolo_dir=str(tmp_path), yolo_tiny=True)
    assert vm.yolo is not None and vm.yolo.tiny is True
    # the real loader on files it refuses: a warning, the stage off, the run as without it
    monkeypatch.setattr(motion, "YoloDetector", _native.YoloDetector)
    monkeypatch.setattr(motion, "_YOLOS", {})
    (tmp_path / "yolov3-tiny.cfg").write_text("[net]\nwidth=8\n[dropout]\nprobability=.5\n")
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        vm = _vm(tmp_path, yolo_dir=str(tmp_path), yolo_tiny=True)
    assert vm.yolo is None
    assert any("refused" in r.getMessage() and "[dropout]" in r.getMessage() for r in caplog.records)
    wrote, err, seen = vm.find_motion()
    assert wrote and seen == ()


def test_cli_flag_and_ini_setting(tmp_path):
    parser = ArgumentParser()
    cli.get_args(parser)
    args = parser.parse_args(["x.avi"])
    assert args.yolo_dir is None and cli._job_kwargs(args)["yolo_dir"] is None
    args = parser.parse_args(["x.avi", "--yolo-dir", "/models", "--yolo-tiny"])
    kw = cli._job_kwargs(args)
    assert kw["yolo_dir"] == "/models" and kw["yolo_tiny"] is True
    ini = tmp_path / "c.ini"
    ini.write_text("[settings]\nyolo-dir = /from/ini\nyolo_tiny = True\n")
    args = cli.process_config(str(ini), parser.parse_args(["x.avi"]))
    assert args.yolo_dir == "/from/ini" and args.yolo_tiny is True


# ---- the two real topologies from the shared generators, and the exact convolution reference ---------------------
def _param_count(layers):
    """Floats of a .weights file after its header: weights + (beta, gamma, mean, var) or the bias."""
    return sum(ly["filters"] * ly["in_c"] * ly["size"] ** 2 + (4 if ly["batch_normalize"] else 1) * ly["filters"]
               for ly in layers if ly["kind"] == dk.CONV)


TOPOLOGIES = [
    pytest.param(yr.full_cfg, 107, 75, 23, 62001757, 248007048, {83: [79], 86: [85, 61], 95: [91], 98: [97, 36]},
                 {82: 13, 94: 26, 106: 52}, 10647, id="yolov3"),
    pytest.param(yr.tiny_cfg, 24, 13, 0, 8858734, 35434956, {17: [13], 20: [19, 8]}, {16: 13, 23: 26}, 2535,
                 id="yolov3-tiny"),
]


@pytest.mark.parametrize("gen, n_layers, n_convs, n_shortcuts, n_params, n_bytes, routes, heads, rows", TOPOLOGIES)
def test_real_topology_known_answers(gen, n_layers, n_convs, n_shortcuts, n_params, n_bytes, routes, heads, rows):
    net, layers = dk.parse_cfg(gen())
    assert (net["width"], net["height"], net["channels"]) == ("416", "416", "3")
    convs = [ly for ly in layers if ly["kind"] == dk.CONV]
    assert len(layers) == n_layers and len(convs) == n_convs
    assert sum(ly["kind"] == dk.SHORTCUT for ly in layers) == n_shortcuts
    assert _param_count(layers) == n_params
    assert max(ly["in_c"] * ly["size"] ** 2 for ly in convs) == 4608 and max(ly["filters"] for ly in convs) == 1024
    assert {ly["index"]: ly["layers"] for ly in layers if ly["kind"] == dk.ROUTE} == routes
    shapes = yr.layer_shapes(layers, 416, 416)
    ys = [ly for ly in layers if ly["kind"] == dk.YOLO]
    assert {ly["index"]: shapes[ly["index"]] for ly in ys} == {i: (255, g, g) for i, g in heads.items()}
    assert all(ly["classes"] == 80 and len(ly["mask"]) == 3 for ly in ys)
    assert sum(len(ly["mask"]) * shapes[ly["index"]][1] * shapes[ly["index"]][2] for ly in ys) == rows
    # every head's convolution is linear, without batch norm, 255 wide; every other one leaky with batch norm
    for ly in convs:
        head = layers[ly["index"] + 1]["kind"] == dk.YOLO
        assert (ly["activation"], ly["batch_normalize"]) == (("linear", 0) if head else ("leaky", 1)), ly["index"]
        assert not head or (ly["filters"], ly["size"]) == (255, 1)
    # the file write_weights makes of it: the 20-byte header and every parameter, and load_weights takes it back
    raw = {ly["index"]: tuple(np.zeros(k, np.float32) for k in
                              ([ly["filters"]] * (4 if ly["batch_normalize"] else 1)
                               + [ly["filters"] * ly["in_c"] * ly["size"] ** 2])) for ly in convs}
    data = dk.write_weights(layers, raw)
    del raw
    assert len(data) == n_bytes == 20 + 4 * n_params
    del data


def test_real_topology_generators_take_classes_and_size():
    for gen, n_heads in ((yr.full_cfg, 3), (yr.tiny_cfg, 2)):
        net, layers = dk.parse_cfg(gen(classes=3, width=96, height=64))
        assert (net["width"], net["height"]) == ("96", "64")
        ys = [ly for ly in layers if ly["kind"] == dk.YOLO]
        assert len(ys) == n_heads and all(ly["classes"] == 3 and ly["in_c"] == 24 for ly in ys)
        shapes = yr.layer_shapes(layers, 96, 64)
        assert [shapes[ly["index"]][1:] for ly in ys] == [(2, 3), (4, 6), (8, 12)][:n_heads]
    # the shapes the walk gives are fm_yolo_create's own: a route joining what it says are equal sizes is accepted,
    # and an odd size through tiny's stride-2 pools rounds up
    _, layers = dk.parse_cfg(yr.tiny_cfg(classes=1, width=72, height=40))
    assert yr.layer_shapes(layers, 72, 40)[11] == (512, 2, 3) and yr.layer_shapes(layers, 72, 40)[9] == (256, 2, 3)


@pytest.mark.parametrize("cin, cout, size, stride, h, w", [(5, 7, 3, 1, 4, 6), (6, 9, 3, 2, 5, 7), (6, 9, 3, 2, 6, 4),
                                                          (8, 3, 1, 1, 3, 5), (4, 4, 3, 1, 1, 1)])
def test_conv_exact_equals_the_float64_convolution_on_integers(cin, cout, size, stride, h, w):
    rng = np.random.default_rng(cin * 10 + cout)
    x = rng.integers(-3, 4, (2, cin, h, w))
    wt = rng.integers(-2, 3, (cout, cin, size, size))
    b = rng.integers(-8, 9, cout)
    want, wmag = yr.conv(x, wt, b, stride, size // 2, False)
    for args in ((x, wt, b), (x.astype(np.float32), wt.astype(np.float32), b.astype(np.float32))):
        got, mag = yr.conv_exact(*args, stride, size // 2, False)
        assert got.dtype == np.float32 and mag.dtype == np.int64
        assert got.shape == want.shape and np.array_equal(got, want) and np.array_equal(mag, wmag)
    assert (want < 0).any() and (want >= 0).any()
    # leaky: the values that are not negative as they were, a negative one times f32 0.1 with one rounding
    leaky, lmag = yr.conv_exact(x, wt, b, stride, size // 2, True)
    assert leaky.dtype == np.float32 and np.array_equal(lmag, mag)
    neg = want < 0
    assert np.array_equal(leaky[~neg], want[~neg])
    assert np.array_equal(leaky[neg], np.float32(0.1) * want[neg].astype(np.float32))
    assert float(np.float32(0.1)) != 0.1  # (so that the line above is not the float64 product)
    w64, _ = yr.conv(x, wt, b, stride, size // 2, True)
    assert np.all(np.abs(leaky - w64) <= 2 * yr.U * np.abs(w64))


def test_conv_exact_refuses_what_breaks_its_condition():
    x = np.full((1, 2, 3, 3), 3)
    w = np.full((1, 2, 3, 3), 2)
    b = np.array([8])
    out, mag = yr.conv_exact(x, w, b, 1, 1, False)
    assert int(mag.max()) == 2 * 9 * 6 + 8 == int(out.max())
    # a magnitude sum of exactly 2^24 is refused, one below it is taken, whatever the sign of the terms
    big = (1 << 24) - 8
    for sign in (1, -1):
        x1 = np.array([[[[sign * big]]]])
        with pytest.raises(AssertionError, match="2\\^24"):
            yr.conv_exact(x1, np.array([[[[1]]]]), np.array([8]), 1, 0, False)
        out, mag = yr.conv_exact(x1, np.array([[[[1]]]]), np.array([7 * sign]), 1, 0, False)
        assert int(mag[0, 0, 0, 0]) == (1 << 24) - 1 and float(out[0, 0, 0, 0]) == sign * ((1 << 24) - 1)
    # terms that cancel in the result still count
    with pytest.raises(AssertionError, match="2\\^24"):
        yr.conv_exact(np.array([[[[1 << 23]], [[1 << 23]]]]), np.array([[[[1]], [[-1]]]]), np.array([0]), 1, 0, False)
    # values that are no integers
    for bad in ((x + 0.5, w, b), (x, w * 0.25, b), (x, w, b + 0.1)):
        with pytest.raises(AssertionError, match="integer"):
            yr.conv_exact(*bad, 1, 1, False)
    # and forward_exact holds a shortcut's sum to the same
    body = [yr.conv_cfg(1, 1, 1, "linear", 0), "[shortcut]\nfrom=-1\nactivation=linear\n"]
    _, layers = dk.parse_cfg(yr.net_cfg(1, body, 1, 1))
    params = [(np.ones((1, 1, 1, 1)), np.zeros(1)), None]
    outs = yr.forward_exact(layers, params, np.full((1, 1, 1, 1), (1 << 23) - 1))
    assert outs[1].dtype == np.float32 and float(outs[1][0, 0, 0, 0]) == (1 << 24) - 2
    with pytest.raises(AssertionError, match="shortcut"):
        yr.forward_exact(layers, params, np.full((1, 1, 1, 1), 1 << 23))
