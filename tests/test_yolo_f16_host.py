"""The YOLOv3 stage's f16 mode (FM_YOLO_F16) without a GPU: the two new entry points and their
refusals (host code that runs before any HIP call), the drop-in's wiring of `yolo_precision`, and known answers
of the numpy restatement tests/yolo_ref16.py that the GPU tests compare with."""
import ctypes as C
import os
import re
from argparse import ArgumentParser

import numpy as np
import pytest

import yolo_ref as yr
import yolo_ref16 as y16
from fake_engine import OracleEngine
from find_motion_amd import _native, cli, motion, videoio
from find_motion_amd import darknet as dk

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "find_motion_amd.h")


def _lin(filters, size, stride=1):
    return yr.conv_cfg(filters, size, stride, "linear", bn=0)


# ---- the C ABI -------------------------------------------------------------------------------------------------
def test_precision_entry_points_are_declared_and_exported():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"^#define FM_YOLO_F32 0$", text, re.M) and re.search(r"^#define FM_YOLO_F16 1$", text, re.M)
    assert re.search(r"int fm_yolo_create_precision\(int device, const fm_yolo_desc\* desc, int precision, fm_yolo\*\* out\);", text)
    assert re.search(r"int fm_yolo_precision\(const fm_yolo\* det\);", text)
    assert {"fm_yolo_create_precision", "fm_yolo_precision"} <= set(_native.EXPORTED)
    L = _native.load()
    assert L.fm_yolo_create_precision and L.fm_yolo_precision
    assert _native.YOLO_PRECISIONS == {"f32": 0, "f16": 1}
    assert L.fm_yolo_precision(None) == _native.FM_EINVAL


def _create(layers, params, precision, device=0, **kw):
    """(code, message, fm_yolo_precision) of a create that some host check refuses: like fm_yolo_create's own
    refusals these come before the first HIP call, and this file runs where there is no device."""
    L = _native.load()
    d, keep = _native.yolo_desc(layers, params, **{"net_w": 16, "net_h": 16, **kw})
    h = C.c_void_p()
    rc = L.fm_yolo_create_precision(device, C.byref(d), precision, C.byref(h))
    msg = L.fm_yolo_last_error(h).decode()
    assert h.value, "*out is set even on failure"
    prec = L.fm_yolo_precision(h)
    L.fm_yolo_destroy(h)
    return rc, msg, prec


def _two_convs(cin=4, cout=6):
    """Two convolutions, then a route that reads a head's convolution: FM_YOLO_F16 refuses that (the last of
    its host checks), so a description that gets this far has passed the checks before it."""
    body = [_lin(cout, 3), yr.conv_cfg(24, 1, 1, "linear", bn=0), yr.yolo_cfg("0,1,2"), "[route]\nlayers=1\n"]
    _, layers = dk.parse_cfg(yr.net_cfg(cin, body, 16, 16))
    rng = np.random.default_rng(0)
    params = [(rng.integers(-2, 3, (cout, cin, 3, 3)).astype(np.float32), np.zeros(cout, np.float32)),
              (rng.integers(-2, 3, (24, cout, 1, 1)).astype(np.float32), np.zeros(24, np.float32)), None, None]
    return layers, params


LAST_CHECK = "layer 3: in f16 only a head reads layer 1"


def test_unknown_precision_is_refused_before_any_device_call():
    layers, params = _two_convs()
    for bad in (2, -1, 16):
        rc, msg, _ = _create(layers, params, bad)
        assert rc == _native.FM_EINVAL and f"precision {bad}" in msg, msg
    # the two known ones pass that check: the next one refuses the device ordinal
    for good in (0, 1):
        rc, msg, prec = _create(layers, params, good, device=-1)
        assert rc == _native.FM_EINVAL and msg == "device -1" and prec == good, msg
    L = _native.load()
    assert L.fm_yolo_create_precision(0, None, 1, None) == _native.FM_EINVAL
    with pytest.raises(ValueError, match="precision"):
        _native.YoloDetector(layers, params, [], precision="bf16")


def test_f16_refuses_a_weight_outside_the_half_range_and_names_its_layer():
    layers, params = _two_convs()
    rc, msg, _ = _create(layers, params, 1)
    assert rc == _native.FM_ENOTSUP and msg.startswith(LAST_CHECK), msg
    for value in (1e5, -70000.0, 65520.0, float("inf"), float("nan")):
        bad = list(params)
        bad[1] = (params[1][0].copy(), params[1][1])
        bad[1][0][3, 2, 0, 0] = value
        rc, msg, _ = _create(layers, bad, 1)
        assert rc == _native.FM_ENOTSUP and msg.startswith("layer 1: weight 20 ") and "f16" in msg, (value, msg)
    # 65519 rounds to 65504, the largest half: not refused, the checks go on
    ok = list(params)
    ok[0] = (params[0][0].copy(), params[0][1])
    ok[0][0][0, 0, 0, 0] = -65519.0
    rc, msg, _ = _create(layers, ok, 1)
    assert rc == _native.FM_ENOTSUP and msg.startswith(LAST_CHECK), msg


def test_f16_refuses_readers_of_a_heads_f32_tensor():
    body = [yr.conv_cfg(24, 1, 1, "linear", bn=0), yr.yolo_cfg("0,1,2"), "[route]\nlayers=0\n",
            "[maxpool]\nsize=2\nstride=2\n", yr.yolo_cfg("3,4,5")]
    _, layers = dk.parse_cfg(yr.net_cfg(24, body, 8, 8))
    params = [None] * len(layers)
    params[0] = (np.eye(24, dtype=np.float32).reshape(24, 24, 1, 1), np.zeros(24, np.float32))
    rc, msg, _ = _create(layers, params, 1, net_w=8, net_h=8)
    assert rc == _native.FM_ENOTSUP and msg.startswith("layer 4: in f16 a head reads a convolution"), msg
    rc, msg, _ = _create(layers[:3], params[:3], 1, net_w=8, net_h=8)
    assert rc == _native.FM_ENOTSUP and msg.startswith("layer 2: in f16 only a head reads layer 0"), msg


# ---- the drop-in's wiring -----------------------------------------------------------------------------------------
class FakeDetector:
    made = []

    def __init__(self, directory, tiny, device, precision):
        self.directory, self.tiny, self.device, self.precision = directory, tiny, device, precision

    @classmethod
    def from_dir(cls, directory, tiny=False, device=0, precision="f32"):
        d = cls(directory, tiny, device, precision)
        cls.made.append(d)
        return d

    def detect_frames(self, src, width=300, confidence=0.25, nms=0.3):
        return [([], [], [])]


def _vm(tmp_path, **kw):
    W, H = 192, 108
    eng = OracleEngine(n_streams=1, src_w=W, src_h=H, box_size=100, ksize=5, threshold=12, avg=0.1, max_batch=4)
    return motion.VideoMotion(filename=str(tmp_path / "v"), capture=videoio.SyntheticCapture(W, H, 8, 0), engine=eng,
                              batch=4, box_size=100, threshold=12, cache_time=0.3, min_time=0.1,
                              outdir=str(tmp_path), **kw)


def _cvlib_files(d):
    (d / "yolov3.cfg").write_text("x")
    (d / "yolov3.weights").write_bytes(b"x")
    (d / "yolov3_classes.txt").write_text("dog\n")


def test_yolos_cache_keeps_the_precisions_apart_and_the_environment_gives_the_default(tmp_path, monkeypatch, caplog):
    import logging
    monkeypatch.delenv("FM_YOLO_DIR", raising=False)
    monkeypatch.delenv("FM_YOLO_PRECISION", raising=False)
    monkeypatch.setattr(motion, "YoloDetector", FakeDetector)
    monkeypatch.setattr(motion, "_YOLOS", {})
    FakeDetector.made.clear()
    _cvlib_files(tmp_path)
    a = _vm(tmp_path, yolo_dir=str(tmp_path))
    with caplog.at_level(logging.INFO, logger="find_motion_amd.VideoMotion"):
        b = _vm(tmp_path, yolo_dir=str(tmp_path), yolo_precision="f16")
    assert any("YOLO" in r.getMessage() and "f16" in r.getMessage() for r in caplog.records)
    c = _vm(tmp_path, yolo_dir=str(tmp_path), yolo_precision="f16")
    d = _vm(tmp_path, yolo_dir=str(tmp_path), yolo_precision="f32")
    assert (a.yolo_precision, b.yolo_precision) == ("f32", "f16")
    assert [m.precision for m in FakeDetector.made] == ["f32", "f16"]
    assert a.yolo is d.yolo and b.yolo is c.yolo and a.yolo is not b.yolo
    assert len(motion._YOLOS) == 2 and {k[-1] for k in motion._YOLOS} == {"f32", "f16"}
    # the environment supplies the default; an argument wins over it
    monkeypatch.setenv("FM_YOLO_PRECISION", "f16")
    assert _vm(tmp_path, yolo_dir=str(tmp_path)).yolo is b.yolo
    assert _vm(tmp_path, yolo_dir=str(tmp_path), yolo_precision="f32").yolo is a.yolo
    assert _vm(tmp_path).yolo_precision == "f16"
    monkeypatch.setenv("FM_YOLO_PRECISION", "")
    assert _vm(tmp_path).yolo_precision == "f32"
    with pytest.raises(ValueError, match="yolo_precision"):
        _vm(tmp_path, yolo_precision="f64")
    import inspect
    p = inspect.signature(motion.VideoMotion.__init__).parameters["yolo_precision"]
    assert p.kind is p.KEYWORD_ONLY and p.default is None


def test_cli_flag_and_ini_setting_reach_video_motion(tmp_path):
    parser = ArgumentParser()
    cli.get_args(parser)
    args = parser.parse_args(["x.avi"])
    assert args.yolo_precision is None and cli._job_kwargs(args)["yolo_precision"] is None
    args = parser.parse_args(["x.avi", "--yolo-precision", "f16"])
    assert cli._job_kwargs(args)["yolo_precision"] == "f16"
    with pytest.raises(SystemExit):
        parser.parse_args(["x.avi", "--yolo-precision", "f8"])
    ini = tmp_path / "c.ini"
    ini.write_text("[settings]\nyolo-precision = f16\n")
    args = cli.process_config(str(ini), parser.parse_args(["x.avi"]))
    assert args.yolo_precision == "f16" and cli._job_kwargs(args)["yolo_precision"] == "f16"
    ini.write_text("[settings]\nyolo_precision = half\n")
    with pytest.raises(ValueError, match="yolo_precision"):
        cli.process_config(str(ini), parser.parse_args(["x.avi"]))
    # _job_kwargs' dictionary is what VideoMotion (and StreamGroup, which hands its kwargs on) is called with
    import inspect
    assert "yolo_precision" in inspect.signature(motion.VideoMotion.__init__).parameters
    assert inspect.signature(motion.StreamGroup.__init__).parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD


# ---- yolo_ref16's known answers ---------------------------------------------------------------------------------
INT_NET = [_lin(8, 3),                                   # 0
           "[maxpool]\nsize=2\nstride=2\n",               # 1
           _lin(8, 1),                                   # 2
           _lin(8, 3),                                   # 3
           "[shortcut]\nfrom=-3\nactivation=linear\n",    # 4
           "[upsample]\nstride=2\n",                      # 5
           "[route]\nlayers = -1, 0\n",                   # 6
           _lin(5, 3, 2)]                                # 7


def _sparse_int_params(layers, seed, taps):
    rng = np.random.default_rng(seed)
    params = [None] * len(layers)
    for ly in layers:
        if ly["kind"] != dk.CONV:
            continue
        shape = (ly["filters"], ly["in_c"], ly["size"], ly["size"])
        K = ly["in_c"] * ly["size"] ** 2
        wt = (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < min(1.0, taps / K))
        params[ly["index"]] = (wt.astype(np.float32), rng.integers(-2, 3, ly["filters"]).astype(np.float32))
    return params


@pytest.mark.parametrize("acc", ["exact", "chain"])
def test_forward16_equals_forward_exact_on_small_integer_networks(acc):
    """Integers of magnitude <= 2048 are halves, and with linear activations every value of the f16 mode is then
    the exact one: the restatement must reproduce yolo_ref.forward_exact bit for bit in either order."""
    _, layers = dk.parse_cfg(yr.net_cfg(3, INT_NET, 10, 6))
    params = _sparse_int_params(layers, seed=5, taps=4)
    x = np.random.default_rng(1).integers(-3, 4, (2, 3, 6, 10)).astype(np.float32)
    want = yr.forward_exact(layers, params, x)
    assert max(float(np.abs(w).max()) for w in want) <= 2048 and float(np.abs(want[-1]).max()) >= 8
    got = y16.forward16(layers, params, x, acc)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float16 and g.shape == w.shape, i
        assert np.array_equal(g.astype(np.float32), w), f"layer {i} ({layers[i]['kind']})"


def test_restatement_known_answers():
    # the clamp: the largest half on either side, never an infinity; and round to nearest even below it
    v = np.array([65504.0, 65519.9, 65520.0, 1e6, -1e6, np.inf, -np.inf, 2049.0, 2051.0, 1.0 + 2.0 ** -11], np.float32)
    assert y16.to_half(v).tolist() == [65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0, 2048.0, 2052.0, 1.0]
    # a convolution that saturates: 9 taps of 8 x 1000 = 72000, and its negative through leaky = -7200
    x = np.full((1, 1, 3, 3), 8.0, np.float32)
    w = np.stack([np.full((1, 3, 3), 1000.0, np.float32), np.full((1, 3, 3), -1000.0, np.float32)])
    b = np.zeros(2, np.float32)
    for acc in ("exact", "chain"):
        out = y16.conv16(x, w, b, 1, 1, True, acc)
        assert out.dtype == np.float16 and out[0, :, 1, 1].tolist() == [65504.0, -7200.0]
        lin = y16.conv16(x, w, b, 1, 1, False, acc)
        assert lin[0, :, 1, 1].tolist() == [65504.0, -65504.0]
        head = y16.conv16(x, w, b, 1, 1, False, acc, head=True)
        assert head.dtype == np.float32 and head[0, :, 1, 1].tolist() == [72000.0, -72000.0]
    got, _ = y16.conv_exact16(x, w, b, 1, 1, True)
    assert got.dtype == np.float16 and got[0, :, 1, 1].tolist() == [65504.0, -7200.0]
    # a shortcut: one f32 add of the two stored halves, then one rounding to f16, ties to even
    assert float(y16.shortcut16(np.float16(2048.0), np.float16(3.0))) == 2052.0
    assert float(y16.shortcut16(np.float16(2048.0), np.float16(1.0))) == 2048.0     # the tie goes to even
    assert float(y16.shortcut16(np.float16(2050.0), np.float16(1.0))) == 2052.0     # and up to even here
    assert float(y16.shortcut16(np.float16(60000.0), np.float16(60000.0))) == 65504.0
    # Double rounding: two halves 35 binary places apart make the f32 add itself round (1024 + 2^-14 (1 + 2^-10)
    # needs 35 bits), and the f16 rounding follows.  That cannot move the result: a sum of two halves that lies
    # within 2^-24 (relative) of an f16 tie without being that tie would need more than 11 significant bits in
    # one of them.  So the mode's shortcut equals the single rounding of the exact sum (float64 holds it),
    # on the crafted pair, on the pairs around a tie, and on a seeded sample of all magnitudes:
    small = np.float16(2.0 ** -14 * (1 + 2.0 ** -10))
    assert np.float32(1024.0) + np.float32(small) != np.float64(1024.0) + np.float64(small)  # the f32 add rounds
    assert float(y16.shortcut16(np.float16(1024.0), small)) == 1024.0
    tie = [(1.0, 2.0 ** -11), (1.0, 2.0 ** -11 + 2.0 ** -21), (1.0, 2.0 ** -11 - 2.0 ** -22), (1.0 + 2.0 ** -10, 2.0 ** -11),
           (4100.0, -1.9990234375), (32800.0, 16.015625), (-1.0, -(2.0 ** -11)), (1.0, 2.0 ** -24), (6e-5, 6e-8)]
    rng = np.random.default_rng(16)
    a = np.concatenate([np.array([t[0] for t in tie]), rng.standard_normal(100000) * 2.0 ** rng.integers(-14, 13, 100000)])
    b = np.concatenate([np.array([t[1] for t in tie]), rng.standard_normal(100000) * 2.0 ** rng.integers(-14, 13, 100000)])
    a, b = a.astype(np.float16), b.astype(np.float16)
    once = np.clip(a.astype(np.float64) + b.astype(np.float64), -65504.0, 65504.0).astype(np.float16)
    assert np.array_equal(y16.shortcut16(a, b).view(np.uint16), once.view(np.uint16))
    assert float(y16.shortcut16(np.float16(1.0), np.float16(2.0 ** -11 + 2.0 ** -21))) == 1.0 + 2.0 ** -10
    # weights round once, biases stay f32, subnormal halves go only when asked
    hp = y16.half_params([(np.array([0.1, 3e-5, 2049.0], np.float32), np.array([0.1], np.float32)), None])
    assert hp[1] is None and hp[0][1][0] == np.float32(0.1)
    assert hp[0][0].tolist() == [float(np.float16(0.1)), float(np.float16(3e-5)), 2048.0] and hp[0][0][1] != 0
    assert y16.half_params([(np.array([3e-5], np.float32), np.zeros(1, np.float32))], True)[0][0].tolist() == [0.0]


def test_head_convolutions_stay_f32_in_the_restatement():
    cfg, weights, layers, params = yr.mini_net()
    x = np.random.default_rng(3).random((1, 3, 64, 64)).astype(np.float32)
    outs = y16.forward16(layers, params, x)
    kinds = [o.dtype for o in outs]
    assert [i for i, k in enumerate(kinds) if k == np.float32] == [9, 10, 15, 16]
    assert all(k == np.float16 for i, k in enumerate(kinds) if i not in (9, 10, 15, 16))
    assert outs[10] is outs[9] or np.array_equal(outs[10], outs[9])
