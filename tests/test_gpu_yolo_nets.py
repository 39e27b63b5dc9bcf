"""The YOLOv3 object stage (fm_yolo_*) on the real topologies and on exact convolutions.

1. Convolutions of small integers at the real channel counts (K up to 4608, Cout up to 1024): every magnitude sum
   stays below 2^24, so every partial sum of the f32 fma chain is an exact integer in whatever order it is taken,
   and the output must equal the int64 reference bit for bit -- one dropped, doubled or stale k-tile, or one wrong
   tap, shows.
2. Convolutions that write into an in-place route's buffer and that read such a view, in yolov3-tiny's pattern and
   in yolov3's, exact in the same way.
3. yolov3 and yolov3-tiny themselves (107 and 24 layers, 80 classes) on small inputs with seeded weights: every
   layer on the GPU's own inputs, the head tensors and the decoded rows against the float64 restatement.
4. The decode's comparisons on crafted head tensors: scores exactly at a threshold, ties, the first and the last
   class, saturated boxes, every row passing, none passing.
Weights are seeded or constructed; nothing is read from a fixture."""
import functools

import numpy as np
import pytest

import yolo_ref as yr
from find_motion_amd import YoloDetector
from find_motion_amd import darknet as dk
from test_gpu_yolo import _check_layer

pytestmark = pytest.mark.gpu

CLASSES80 = [f"c{i}" for i in range(80)]


def _exact(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, the first at "
                           f"{tuple(int(i) for i in np.argwhere(bad)[0])}: {got[bad][0]!r}, exact {want[bad][0]!r}")


# ---- 1. exact convolutions -------------------------------------------------------------------------------------
EXACT_CONVS = [  # cin, cout, size, stride, h, w
    pytest.param(512, 1024, 3, 1, 3, 2, id="512-1024-3x3-2x3-K4608"),
    pytest.param(512, 1024, 3, 2, 5, 4, id="512-1024-3x3-s2-4x5"),
    pytest.param(1024, 512, 1, 1, 3, 5, id="1024-512-1x1-5x3"),
    pytest.param(768, 256, 1, 1, 4, 6, id="768-256-1x1-6x4"),
    pytest.param(384, 256, 3, 1, 4, 3, id="384-256-3x3-3x4-K3456"),
    pytest.param(1024, 255, 1, 1, 13, 13, id="1024-255-1x1-13x13-head"),
    pytest.param(3, 32, 3, 1, 33, 47, id="3-32-3x3-47x33-K27"),
    pytest.param(3, 16, 3, 1, 20, 36, id="3-16-3x3-36x20"),
    pytest.param(32, 64, 3, 2, 15, 17, id="32-64-3x3-s2-17x15"),
] + [pytest.param(20, cout, 3, 1, 7, 9, id=f"20-{cout}-3x3-9x7") for cout in (31, 32, 33, 64, 65)]


@pytest.mark.parametrize("act", ["linear", "leaky"])
@pytest.mark.parametrize("cin, cout, size, stride, h, w", EXACT_CONVS)
def test_conv_layer_of_integers_is_bit_exact(cin, cout, size, stride, h, w, act):
    _, layers = dk.parse_cfg(yr.net_cfg(cin, [yr.conv_cfg(cout, size, stride, act, bn=0)], w, h))
    rng = np.random.default_rng(cin * 4096 + cout * 2 + stride)
    wt = rng.integers(-2, 3, (cout, cin, size, size)).astype(np.float32)
    b = rng.integers(-8, 9, cout).astype(np.float32)
    det = YoloDetector(layers, [(wt, b)], [], net_w=w, net_h=h, max_frames=3)
    for n in (1, 3):
        x = rng.integers(-3, 4, (n, cin, h, w)).astype(np.float32)
        want, mag = yr.conv_exact(x, wt, b, stride, size // 2, act == "leaky")
        assert int(mag.max()) <= 6 * cin * size * size + 8
        assert (want < 0).any() and (want > 0).any()
        det.forward(x)
        _exact(det.layer_output(0, n), want, f"n = {n}")
    det.close()


# ---- 2. convolutions in and behind in-place routes --------------------------------------------------------------
def _sparse_int_params(layers, seed, taps):
    """Weights in {-1, 0, 1} with about `taps` non-zero ones per output (so that values grow by a small factor
    per layer and a chain of layers stays below 2^24), biases in [-2, 2]."""
    rng = np.random.default_rng(seed)
    params = [None] * len(layers)
    for ly in layers:
        if ly["kind"] != dk.CONV:
            continue
        shape = (ly["filters"], ly["in_c"], ly["size"], ly["size"])
        K = ly["in_c"] * ly["size"] ** 2
        wt = rng.integers(0, 2, shape) * 2 - 1
        wt = wt * (rng.random(shape) < min(1.0, taps / K))
        params[ly["index"]] = (wt.astype(np.float32), rng.integers(-2, 3, ly["filters"]).astype(np.float32))
    return params


def _lin(filters, size, stride=1):
    return yr.conv_cfg(filters, size, stride, "linear", bn=0)


TINY_PATTERN = [_lin(11, 3),                          # 0  writes channels 7..17 of the route's buffer
                "[maxpool]\nsize=2\nstride=2\n",       # 1  reads that view
                _lin(7, 1),                           # 2
                "[upsample]\nstride=2\n",              # 3  writes channels 0..6
                "[route]\nlayers = -1, 0\n",           # 4  in place
                _lin(13, 3)]                          # 5
FULL_PATTERN = [_lin(16, 3),                          # 0
                _lin(8, 1),                           # 1
                _lin(16, 3),                          # 2
                "[shortcut]\nfrom=-3\nactivation=linear\n",   # 3  writes channels 12..27 of route 10's buffer
                _lin(24, 3, 2),                       # 4  stride 2 over that view (in_bs wider than Cin H W)
                _lin(12, 1),                          # 5
                _lin(24, 3),                          # 6
                "[shortcut]\nfrom=-3\nactivation=linear\n",   # 7  the second residual block
                _lin(12, 1),                          # 8
                "[upsample]\nstride=2\n",              # 9  writes channels 0..11
                "[route]\nlayers = -1, 3\n",           # 10 in place
                _lin(16, 1),                          # 11
                "[shortcut]\nfrom=3\nactivation=linear\n",    # 12 its `from` is the view
                _lin(9, 3)]                           # 13
ROUTE_NETS = [pytest.param(TINY_PATTERN, 4, id="tiny-route-1-0"),
              pytest.param(FULL_PATTERN, 10, id="yolov3-route-1-shortcut")]


@pytest.mark.parametrize("body, route", ROUTE_NETS)
def test_convolutions_in_and_behind_in_place_routes_are_bit_exact(body, route):
    cin, w, h = 5, 10, 6
    _, layers = dk.parse_cfg(yr.net_cfg(cin, body, w, h))
    params = _sparse_int_params(layers, seed=len(body), taps=6)
    det = YoloDetector(layers, params, [], net_w=w, net_h=h, max_frames=3)
    assert det.route_in_place(route)
    rng = np.random.default_rng(route)
    for n in (1, 3):
        x = rng.integers(-3, 4, (n, cin, h, w)).astype(np.float32)
        want = yr.forward_exact(layers, params, x)  # asserts the 2^24 condition at every layer
        det.forward(x)
        got = [det.layer_output(i, n) for i in range(len(layers))]
        for i in range(len(layers)):
            assert np.abs(want[i]).max() >= 3, f"layer {i} is all but empty"
            _exact(got[i], want[i], f"n = {n}, layer {i} ({layers[i]['kind']})")
        srcs = layers[route]["layers"]
        _exact(got[route], np.concatenate([want[s] for s in srcs], axis=1), f"n = {n}, the route")
        assert np.array_equal(got[route], np.concatenate([got[s] for s in srcs], axis=1))
    det.close()


# ---- 3. the real topologies, end to end --------------------------------------------------------------------------
# name: generator, net_w, net_h, the weights' seed and gain, the frames' seed, routes in place, routes copied.  The
# seeds were chosen on the CPU: with them the reference alone meets _assert_reference_conditions.
NETS = {"yolov3": (yr.full_cfg, 64, 32, 6, 0.7, 5, (86, 98), (83, 95)),
        "yolov3-tiny": (yr.tiny_cfg, 96, 64, 1, 1.0, 101, (20,), (17,))}
N_FRAMES = 2
ZERO_THRESH, CONFIDENCE = 0.2, 0.25
# Head tensors against float64: the largest absolute error measured on the MI355X over the heads and the 2 frames
# (see the docstring of test_real_topology_heads_against_float64); the bound is 8 x that.
HEAD_MEASURED = {"yolov3": 9.240e-06, "yolov3-tiny": 8.750e-06}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The network's layers and folded parameters, the two blobs, the float64 forward pass and its decoded rows
    (at the confidence, and at a zero threshold and confidence of nothing: every row's score), computed once."""
    gen, net_w, net_h, seed, gain, frame_seed, _, _ = NETS[name]
    _, layers = dk.parse_cfg(gen(80, net_w, net_h))
    params = dk.load_weights(dk.write_weights(layers, yr.random_raw(layers, seed, gain, obj_bias=-2.0)), layers)
    frames = yr.make_frames(N_FRAMES, 640, 360, frame_seed)
    x = np.stack([yr.blob(f, net_w, net_h)[0] for f in frames])
    outs = yr.forward(layers, params, x)
    heads = [ly["index"] for ly in layers if ly["kind"] == dk.YOLO]
    houts = {i: outs[i] for i in heads}
    rows = [yr.decode(layers, houts, net_w, net_h, ZERO_THRESH, CONFIDENCE, f) for f in range(N_FRAMES)]
    scores = [yr.decode(layers, houts, net_w, net_h, 0.0, -1.0, f) for f in range(N_FRAMES)]
    for a in [x, *outs, *rows, *scores]:
        a.setflags(write=False)
    return layers, params, x, outs, heads, rows, scores


def _assert_reference_conditions(name):
    """Conditions on the float64 reference alone, met by the choice of the seed."""
    layers, params, x, outs, heads, rows, scores = _reference(name)
    classes, from_heads = set(), set()
    for f in range(N_FRAMES):
        p = scores[f][:, 8]
        assert len(p) == sum(3 * outs[i].shape[2] * outs[i].shape[3] for i in heads)
        assert np.all(np.abs(p - ZERO_THRESH) > 1e-3) and np.all(np.abs(p - CONFIDENCE) > 1e-3), \
            "a reference score within 1e-3 of a threshold"
        assert len(rows[f]) >= 10, (f, len(rows[f]))
        classes.update(rows[f][:, 7].tolist())
        from_heads.update(rows[f][:, 0].tolist())
        for r in rows[f]:  # the winning class leads the next one by more than the heads' errors can close
            t = outs[heads[int(r[0])]][f]
            cell, a = divmod(int(r[1]), 3)
            logits = t.reshape(3, 85, -1)[a, 5:, cell]
            top = np.sort(logits)[-2:]
            assert int(np.argmax(logits)) == int(r[7]) and top[1] - top[0] > 1e-3, (f, r[:2], top)
    assert len(from_heads) >= 2 and len(classes) >= 3, (from_heads, classes)
    assert all(np.isfinite(outs[i]).all() and np.abs(outs[i]).max() < 50 for i in heads)


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """One run of the network on the GPU over the reference's blobs: routes in place, every layer's output, the
    decoded rows."""
    layers, params, x, *_ = _reference(name)
    _, net_w, net_h, _, _, _, placed, copied = NETS[name]
    det = YoloDetector(layers, params, CLASSES80, net_w=net_w, net_h=net_h, max_frames=N_FRAMES,
                       zero_thresh=ZERO_THRESH)
    routes = {i: det.route_in_place(i) for i in placed + copied}
    det.forward(x)
    assert np.array_equal(det.layer_output(-1, N_FRAMES), x)
    gouts = [det.layer_output(i, N_FRAMES) for i in range(len(layers))]
    rows = det.decode(N_FRAMES, CONFIDENCE)
    n_rows = det.rows
    det.close()
    return routes, gouts, rows, n_rows


@pytest.mark.parametrize("name", list(NETS))
def test_real_topology_routes_and_every_layer(name):
    layers, params, x, outs, heads, _, _ = _reference(name)
    _assert_reference_conditions(name)
    *_, placed, copied = NETS[name]
    routes, gouts, _, n_rows = _gpu(name)
    assert routes == {**{i: True for i in placed}, **{i: False for i in copied}}
    assert sorted(routes) == [ly["index"] for ly in layers if ly["kind"] == dk.ROUTE]
    assert n_rows == sum(3 * outs[i].shape[2] * outs[i].shape[3] for i in heads)
    assert [g.shape for g in gouts] == [o.shape for o in outs]
    worst = 0.0
    for i in range(len(layers)):  # every layer on the GPU's own inputs
        worst = max(worst, _check_layer(None, layers, params, i, x, gouts, N_FRAMES))
    print(f"{name}: {len(layers)} layers, largest convolution error on the GPU's own inputs {worst:.3e}")


@pytest.mark.parametrize("name", list(NETS))
def test_real_topology_heads_against_float64(name):
    """Largest absolute error of a head tensor against the float64 forward pass, measured on the MI355X over all
    heads and the 2 frames (HEAD_MEASURED): yolov3 at 64 x 32 9.240e-06 (logits up to 5.60), yolov3-tiny at 96 x 64
    8.750e-06 (logits up to 5.31); the bounds are 8 x that, 7.392e-05 and 7.000e-05, far below the 1e-3 the
    reference's scores keep from the thresholds."""
    layers, params, x, outs, heads, _, _ = _reference(name)
    _, gouts, _, _ = _gpu(name)
    worst = max(float(np.abs(gouts[i].astype(np.float64) - outs[i]).max()) for i in heads)
    big = max(float(np.abs(outs[i]).max()) for i in heads)
    measured = HEAD_MEASURED[name]
    print(f"{name} head tensors: largest absolute error {worst:.3e} (bound {8 * measured:.3e}), "
          f"largest value {big:.2f}")
    assert 8 * measured < 1e-3
    assert worst <= 8 * measured


@pytest.mark.parametrize("name", list(NETS))
def test_real_topology_decoded_rows(name):
    _assert_reference_conditions(name)
    layers, params, x, outs, heads, rows, _ = _reference(name)
    _, net_w, net_h, *_ = NETS[name]
    _, gouts, got, _ = _gpu(name)
    for f in range(N_FRAMES):
        g, want = got[f], rows[f]
        assert g.shape == want.shape, (f, g.shape, want.shape)
        assert g[:, :2].tolist() == want[:, :2].tolist()   # the same (head, row) sequence
        assert g[:, 7].tolist() == want[:, 7].tolist()     # the same classes
        # the values: the decode's own tolerance against the restatement's decode of the GPU's head tensors ...
        mine = yr.decode(layers, {i: gouts[i] for i in heads}, net_w, net_h, ZERO_THRESH, CONFIDENCE, f)
        assert mine[:, :2].tolist() == want[:, :2].tolist() and mine[:, 7].tolist() == want[:, 7].tolist()
        err = np.abs(g[:, 2:].astype(np.float64) - mine[:, 2:])
        assert np.all(err <= 1e-6 * np.abs(mine[:, 2:]) + 1e-7), float(err.max())
        # ... and the scores within the head tensors' bound of the float64 network's: a product of two sigmoids
        # moves by at most half of what its two logits do
        assert np.all(np.abs(g[:, 8] - want[:, 8]) <= 8 * HEAD_MEASURED[name])
    print(f"{name}: {[len(r) for r in rows]} rows, classes {sorted({int(c) for r in rows for c in r[:, 7]})}")


# ---- 4. decode pins ------------------------------------------------------------------------------------------
GRID_W, GRID_H = 4, 3
HEAD_LAYERS = (1, 4, 7)


def _heads80(zero_thresh=ZERO_THRESH, max_frames=3):
    """Three heads of 80 classes over a given [n, 255, 3, 4] tensor: a 1 x 1 identity convolution (exact), then
    the tensor itself, its 2 x 2 maxima on 2 x 2 and those upsampled to 4 x 4."""
    body = [yr.conv_cfg(255, 1, 1, "linear", bn=0), yr.yolo_cfg("0,1,2", 80), "[route]\nlayers=0\n",
            "[maxpool]\nsize=2\nstride=2\n", yr.yolo_cfg("3,4,5", 80), "[route]\nlayers=3\n", "[upsample]\nstride=2\n",
            yr.yolo_cfg("1,3,5", 80)]
    _, layers = dk.parse_cfg(yr.net_cfg(255, body, GRID_W, GRID_H))
    params = [None] * len(layers)
    params[0] = (np.eye(255, dtype=np.float32).reshape(255, 255, 1, 1), np.zeros(255, np.float32))
    det = YoloDetector(layers, params, CLASSES80, net_w=GRID_W, net_h=GRID_H, max_frames=max_frames,
                       zero_thresh=zero_thresh)
    assert det.rows == 3 * (12 + 4 + 16)
    return det, layers


def _run_heads(det, layers, x):
    """Forward x; the three head tensors as the GPU holds them, checked against the restatement's pool and upsample."""
    n = len(x)
    det.forward(x)
    outs = {i: det.layer_output(i, n) for i in HEAD_LAYERS}
    pooled = yr.maxpool(x, 2)
    assert all(np.array_equal(outs[i], t) for i, t in zip(HEAD_LAYERS, (x, pooled, yr.upsample(pooled))))
    return outs


def _assert_rows(layers, outs, got, n, zero_thresh, confidence):
    """The GPU's rows of every frame against yr.decode: the same rows and classes, values within the decode's
    tolerance.  Returns the reference's rows."""
    ref = []
    for f in range(n):
        want = yr.decode(layers, outs, GRID_W, GRID_H, zero_thresh, confidence, f)
        g = got[f]
        assert g.shape == want.shape, (f, g.shape, want.shape)
        assert g[:, :2].tolist() == want[:, :2].tolist() and g[:, 7].tolist() == want[:, 7].tolist()
        err = np.abs(g[:, 2:].astype(np.float64) - want[:, 2:])
        assert np.isfinite(g).all() and np.all(err <= 1e-6 * np.abs(want[:, 2:]) + 1e-7), float(err.max())
        ref.append(want)
    return ref


def _blank(n):
    """[n, 3 anchors, 85, 3, 4]: no objectness anywhere (sigmoid(-100) is 0 in f32), every class far down."""
    t = np.full((n, 3, 85, GRID_H, GRID_W), -100.0, np.float32)
    t[:, :, :4] = 0.0
    return t


def test_decode_score_exactly_at_a_threshold():
    """sigmoid(40) is exactly 1 and sigmoid(0) exactly 0.5, in f32 as in f64: a row whose score is exactly 0.5 is
    dropped at confidence 0.5 (`best > confidence`) and at zero_thresh 0.5 (`s <= zero_thresh`), kept just below."""
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert np.float32(below) == np.float32(0.5) - np.float32(2.0 ** -25) and below < 0.5
    t = _blank(1)
    t[0, 1, 4, 2, 1] = 40.0       # anchor 1 of cell (y 2, x 1): objectness 1
    t[0, 1, 5 + 37, 2, 1] = 0.0   # class 37: 0.5
    x = t.reshape(1, 255, GRID_H, GRID_W)
    pin = [0.0, float((2 * GRID_W + 1) * 3 + 1)]
    det, layers = _heads80()
    outs = _run_heads(det, layers, x)
    # the pooled heads hold the same logits in the cell over it: one row per head, each at exactly 0.5
    at = det.decode(1, 0.5)
    assert [len(r) for r in at] == [0]
    assert len(_assert_rows(layers, outs, at, 1, ZERO_THRESH, 0.5)[0]) == 0
    kept = det.decode(1, below)
    ref = _assert_rows(layers, outs, kept, 1, ZERO_THRESH, below)[0]
    assert len(ref) == 1 + 1 + 4 and kept[0][0, :2].tolist() == pin
    assert np.all(kept[0][:, 8] == np.float32(0.5)) and np.all(kept[0][:, 6] == np.float32(1.0))
    assert np.all(kept[0][:, 7] == 37) and np.all(ref[:, 8] == 0.5)
    assert [len(r) for r in det.decode(1, 0.0)] == [6]
    det.close()
    # zero_thresh 0.5: the score is zeroed, and 0 passes no confidence >= 0
    det, layers = _heads80(zero_thresh=0.5)
    _run_heads(det, layers, x)
    for conf in (0.0, below, 0.25):
        assert [len(r) for r in det.decode(1, conf)] == [0], conf
    det.close()
    det, layers = _heads80(zero_thresh=below)
    outs = _run_heads(det, layers, x)
    for conf in (0.0, below):
        got = det.decode(1, conf)
        assert len(_assert_rows(layers, outs, got, 1, below, conf)[0]) == 6 and np.all(got[0][:, 8] == np.float32(0.5))
    assert [len(r) for r in det.decode(1, 0.5)] == [0]
    det.close()


def test_decode_ties_first_and_last_class():
    t = _blank(1)
    t[:, :, 5:] = -3.0
    cases = {  # (anchor, y, x): ({class: logit}, the winner)
        (0, 0, 0): ({17: 2.0, 42: 2.0}, 17),
        (1, 0, 2): ({0: 3.0}, 0),
        (2, 0, 0): ({79: 3.0}, 79),
        (0, 2, 2): ({0: 1.5, 79: 1.5}, 0),
        (1, 2, 0): ({c: 1.0 for c in range(80)}, 0),
        (2, 2, 2): ({78: 2.5, 79: 2.5, 3: 2.0}, 78),
        (1, 0, 0): ({79: 2.0, 5: 2.0 + 2.0 ** -12}, 5),   # the larger logit wins whatever its index
        (2, 2, 0): ({79: 2.0 + 2.0 ** -12, 5: 2.0}, 79),
    }
    for (a, y, x_), (logits, _) in cases.items():
        t[0, a, 4, y, x_] = 40.0
        for c, v in logits.items():
            t[0, a, 5 + c, y, x_] = v
    x = t.reshape(1, 255, GRID_H, GRID_W)
    det, layers = _heads80()
    outs = _run_heads(det, layers, x)
    got = det.decode(1, CONFIDENCE)
    _assert_rows(layers, outs, got, 1, ZERO_THRESH, CONFIDENCE)
    head0 = {int(r[1]): int(r[7]) for r in got[0] if r[0] == 0}
    assert head0 == {(y * GRID_W + x_) * 3 + a: win for (a, y, x_), (_, win) in cases.items()}
    assert {0, 79} <= set(got[0][got[0][:, 0] > 0][:, 7].astype(int).tolist())  # the pooled heads see both ends too
    det.close()


def test_decode_saturated_boxes():
    """tx, ty = +-100 (the sigmoid at 1 and 0), tw, th = -100 (expf may flush: the absolute tolerance covers it)
    and +80 (3.9e35 at most after the anchor: finite in f32; f32 overflows from 88.7 on, and what an infinite box
    becomes the reference does not pin)."""
    t = _blank(3)
    t[:, :, 4] = 40.0
    t[:, :, 5:] = -2.0
    t[:, :, 5 + 11] = 1.0
    rng = np.random.default_rng(80)
    for f, sizes in enumerate([(-100.0, 80.0), (-100.0,), (80.0,)]):
        t[f, :, 0:2] = rng.choice([-100.0, 100.0], (3, 2, GRID_H, GRID_W))
        t[f, :, 2:4] = rng.choice(sizes, (3, 2, GRID_H, GRID_W))
    assert np.abs(t[:, :, 2:4]).max() <= 100 and t[:, :, 2:4].max() == 80
    x = t.reshape(3, 255, GRID_H, GRID_W)
    det, layers = _heads80()
    outs = _run_heads(det, layers, x)
    got = det.decode(3, CONFIDENCE)
    ref = _assert_rows(layers, outs, got, 3, ZERO_THRESH, CONFIDENCE)
    assert [len(r) for r in ref] == [det.rows] * 3
    allrows = np.concatenate(got)
    assert allrows[:, 4:6].max() > 1e34 and allrows[:, 4:6].min() < 1e-30
    cols = np.where(allrows[:, 0] == 1, 2, 4)
    fx = allrows[:, 2] * cols  # x + sigmoid(tx): an integer at either end
    assert np.all(np.abs(fx - np.rint(fx)) < 1e-5) and {0, 4} <= set(np.rint(fx).astype(int).tolist())
    det.close()


def test_decode_every_row_then_none():
    t = _blank(3)
    t[:, :, 4] = 40.0
    rng = np.random.default_rng(96)
    t[:, :, 5:] = rng.integers(-8, 9, t[:, :, 5:].shape) / 4.0   # ties among the 80 classes included
    t[:, :, 0:4] = rng.standard_normal(t[:, :, 0:4].shape)
    x = t.reshape(3, 255, GRID_H, GRID_W)
    det, layers = _heads80()
    outs = _run_heads(det, layers, x)
    got = det.decode(3, CONFIDENCE)
    every = [[float(h), float(r)] for h, k in enumerate((12, 4, 16)) for r in range(3 * k)]
    for f in range(3):
        assert len(got[f]) == det.rows and got[f][:, :2].tolist() == every
        assert np.all(got[f][:, 8] > 0.8)
    _assert_rows(layers, outs, got, 3, ZERO_THRESH, CONFIDENCE)
    # at once a decode nothing passes: the counters were reset, no row is left over
    assert [len(r) for r in det.decode(3, 1.0)] == [0, 0, 0]
    assert [len(r) for r in det.decode(3, CONFIDENCE)] == [det.rows] * 3
    det.close()
