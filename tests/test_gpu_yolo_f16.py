"""The YOLOv3 stage's f16 mode (FM_YOLO_F16) on the GPU against tests/yolo_ref16.py.

1. Single convolutions of small integers, bit for bit: every f32 partial sum is exact in any order, so the f16
   kernel (k_conv16: NHWC halves, channel padding, k = (ky, kx, c), v_mfma_f32_32x32x16_f16) has one right answer.
2. The two in-place route patterns on integer networks, and routes whose channel offset is no multiple of 8 and
   are copied.
3. The layers without arithmetic and the blob, bit for bit.
4. Random values: every layer on the GPU's own input inside a derived bound.
5. Head tensors end to end inside 4 x what the restatement's own two accumulation orders differ by (a CPU
   measurement of the restatement, not of the GPU).
6. Detections of the miniature network, and the drop-in.
Weights are seeded or constructed; halves that are subnormal are zeroed in the parameters (what the matrix
instruction does with subnormal f16 inputs is not known)."""
import functools

import numpy as np
import pytest

import yolo_ref as yr
import yolo_ref16 as y16
from find_motion_amd import YoloDetector
from find_motion_amd import darknet as dk
from test_gpu_yolo import _run_vm, _write_cvlib_dir
from test_gpu_yolo_nets import CLASSES80, FULL_PATTERN, NETS, TINY_PATTERN, _sparse_int_params

pytestmark = pytest.mark.gpu


def _lin(filters, size, stride=1):
    return yr.conv_cfg(filters, size, stride, "linear", bn=0)


def _exact(got, want, what):
    """got: fm_yolo_layer_output's float32; want: the restatement's float16 (widened exactly) or float32."""
    want = np.asarray(want).astype(np.float32)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, the first at "
                           f"{tuple(int(i) for i in np.argwhere(bad)[0])}: {got[bad][0]!r}, exact {want[bad][0]!r}")


def _det(layers, params, w, h, max_frames=3, classes=(), **kw):
    return YoloDetector(layers, params, list(classes), net_w=w, net_h=h, max_frames=max_frames, precision="f16", **kw)


# ---- 1. exact convolutions -------------------------------------------------------------------------------------
def _exact_conv(cin, cout, size, stride, h, w, act, seed, head=False, frames=(1, 3)):
    body = [yr.conv_cfg(cout, size, stride, act, bn=0)]
    if head:
        body.append(yr.yolo_cfg("0,1,2", cout // 3 - 5))
    _, layers = dk.parse_cfg(yr.net_cfg(cin, body, w, h))
    rng = np.random.default_rng(seed)
    wt = rng.integers(-2, 3, (cout, cin, size, size)).astype(np.float32)
    b = rng.integers(-8, 9, cout).astype(np.float32)
    det = _det(layers, [(wt, b)] + [None] * head, w, h, classes=CLASSES80 if head else ())
    assert det.precision == "f16"
    for n in frames:
        x = rng.integers(-3, 4, (n, cin, h, w)).astype(np.float32)
        want, mag = y16.conv_exact16(x, wt, b, stride, size // 2, act == "leaky", head)
        assert int(mag.max()) <= 6 * cin * size * size + 8
        assert want.dtype == (np.float32 if head else np.float16)
        det.forward(x)
        _exact(det.layer_output(-1, n), x, "the input")
        _exact(det.layer_output(0, n), want, f"{cin}->{cout} {size}x{size} s{stride} {w}x{h} {act}, n = {n}")
    det.close()


@pytest.mark.parametrize("cout", [1, 31, 32, 33, 64, 65])
@pytest.mark.parametrize("cin", [3, 5, 8, 12, 16])
def test_conv_layer_of_integers_is_bit_exact(cin, cout):
    """Channel padding (3, 5, 12 -> 8, 8, 16), K tails (Cin = 5, 3 x 3: K = 45 of 72 padded), Cout around the 32
    and 64 of a tile, both sizes, strides and activations, odd images, 1 and 3 frames (N no multiple of a tile)."""
    for size in (1, 3):
        for stride in (1, 2):
            for h, w in ((5, 7), (13, 13)):
                for act in ("leaky", "linear"):
                    _exact_conv(cin, cout, size, stride, h, w, act, seed=cin * 4096 + cout * 2 + stride)


REAL_CONVS = [  # cin, cout, size, stride, h, w
    pytest.param(512, 1024, 3, 1, 3, 2, id="512-1024-3x3-2x3-K4608"),
    pytest.param(512, 1024, 3, 2, 5, 4, id="512-1024-3x3-s2-4x5"),
    pytest.param(1024, 512, 1, 1, 3, 5, id="1024-512-1x1-5x3"),
    pytest.param(768, 256, 1, 1, 4, 6, id="768-256-1x1-6x4"),
    pytest.param(384, 256, 3, 1, 4, 3, id="384-256-3x3-3x4-K3456"),
]


@pytest.mark.parametrize("act", ["linear", "leaky"])
@pytest.mark.parametrize("cin, cout, size, stride, h, w", REAL_CONVS)
def test_conv_at_the_real_channel_counts_is_bit_exact(cin, cout, size, stride, h, w, act):
    """Integers of up to 6 K + 8 = 27656, rounded to f16 exactly once."""
    _exact_conv(cin, cout, size, stride, h, w, act, seed=cin * 4096 + cout * 2 + stride)


def test_head_convolution_stores_f32():
    """The 1024 -> 255 convolution before a [yolo] on 13 x 13: its output is f32 and equals conv_exact itself (values
    beyond 2048, which f16 would round)."""
    _exact_conv(1024, 255, 1, 1, 13, 13, "linear", seed=1024 * 4096 + 255 * 2 + 1, head=True)
    _, layers = dk.parse_cfg(yr.net_cfg(16, [yr.conv_cfg(255, 1, 1, "linear", bn=0), yr.yolo_cfg("0,1,2", 80)], 3, 3))
    rng = np.random.default_rng(0)
    wt, b = rng.integers(-2, 3, (255, 16, 1, 1)).astype(np.float32), np.zeros(255, np.float32)
    x = rng.integers(-300, 301, (1, 16, 3, 3)).astype(np.float32)
    want, _ = yr.conv_exact(x, wt, b, 1, 0, False)
    assert np.abs(want).max() > 2048 and (want.astype(np.float16).astype(np.float32) != want).any()
    det = _det(layers, [(wt, b), None], 3, 3, classes=CLASSES80)
    det.forward(x)
    _exact(det.layer_output(0, 1), want, "layer 0")
    _exact(det.layer_output(1, 1), want, "the head's view of it")
    det.close()


@pytest.mark.parametrize("size", [1, 3])
def test_the_large_tile_variant(size):
    """Cout >= 128 and at least 512 blocks of 128 x 128 take the kernel's 2 x 2-tiles-a-wave variant: 130 channels
    (2 blocks of M, the second nearly empty) over 3 x 105 x 105 = 33075 pixels (259 blocks of N, the last partial)."""
    _exact_conv(8, 130, size, 1, 105, 105, "leaky", seed=size, frames=(3,))


def test_saturating_convolution_stores_the_largest_half():
    cin, cout, h, w = 8, 4, 5, 5
    _, layers = dk.parse_cfg(yr.net_cfg(cin, [yr.conv_cfg(cout, 3, 1, "leaky", bn=0)], w, h))
    wt = np.full((cout, cin, 3, 3), 300.0, np.float32)
    wt[1::2] = -300.0
    b = np.array([8, -8, 0, 0], np.float32)
    x = np.full((1, cin, h, w), 30.0, np.float32)
    want, mag = y16.conv_exact16(x, wt, b, 1, 1, True)
    assert np.isfinite(want.astype(np.float32)).all() and want[0, 0, 2, 2] == 65504.0 and want[0, 1, 2, 2] == -64800.0
    det = _det(layers, [(wt, b)], w, h)
    det.forward(x)
    _exact(det.layer_output(0, 1), want, "leaky")
    det.close()
    _, layers = dk.parse_cfg(yr.net_cfg(cin, [_lin(cout, 3)], w, h))
    want, _ = y16.conv_exact16(x, wt, b, 1, 1, False)
    assert want[0, 0, 2, 2] == 65504.0 and want[0, 1, 2, 2] == -65504.0 and want[0, 1, 0, 0] == -65504.0
    det = _det(layers, [(wt, b)], w, h)
    det.forward(x)
    got = det.layer_output(0, 1)
    assert np.isfinite(got).all()
    _exact(got, want, "linear")
    det.close()


# ---- 2. routes -------------------------------------------------------------------------------------------------
TINY_PLACED = [_lin(11, 3),                          # 0  writes channels 8..18 of the route's buffer
               "[maxpool]\nsize=2\nstride=2\n",       # 1  reads that view
               _lin(8, 1),                           # 2
               "[upsample]\nstride=2\n",              # 3  writes channels 0..7
               "[route]\nlayers = -1, 0\n",           # 4  in place: the offset is 8
               _lin(13, 3)]                          # 5
FULL_PLACED = [_lin(16, 3),                          # 0
               _lin(8, 1),                           # 1
               _lin(16, 3),                          # 2
               "[shortcut]\nfrom=-3\nactivation=linear\n",   # 3  writes channels 16..31 of route 10's buffer
               _lin(24, 3, 2),                       # 4  stride 2 over that view
               _lin(12, 1),                          # 5
               _lin(24, 3),                          # 6
               "[shortcut]\nfrom=-3\nactivation=linear\n",   # 7
               _lin(16, 1),                          # 8
               "[upsample]\nstride=2\n",              # 9  writes channels 0..15
               "[route]\nlayers = -1, 3\n",           # 10 in place: the offset is 16
               _lin(16, 1),                          # 11
               "[shortcut]\nfrom=3\nactivation=linear\n",    # 12 its `from` is the view
               _lin(9, 3)]                           # 13
ROUTE_NETS = [pytest.param(TINY_PLACED, 4, True, id="tiny-pattern-offset-8"),
              pytest.param(FULL_PLACED, 10, True, id="yolov3-pattern-shortcut-offset-16"),
              pytest.param(TINY_PATTERN, 4, False, id="tiny-pattern-offset-7-copied"),
              pytest.param(FULL_PATTERN, 10, False, id="yolov3-pattern-offset-12-copied")]


@pytest.mark.parametrize("body, route, placed", ROUTE_NETS)
def test_routes_in_place_and_copied_are_bit_exact(body, route, placed):
    cin, w, h = 5, 10, 6
    _, layers = dk.parse_cfg(yr.net_cfg(cin, body, w, h))
    params = _sparse_int_params(layers, seed=len(body), taps=6)
    det = _det(layers, params, w, h)
    assert det.route_in_place(route) == placed
    rng = np.random.default_rng(route)
    for n in (1, 3):
        x = rng.integers(-3, 4, (n, cin, h, w)).astype(np.float32)
        exact = yr.forward_exact(layers, params, x)  # asserts the 2^24 condition at every layer
        want = y16.forward16(layers, params, x, "exact")
        chain = y16.forward16(layers, params, x, "chain")
        det.forward(x)
        got = [det.layer_output(i, n) for i in range(len(layers))]
        halves = True  # so far every value is an integer of at most 2048, which f16 holds
        for i in range(len(layers)):
            assert np.abs(exact[i]).max() >= 3, f"layer {i} is all but empty"
            assert np.array_equal(want[i], chain[i])  # integers: the order of the sum does not matter
            halves = halves and np.abs(exact[i]).max() <= 2048
            if halves:
                assert np.array_equal(want[i].astype(np.float32), exact[i])
            _exact(got[i], want[i], f"n = {n}, layer {i} ({layers[i]['kind']})")
        srcs = layers[route]["layers"]
        assert np.array_equal(got[route], np.concatenate([got[s] for s in srcs], axis=1))
    det.close()


# ---- 3. layers without arithmetic, the blob --------------------------------------------------------------------
MOVES = ["[maxpool]\nsize=2\nstride=1\n",            # 0  7 x 9
         "[maxpool]\nsize=2\nstride=1\n",            # 1
         "[shortcut]\nfrom=0\nactivation=linear\n",  # 2  layer 1 + layer 0
         "[route]\nlayers=2\n",                      # 3  one layer: the copy kernel
         "[route]\nlayers=1,2\n",                    # 4  two layers that write: in place when C is a multiple of 8
         "[route]\nlayers=2,1\n",                    # 5  the same two, already placed: copied
         "[maxpool]\nsize=2\nstride=2\n",            # 6  4 x 5
         "[upsample]\nstride=2\n",                   # 7  8 x 10
         "[maxpool]\nsize=2\nstride=2\n",            # 8  4 x 5
         "[route]\nlayers=-1,-3\n",                  # 9  two pools
         "[route]\nlayers=0,0\n",                    # 10 one layer twice: copied
         "[maxpool]\nsize=2\nstride=2\n"]            # 11 4 x 5 from odd 7 x 9


@pytest.mark.parametrize("c, placed, placed9", [(5, False, False), (8, True, True), (12, False, True), (16, True, True)])
def test_layers_without_arithmetic_are_exact(c, placed, placed9):
    """5 and 12 channels: one channel a thread, route 4 at offset 5 or 12 copied (12: the padded width is 16), and
    route 9 of twice the channels at offset 10 copied, at offset 24 in place; 8 and 16: 16 bytes a thread, routes in
    place."""
    _, layers = dk.parse_cfg(yr.net_cfg(c, MOVES, 9, 7))
    params = [None] * len(layers)
    det = _det(layers, params, 9, 7)
    assert [det.route_in_place(i) for i in (3, 4, 5, 9, 10)] == [False, placed, False, placed9, False]
    rng = np.random.default_rng(c)
    for n in (1, 3):
        x = rng.standard_normal((n, c, 7, 9)).astype(np.float32)
        x[0, 0, 0, :4] = [70000.0, -70000.0, 65519.0, 1e-8]  # np.float16: inf, -inf, 65504, 0 -- the input is not clamped
        det.forward(x)
        with np.errstate(over="ignore"):
            x16 = x.astype(np.float16)
        got = det.layer_output(-1, n)
        assert np.array_equal(got.view(np.uint32), x16.astype(np.float32).view(np.uint32))  # np.float16(x) widened
        x16[0, 0, 0, :2] = [65504.0, -65504.0]  # (no infinities into the sums below)
        x16[0, 1] = -60000.0                    # a channel whose shortcut sum is -120000
        det.forward(x16.astype(np.float32))
        outs = [det.layer_output(i, n) for i in range(len(layers))]
        assert [o.shape[1:] for o in outs] == [(c, 7, 9)] * 4 + [(2 * c, 7, 9)] * 2 + [(2 * c, 4, 5), (2 * c, 8, 10),
                                                                                     (2 * c, 4, 5), (4 * c, 4, 5), (2 * c, 7, 9), (2 * c, 4, 5)]
        halves = []
        for i in range(len(layers)):
            want = y16.layer16(layers, params, i, halves[i - 1] if i else x16, halves)
            assert want.dtype == np.float16
            _exact(outs[i], want, f"c = {c}, n = {n}, layer {i} ({layers[i]['kind']})")
            halves.append(want)
        assert outs[2][0, 0, 0, 0] == 65504.0 and np.all(outs[2][0, 1] == -65504.0)  # the shortcut clamps
    det.close()


@pytest.mark.parametrize("W, H, net", [(640, 480, 64), (300, 200, 416), (1920, 1080, 96)])
def test_blob_is_the_f32_blob_rounded_to_f16(W, H, net):
    _, layers = dk.parse_cfg(yr.net_cfg(3, [_lin(4, 1)], net, net))
    det = _det(layers, [(np.zeros((4, 3, 1, 1), np.float32), np.zeros(4, np.float32))], net, net, max_frames=2)
    frames = yr.make_frames(2, W, H, seed=W + net)
    want = np.stack([yr.blob(f, net, net)[0] for f in frames]).astype(np.float16)
    det.forward(np.ones((2, 3, net, net), np.float32))
    rows, rh = det.candidates(frames)
    assert rh == int(H * (300 / W))
    _exact(det.layer_output(-1, 2), want, "the blob")
    table = np.array([yr.blob_value(v) for v in range(256)], np.float32).astype(np.float16)
    assert set(np.unique(want).tolist()) <= set(table.tolist())
    det.close()


# ---- 4. random values: every layer on the GPU's own input ------------------------------------------------------
def _check_layer16(layers, hp, i, x16, gouts):
    """Layer i's GPU output against exact arithmetic on the GPU's own (f16) inputs.  A convolution output y with
    magnitude sum S = sum |w x| + |b| may differ from the exact one by
        (K + 3) 2^-23 S   the f32 accumulation in any order, each add rounding to nearest or truncating (the
                          instruction's adder is not documented), with the bias add and leaky's product
      + 2^-11 |y|         half an ulp of the f16 store (not for a head's convolution, which stores f32)
      + 2^-24             the same where f16 is subnormal.
    The bound is derived, not measured.  Everything else is bit exact."""
    got = gouts[i]
    ly = layers[i]
    prev = x16 if i == 0 else gouts[i - 1]
    if ly["kind"] != dk.CONV:
        if ly["kind"] == dk.YOLO:
            want = prev
        else:
            want = y16.layer16(layers, hp, i, prev.astype(np.float16), [g.astype(np.float16) for g in gouts[:i]])
        _exact(got, want, f"layer {i} ({ly['kind']})")
        return 0.0
    want, mag = yr.layer(ly, hp, prev, gouts)  # float64 on the widened halves
    K = ly["in_c"] * ly["size"] ** 2
    head = y16.is_head_conv(layers, i)
    bound = (K + 3) * 2.0 ** -23 * mag + (0.0 if head else 2.0 ** -11 * np.abs(want)) + 2.0 ** -24
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    assert np.all(err <= bound), f"layer {i}: error up to {worst:.2f} x the bound ({int((err > bound).sum())} outputs)"
    if not head:
        assert np.array_equal(got.astype(np.float16).astype(np.float32), got), f"layer {i}: values that are no halves"
    return worst


F16_NETS = ("mini", "yolov3", "yolov3-tiny")
# The largest absolute difference of a head tensor between forward16's two accumulation orders (f64 rounded once,
# and the k-ordered f32 chain), and forward16(exact)'s distance from the float64 network on the same heads: CPU
# measurements of the restatement alone (no GPU in them), with the parameters _reference16 builds.
# (With the few subnormal halves among the weights kept instead of zeroed, the figures are 1.246e-03, 6.002e-03 and
# 2.824e-03, and 1.290e-02, 6.354e-03 and 4.193e-03: which f16 stores flip is an accident of the values.)
ORDERS_DIFFER = {"mini": 2.684e-03, "yolov3": 5.280e-03, "yolov3-tiny": 3.318e-03}
FROM_FLOAT64 = {"mini": 1.114e-02, "yolov3": 4.107e-03, "yolov3-tiny": 2.905e-03}
ZERO_THRESH, CONFIDENCE = 0.2, 0.25


@functools.lru_cache(maxsize=None)
def _reference16(name, frame_seed=None):
    """(layers, params with every weight a normal half or 0, the f32 blobs, forward16 in both orders, the float64
    network), computed once."""
    if name == "mini":
        _, _, layers, params = yr.mini_net()
        net_w = net_h = 64
        n, W, H, fs = yr.MINI_FRAMES
        frames = yr.make_frames(n, W, H, fs if frame_seed is None else frame_seed)
    else:
        gen, net_w, net_h, seed, gain, fseed, _, _ = NETS[name]
        _, layers = dk.parse_cfg(gen(80, net_w, net_h))
        params = dk.load_weights(dk.write_weights(layers, yr.random_raw(layers, seed, gain, obj_bias=-2.0)), layers)
        frames = yr.make_frames(2, 640, 360, fseed)
    hp = y16.half_params(params, flush_subnormals=True)
    blobs, rh = zip(*[yr.blob(f, net_w, net_h) for f in frames])
    x = np.stack(blobs)
    exact = y16.forward16(layers, hp, x, "exact")
    chain = y16.forward16(layers, hp, x, "chain")
    f64 = yr.forward(layers, hp, x)
    heads = [ly["index"] for ly in layers if ly["kind"] == dk.YOLO]
    for a in [x, *exact, *chain, *f64]:
        a.setflags(write=False)
    return layers, hp, frames, x, rh[0], exact, chain, f64, heads, (net_w, net_h)


@functools.lru_cache(maxsize=None)
def _gpu16(name, frame_seed=None):
    layers, hp, frames, x, rh, exact, chain, f64, heads, (net_w, net_h) = _reference16(name, frame_seed)
    n = len(x)
    det = _det(layers, hp, net_w, net_h, max_frames=n, classes=yr.MINI_CLASSES if name == "mini" else CLASSES80,
               zero_thresh=ZERO_THRESH)
    routes = {ly["index"]: det.route_in_place(ly["index"]) for ly in layers if ly["kind"] == dk.ROUTE}
    dets = det.detect_frames(frames)
    _exact(det.layer_output(-1, n), x.astype(np.float16), "the blob")
    gouts = [det.layer_output(i, n) for i in range(len(layers))]
    rows = det.decode(n, CONFIDENCE)
    det.close()
    return routes, gouts, rows, dets


@pytest.mark.parametrize("name", F16_NETS)
def test_every_layer_on_the_gpus_own_input(name):
    layers, hp, frames, x, rh, exact, chain, f64, heads, _ = _reference16(name)
    for p in hp:  # no subnormal half among the parameters
        assert p is None or not ((np.abs(p[0]) < y16.H_TINY) & (p[0] != 0)).any()
    routes, gouts, _, _ = _gpu16(name)
    placed = {"mini": {11: False, 14: True}, "yolov3": {83: False, 86: True, 95: False, 98: True},
              "yolov3-tiny": {17: False, 20: True}}[name]
    assert routes == placed
    assert [g.shape for g in gouts] == [e.shape for e in exact]
    x16 = x.astype(np.float16).astype(np.float32)
    worst = max(_check_layer16(layers, hp, i, x16, gouts) for i in range(len(layers)))
    print(f"{name}: {len(layers)} layers, the worst convolution output at {worst:.3f} of its bound")


@pytest.mark.parametrize("name", F16_NETS)
def test_head_tensors_within_four_times_the_restatements_own_spread(name):
    """The GPU differs from forward16 only by the order of its f32 accumulation, which shows as rare flips of an
    f16 store further down.  How much that moves a head is measured on the CPU between the restatement's own two
    orders (ORDERS_DIFFER: mini 2.684e-03 with logits up to 15.5, yolov3 at 64 x 32 5.280e-03 with logits up to
    5.6, yolov3-tiny at 96 x 64 3.318e-03 with logits up to 5.3; the emulation's distance from float64 on the same
    heads: 1.114e-02, 4.107e-03, 2.905e-03).  The GPU's order is a third one: its heads must lie within 4 x that of forward16(exact)."""
    layers, hp, frames, x, rh, exact, chain, f64, heads, _ = _reference16(name)
    spread = max(float(np.abs(exact[i].astype(np.float64) - chain[i]).max()) for i in heads)
    dist = max(float(np.abs(exact[i].astype(np.float64) - f64[i]).max()) for i in heads)
    print(f"{name}: the restatement's orders differ by {spread:.3e}, it lies {dist:.3e} from float64")
    assert abs(spread - ORDERS_DIFFER[name]) <= 1e-3 * ORDERS_DIFFER[name], spread  # the recorded CPU measurements
    assert abs(dist - FROM_FLOAT64[name]) <= 1e-3 * FROM_FLOAT64[name], dist
    _, gouts, _, _ = _gpu16(name)
    worst = max(float(np.abs(gouts[i].astype(np.float64) - exact[i]).max()) for i in heads)
    print(f"{name}: the GPU's heads lie {worst:.3e} from forward16(exact); the bound is {4 * ORDERS_DIFFER[name]:.3e}")
    assert worst <= 4 * ORDERS_DIFFER[name]


# ---- 6. detections ---------------------------------------------------------------------------------------------
DET_FRAME_SEED = 12          # with MINI_SEED's weights: chosen on the CPU, see _assert_detection_reference
DET_ORDERS_DIFFER = 2.430e-03  # the same CPU measurement as ORDERS_DIFFER, on these frames
DET_HEAD_BOUND = 4 * DET_ORDERS_DIFFER


def _margins(rows, roi_w, roi_h, eps):
    """yolo_ref.margins_ok's conditions on scores and IoUs: none within eps of its threshold."""
    if any(abs(r[8] - CONFIDENCE) <= eps for r in rows):
        return False
    rows = [r for r in rows if r[8] > CONFIDENCE]
    boxes, _, _ = yr.cvlib_loop(rows, roi_w, roi_h)
    return all(abs(yr.iou(boxes[i], boxes[j]) - 0.3) > eps for i in range(len(boxes)) for j in range(i))


def _assert_detection_reference():
    """Conditions on the restatement alone, met by the choice of the frames' seed: both accumulation orders give
    the same boxes and labels; their labels, rows and box counts are the float64 network's; no score and no IoU
    within DET_HEAD_BOUND / 2 of its threshold (a score, the product of two sigmoids, moves by at most half of
    what its two logits move)."""
    layers, hp, frames, x, rh, exact, chain, f64, heads, _ = _reference16("mini", DET_FRAME_SEED)
    spread = max(float(np.abs(exact[i].astype(np.float64) - chain[i]).max()) for i in heads)
    assert abs(spread - DET_ORDERS_DIFFER) <= 1e-3 * DET_ORDERS_DIFFER, spread
    out, labels = [], set()
    for f in range(len(frames)):
        res = []
        for o in (exact, chain, f64):
            rows = yr.decode(layers, o, 64, 64, ZERO_THRESH, CONFIDENCE, f)
            res.append((rows, yr.detect(rows, 300, rh, yr.MINI_CLASSES, CONFIDENCE, 0.3)))
        assert res[0][1][:2] == res[1][1][:2], f"frame {f}: the two orders disagree"
        assert res[0][1][1] == res[2][1][1] and len(res[0][1][0]) == len(res[2][1][0]), f"frame {f}: not float64's labels"
        assert res[0][0][:, :2].tolist() == res[2][0][:, :2].tolist()
        near = yr.decode(layers, exact, 64, 64, ZERO_THRESH, CONFIDENCE - DET_HEAD_BOUND / 2, f)
        assert _margins(near, 300, rh, DET_HEAD_BOUND / 2), f"frame {f}: a score or an IoU next to its threshold"
        assert len(res[0][1][0]) >= 4 and len(res[0][0]) - len(res[0][1][0]) >= 1
        labels.update(res[0][1][1])
        out.append(res[0])
    assert len(labels) >= 2
    return out


def test_detections_of_the_miniature_network():
    want = _assert_detection_reference()
    layers, hp, frames, x, rh, exact, chain, f64, heads, _ = _reference16("mini", DET_FRAME_SEED)
    _, gouts, grows, dets = _gpu16("mini", DET_FRAME_SEED)
    worst = max(float(np.abs(gouts[i].astype(np.float64) - exact[i]).max()) for i in heads)
    assert worst <= DET_HEAD_BOUND, worst
    B = DET_HEAD_BOUND
    for f in range(len(frames)):
        rows, (bbox, label, conf) = want[f]
        g = grows[f]
        assert g.shape == rows.shape and g[:, :2].tolist() == rows[:, :2].tolist() and g[:, 7].tolist() == rows[:, 7].tolist()
        assert np.all(np.abs(g[:, 8] - rows[:, 8]) <= B / 2 + 1e-6)
        gb, gl, gc = dets[f]
        assert gl == label and len(gb) == len(bbox), f   # the same labels, count and order
        # the rows NMS kept, in its order: the restatement's own NMS over its rows
        boxes, ids, confs = yr.cvlib_loop(rows, 300, rh)
        kept = yr.nms(boxes, confs, CONFIDENCE, 0.3)
        assert len(kept) == len(bbox)
        for k, i in enumerate(kept):
            r = rows[i]
            cols = exact[heads[int(r[0])]].shape[3]
            rws = exact[heads[int(r[0])]].shape[2]
            # centre: sigmoid' <= 1/4; size: exp(t + B) - exp(t) = size (e^B - 1); x = centre - w / 2
            dcx, dcy = 300 * B / (4 * cols), rh * B / (4 * rws)
            dw, dh = 300 * r[4] * np.expm1(B), rh * r[5] * np.expm1(B)
            tol = [dcx + dw / 2 + 1, dcy + dh / 2 + 1, dcx + dw / 2 + 1, dcy + dh / 2 + 1]
            for j in range(4):
                assert abs(gb[k][j] - bbox[k][j]) <= tol[j], (f, k, j, gb[k], bbox[k], tol)
            assert abs(gc[k] - conf[k]) <= B / 2 + 1e-6


# ---- 7. the drop-in --------------------------------------------------------------------------------------------
def test_video_motion_in_f16_tags_the_f32_runs_labels(tmp_path, monkeypatch):
    from find_motion_amd import motion
    monkeypatch.delenv("FM_YOLO_DIR", raising=False)
    monkeypatch.delenv("FM_YOLO_PRECISION", raising=False)
    monkeypatch.setattr(motion, "_YOLOS", {})
    frames3 = yr.make_frames(*yr.MINI_FRAMES)
    _write_cvlib_dir(tmp_path, False)
    seq = [np.roll(frames3[i % 3], 7 * i, axis=1) for i in range(33)]
    vm32, wrote32, seen32, asked32 = _run_vm(tmp_path, seq, yolo_dir=str(tmp_path))
    vm16, wrote16, seen16, asked16 = _run_vm(tmp_path, seq, yolo_dir=str(tmp_path), yolo_precision="f16")
    assert vm32.yolo is not None and vm32.yolo.precision == "f32"
    assert vm16.yolo is not None and vm16.yolo.precision == "f16" and vm16.yolo is not vm32.yolo
    assert seen32 and seen16 == seen32 and asked16 == asked32 and vm16.written_indices == vm32.written_indices
