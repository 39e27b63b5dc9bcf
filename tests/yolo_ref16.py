"""TEST ONLY: a numpy restatement of the YOLOv3 stage's f16 mode (FM_YOLO_F16), on top of
yolo_ref for everything the two modes share (the blob's integer arithmetic, the layers without arithmetic, the
decode, cvlib's loop, the seeded networks).

The mode's rules: the blob's f32 values and the folded f32 weights are each rounded once to f16 (nearest even);
biases stay f32.  A convolution accumulates the f16 x f16 products (exact in f32: 11 x 11 significant bits) in
f32, adds the bias and applies leaky in f32, clamps to +-65504 and rounds to f16 -- except a convolution that a
[yolo] head reads, which stays f32.  A shortcut is f16(float(a) + float(b)), clamped alike.  Maxpool, upsample
and route move halves.  The order of the f32 accumulation is the implementation's; `forward16` offers two:
"exact" (float64, rounded once to f32) and "chain" (an f32 chain in k = (ky, kx, c) order).
"""
import numpy as np

import yolo_ref as yr
from find_motion_amd import darknet as dk

H_MAX = np.float32(65504.0)
H_TINY = 2.0 ** -14  # the smallest normal half


def to_half(v):
    """f32 -> f16 as the mode stores it: clamped to +-65504, round to nearest even."""
    return np.clip(np.asarray(v, np.float32), -H_MAX, H_MAX).astype(np.float16)


def half_params(params, flush_subnormals=False):
    """Folded parameters with every weight rounded to f16 (kept as float32 values); biases untouched.  With
    flush_subnormals a weight whose half is subnormal becomes 0."""
    out = []
    for p in params:
        if p is None:
            out.append(None)
            continue
        w = np.asarray(p[0], np.float32).astype(np.float16).astype(np.float32)
        if flush_subnormals:
            w = np.where(np.abs(w) < H_TINY, np.float32(0), w)
        out.append((w, np.asarray(p[1], np.float32)))
    return out


def conv_exact16(x, w, b, stride, pad, leaky, head=False):
    """yolo_ref.conv_exact (integers, int64, every f32 partial sum exact in any order) and the mode's store:
    (np.float16 of the clamped f32 result -- or that f32 result for a head's convolution --, the magnitudes)."""
    f, mag = yr.conv_exact(x, w, b, stride, pad, leaky)
    return (f if head else to_half(f)), mag


def _cols(x, s, stride, pad):
    """x [n, c, h, w] float32 -> ([n, s * s * c, ho * wo] in k = (ky, kx, c) order, ho, wo)."""
    n, c, H, W = x.shape
    ho, wo = (H + 2 * pad - s) // stride + 1, (W + 2 * pad - s) // stride + 1
    xp = np.zeros((n, c, H + 2 * pad, W + 2 * pad), np.float32)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    cols = np.empty((n, s, s, c, ho, wo), np.float32)
    for ky in range(s):
        for kx in range(s):
            cols[:, ky, kx] = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
    return cols.reshape(n, s * s * c, ho * wo), ho, wo


def conv16(x, w, b, stride, pad, leaky, acc="exact", head=False):
    """x [n, c, h, w] halves, w [m, c, s, s] f32 values that are halves, b [m] f32 -> [n, m, ho, wo], float16
    (float32 for a head's convolution)."""
    x = np.asarray(x).astype(np.float32)
    w = np.asarray(w, np.float32)
    assert np.array_equal(w.astype(np.float16).astype(np.float32), w), "conv16 takes weights already rounded to f16"
    m, c, s, _ = w.shape
    cols, ho, wo = _cols(x, s, stride, pad)
    wm = w.transpose(0, 2, 3, 1).reshape(m, s * s * c)
    n = x.shape[0]
    if acc == "exact":
        a = np.einsum("mk,nkp->nmp", wm.astype(np.float64), cols.astype(np.float64)).astype(np.float32)
    elif acc == "chain":
        a = np.zeros((n, m, ho * wo), np.float32)
        for k in range(wm.shape[1]):
            a += wm[None, :, k, None] * cols[:, None, k, :]   # the product is exact, the add rounds to f32
    else:
        raise ValueError(acc)
    v = a + np.asarray(b, np.float32)[None, :, None]
    if leaky:
        v = np.where(v > 0, v, np.float32(0.1) * v).astype(np.float32)
    v = v.reshape(n, m, ho, wo)
    assert v.dtype == np.float32
    return v if head else to_half(v)


def shortcut16(a, b):
    return to_half(np.asarray(a).astype(np.float32) + np.asarray(b).astype(np.float32))


def is_head_conv(layers, i):
    return layers[i]["kind"] == dk.CONV and i + 1 < len(layers) and layers[i + 1]["kind"] == dk.YOLO


def layer16(layers, params, i, prev, outs, acc="exact"):
    """Layer i's output in the f16 mode from its input `prev` and the earlier outputs (halves; `params` already
    rounded by half_params)."""
    ly = layers[i]
    if ly["kind"] == dk.CONV:
        w, b = params[i]
        return conv16(prev, w, b, ly["stride"], ly["pad"], ly["activation"] == "leaky", acc, is_head_conv(layers, i))
    if ly["kind"] == dk.SHORTCUT:
        return shortcut16(prev, outs[ly["from"]])
    out, _ = yr.layer(ly, params, prev, outs)  # maxpool, upsample, route, yolo: values move
    return out


def forward16(layers, params, x, acc="exact", flush_subnormals=False):
    """Every layer's output in the f16 mode from the f32 blob x [n, c, h, w] and the folded f32 parameters:
    float16 arrays, float32 for a head's convolution and the head."""
    hp = half_params(params, flush_subnormals)
    outs = []
    prev = np.asarray(x, np.float32).astype(np.float16)
    for i in range(len(layers)):
        prev = layer16(layers, hp, i, prev, outs, acc)
        outs.append(prev)
    return outs
