"""TEST ONLY: a plain float64 numpy restatement of the YOLOv3 object stage, independent of
find_motion_amd's kernels and host tail: the blob with its integer arithmetic (imutils.resize's INTER_AREA from
the oracle, cv2.resize's 8-bit INTER_LINEAR, the R/B swap and cvlib's 0.00392), the Darknet layers, the region
layer's decode, cvlib's box loop and cv2.dnn.NMSBoxes.  Also the exact convolution of small integers (int64),
the seeded miniature networks the tests run, and the one copy of the yolov3 and yolov3-tiny cfg generators, which
tools/bench_yolo.py imports.
"""
import math

import numpy as np

from find_motion_amd import darknet as dk

U = 2.0 ** -24  # f32 unit roundoff


# ---- blob ------------------------------------------------------------------------------------------------
def linear_taps(ssize: int, dsize: int):
    """cv2.resize INTER_LINEAR on 8-bit, one axis: first tap, second tap (clamped), the two short coefficients."""
    s0, s1, a0, a1 = [], [], [], []
    scale = ssize / dsize
    for d in range(dsize):
        fx = np.float32((d + 0.5) * scale - 0.5)
        sx = int(math.floor(fx))
        fx = np.float32(fx - np.float32(sx))
        if sx < 0:
            sx, fx = 0, np.float32(0)
        if sx >= ssize - 1:
            sx, fx = ssize - 1, np.float32(0)
        s0.append(sx)
        s1.append(min(sx + 1, ssize - 1))
        a0.append(int(np.rint(np.float32(np.float32(1) - fx) * np.float32(2048))))
        a1.append(int(np.rint(fx * np.float32(2048))))
    return np.array(s0), np.array(s1), np.array(a0, np.int64), np.array(a1, np.int64)


def resize_linear_u8(img: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """cv2.resize(img, (dw, dh), interpolation=INTER_LINEAR) for uint8 [H, W, C]."""
    H, W = img.shape[:2]
    if (H, W) == (dh, dw):
        return img.copy()
    x0, x1, a0, a1 = linear_taps(W, dw)
    y0, y1, b0, b1 = linear_taps(H, dh)
    S = img.astype(np.int64)
    D = S[:, x0] * a0[None, :, None] + S[:, x1] * a1[None, :, None]  # [H, dw, C]
    D0, D1 = D[y0], D[y1]
    v = (((b0[:, None, None] * (D0 >> 4)) >> 16) + ((b1[:, None, None] * (D1 >> 4)) >> 16) + 2) >> 2
    return v.astype(np.uint8)


def blob_value(v: int) -> np.float32:
    return np.float32(np.float64(v) * 0.00392)


def blob(frame: np.ndarray, net_w: int, net_h: int, roi_w: int = 300):
    """blobFromImage(imutils.resize(frame, width=roi_w), 0.00392, (net_w, net_h), (0, 0, 0), True, crop=False):
    ([3, net_h, net_w] float32 in R, G, B order, the ROI height)."""
    import oracle
    roi = oracle.resize_area_bgr(np.ascontiguousarray(frame), roi_w)
    lin = resize_linear_u8(roi, net_w, net_h)
    table = np.array([blob_value(v) for v in range(256)], np.float32)
    return table[lin[:, :, ::-1]].transpose(2, 0, 1).copy(), roi.shape[0]


# ---- layers (float64) ---------------------------------------------------------------------------------------
def conv(x, w, b, stride, pad, leaky):
    """x [n, c, h, w], w [m, c, s, s], b [m] -> (out [n, m, ho, wo], sum |w x| + |b|), both float64."""
    x, w, b = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    n, c, H, W = x.shape
    m, _, s, _ = w.shape
    ho, wo = (H + 2 * pad - s) // stride + 1, (W + 2 * pad - s) // stride + 1
    xp = np.zeros((n, c, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    cols = np.empty((n, c, s, s, ho, wo))
    for ky in range(s):
        for kx in range(s):
            cols[:, :, ky, kx] = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
    cols = cols.reshape(n, c * s * s, ho * wo)
    wm = w.reshape(m, c * s * s)
    out = np.einsum("mk,nkp->nmp", wm, cols) + b[None, :, None]
    mag = np.einsum("mk,nkp->nmp", np.abs(wm), np.abs(cols)) + np.abs(b)[None, :, None]
    if leaky:
        out = np.where(out > 0, out, 0.1 * out)
    return out.reshape(n, m, ho, wo), mag.reshape(n, m, ho, wo)


def conv_exact(x, w, b, stride, pad, leaky):
    """The convolution of integer-valued arrays in int64: (the exact result as float32 [n, m, ho, wo], the
    magnitude sums sum |w x| + |b| as int64).  With `leaky` a negative result v becomes
    np.float32(0.1) * np.float32(v): one f32 rounding, what the epilogue computes.  Refuses (AssertionError)
    values that are no integers and any magnitude sum >= 2^24: below it every partial sum of an f32 fma chain,
    in whatever order, is an integer below 2^24 and so exact, and the f32 result must equal this one bit for bit."""
    xi, wi, bi = (np.asarray(a).astype(np.int64) for a in (x, w, b))
    if not all(np.array_equal(i, np.asarray(a)) for i, a in ((xi, x), (wi, w), (bi, b))):
        raise AssertionError("conv_exact takes integer-valued arrays")
    n, c, H, W = xi.shape
    m, _, s, _ = wi.shape
    ho, wo = (H + 2 * pad - s) // stride + 1, (W + 2 * pad - s) // stride + 1
    xp = np.zeros((n, c, H + 2 * pad, W + 2 * pad), np.int64)
    xp[:, :, pad:pad + H, pad:pad + W] = xi
    cols = np.empty((c, s, s, n, ho, wo), np.int64)
    for ky in range(s):
        for kx in range(s):
            cols[:, ky, kx] = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride,
                                 kx:kx + stride * (wo - 1) + 1:stride].transpose(1, 0, 2, 3)
    cols = cols.reshape(c * s * s, n * ho * wo)
    wm = wi.reshape(m, c * s * s)
    out = wm @ cols + bi[:, None]
    mag = np.abs(wm) @ np.abs(cols) + np.abs(bi)[:, None]
    if int(mag.max()) >= 1 << 24:
        raise AssertionError(f"conv_exact: a magnitude sum of {int(mag.max())} is not below 2^24")
    f = out.astype(np.float32)
    if leaky:
        f = np.where(out < 0, np.float32(0.1) * f, f).astype(np.float32)
    shape = (m, n, ho, wo)
    return f.reshape(shape).transpose(1, 0, 2, 3).copy(), mag.reshape(shape).transpose(1, 0, 2, 3).copy()


def forward_exact(layers, params, x):
    """Every layer's output as float32 from an integer-valued x [n, c, h, w] through integer parameters, each
    one exact: the convolutions by conv_exact (which asserts its 2^24 condition), a shortcut's sum asserted
    below 2^24 as well, the other layers moving values only."""
    outs = []
    prev = np.asarray(x, np.float32)
    for ly in layers:
        if ly["kind"] == dk.CONV:
            w, b = params[ly["index"]]
            prev, _ = conv_exact(prev, w, b, ly["stride"], ly["pad"], ly["activation"] == "leaky")
        else:
            prev, _ = layer(ly, params, prev, outs)
            if ly["kind"] == dk.SHORTCUT:
                big = np.abs(outs[ly["index"] - 1].astype(np.int64)) + np.abs(outs[ly["from"]].astype(np.int64))
                if int(big.max()) >= 1 << 24:
                    raise AssertionError(f"layer {ly['index']}: a shortcut's sum is not below 2^24")
        assert prev.dtype == np.float32
        outs.append(prev)
    return outs


def layer_shapes(layers, net_w, net_h):
    """(channels, height, width) of every layer's output for a network input of net_w x net_h."""
    out = []
    for ly in layers:
        h, w = out[-1][1:] if out else (net_h, net_w)
        k = ly["kind"]
        if k == dk.CONV:
            h, w = ((v + 2 * ly["pad"] - ly["size"]) // ly["stride"] + 1 for v in (h, w))
        elif k == dk.MAXPOOL and ly["stride"] == 2:
            h, w = (h + 1) // 2, (w + 1) // 2
        elif k == dk.UPSAMPLE:
            h, w = 2 * h, 2 * w
        elif k == dk.ROUTE:
            h, w = out[ly["layers"][0]][1:]
        out.append((ly["out_c"], h, w))
    return out


def maxpool(x, stride):
    n, c, H, W = x.shape
    ho, wo = (H, W) if stride == 1 else ((H + 1) // 2, (W + 1) // 2)
    out = np.empty((n, c, ho, wo), x.dtype)
    for y in range(ho):
        for xx in range(wo):
            y0, x0 = y * stride, xx * stride
            out[:, :, y, xx] = x[:, :, y0:min(y0 + 2, H), x0:min(x0 + 2, W)].max(axis=(2, 3))
    return out


def upsample(x):
    return x.repeat(2, axis=2).repeat(2, axis=3)


def layer(ly, params, prev, outs):
    """One layer's output from its input `prev` and the earlier outputs `outs` (whatever dtype those have;
    a convolution computes in float64).  Returns (out, magnitude or None)."""
    k = ly["kind"]
    if k == dk.CONV:
        w, b = params[ly["index"]]
        return conv(prev, w, b, ly["stride"], ly["pad"], ly["activation"] == "leaky")
    if k == dk.MAXPOOL:
        return maxpool(prev, ly["stride"]), None
    if k == dk.UPSAMPLE:
        return upsample(prev), None
    if k == dk.ROUTE:
        return np.concatenate([outs[s] for s in ly["layers"]], axis=1), None
    if k == dk.SHORTCUT:
        return prev + outs[ly["from"]], None
    if k == dk.YOLO:
        return prev, None
    raise ValueError(k)


def forward(layers, params, x):
    """Every layer's output in float64 from the blob x [n, c, h, w]."""
    outs = []
    prev = x.astype(np.float64)
    for ly in layers:
        prev, _ = layer(ly, params, prev, outs)
        outs.append(prev)
    return outs


# ---- decode --------------------------------------------------------------------------------------------------
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def decode(layers, outs, net_w, net_h, zero_thresh=0.2, confidence=0.25, frame=0):
    """The region layers in yolo mode over frame `frame`: rows [head, row, bx, by, bw, bh, obj, class, p] (float64)
    in (head, y, x, anchor) order, those whose best class score exceeds the confidence."""
    rows = []
    heads = [ly for ly in layers if ly["kind"] == dk.YOLO]
    for hi, ly in enumerate(heads):
        t = np.asarray(outs[ly["index"]][frame], np.float64)
        A, nc = len(ly["mask"]), ly["classes"]
        _, R, Cc = t.shape
        t = t.reshape(A, 5 + nc, R, Cc)
        for y in range(R):
            for x in range(Cc):
                for a in range(A):
                    v = t[a, :, y, x]
                    obj = _sig(v[4])
                    p = obj * _sig(v[5:])
                    p = np.where(p <= zero_thresh, 0.0, p)
                    j = int(np.argmax(p))
                    if not p[j] > confidence:
                        continue
                    aw, ah = ly["anchors"][ly["mask"][a]]
                    rows.append([hi, (y * Cc + x) * A + a, (x + _sig(v[0])) / Cc, (y + _sig(v[1])) / R,
                                 math.exp(v[2]) * aw / net_w, math.exp(v[3]) * ah / net_h, obj, j, p[j]])
    return np.array(rows, np.float64).reshape(-1, 9)


# ---- cvlib's loop and cv2.dnn.NMSBoxes ----------------------------------------------------------------------------
def iou(a, b):
    """Intersection over union of two (x, y, w, h) rectangles in doubles."""
    iw = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
    ih = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    inter = iw * ih if iw > 0 and ih > 0 else 0.0
    ua = a[2] * a[3] + b[2] * b[3]
    if ua <= np.finfo(float).eps:
        return 1.0
    return inter / (ua - inter)


def cvlib_loop(rows, roi_w, roi_h):
    boxes, ids, confs = [], [], []
    for r in rows:
        center_x, center_y = int(r[2] * roi_w), int(r[3] * roi_h)
        w, h = int(r[4] * roi_w), int(r[5] * roi_h)
        x, y = center_x - w / 2, center_y - h / 2
        boxes.append([x, y, w, h])
        ids.append(int(r[7]))
        confs.append(float(r[8]))
    return boxes, ids, confs


def nms(boxes, scores, score_threshold, nms_threshold):
    idx = [i for i, s in enumerate(scores) if s > score_threshold]
    idx.sort(key=lambda i: scores[i], reverse=True)  # Python's sort is stable: ties stay in input order
    kept = []
    for i in idx:
        keep = True
        for j in kept:
            if iou(boxes[i], boxes[j]) > nms_threshold:
                keep = False
                break
        if keep:
            kept.append(i)
    return kept


def detect(rows, roi_w, roi_h, classes, confidence=0.25, nms_threshold=0.3):
    """cvlib.detect_common_objects' (bbox, label, conf) from decoded rows."""
    boxes, ids, confs = cvlib_loop(rows, roi_w, roi_h)
    bbox, label, conf = [], [], []
    for i in nms(boxes, confs, confidence, nms_threshold):
        x, y, w, h = boxes[i]
        bbox.append([int(x), int(y), int(x + w), int(y + h)])
        label.append(classes[ids[i]])
        conf.append(confs[i])
    return bbox, label, conf


# ---- seeded networks -------------------------------------------------------------------------------------------
def conv_cfg(filters, size=1, stride=1, act="leaky", bn=1):
    return (f"[convolutional]\n{'batch_normalize=1' if bn else ''}\nfilters={filters}\nsize={size}\nstride={stride}\n"
            f"pad=1\nactivation={act}\n")


def net_cfg(channels, body, width=64, height=64):
    return f"[net]\nwidth={width}\nheight={height}\nchannels={channels}\n\n" + "\n".join(body)


MINI_ANCHORS = "6,7, 9,12, 13,9, 16,20, 22,15, 26,28"
MINI_CLASSES = ["cat", "dog", "fox"]


def yolo_cfg(mask, classes=3):
    return (f"[yolo]\nmask = {mask}\nanchors = {MINI_ANCHORS}\nclasses={classes}\nnum=6\njitter=.3\n"
            "ignore_thresh = .7\ntruth_thresh = 1\nrandom=1\n")


def mini_cfg() -> str:
    """A two-head network with every layer kind: 17 layers, channels <= 32, 3 classes; at 64 x 64 its heads
    are 8 x 8 and 16 x 16."""
    return net_cfg(3, [
        conv_cfg(8, 3),                         # 0   64
        "[maxpool]\nsize=2\nstride=2\n",         # 1   32
        conv_cfg(16, 3, 2),                     # 2   16
        conv_cfg(16, 1),                        # 3
        conv_cfg(16, 3),                        # 4
        "[shortcut]\nfrom=-3\nactivation=linear\n",  # 5
        "[maxpool]\nsize=2\nstride=2\n",         # 6   8
        conv_cfg(32, 3),                        # 7
        "[maxpool]\nsize=2\nstride=1\n",         # 8
        conv_cfg(24, 1, 1, "linear", 0),        # 9
        yolo_cfg("3,4,5"),                      # 10
        "[route]\nlayers = -3\n",                # 11  (layer 8)
        conv_cfg(16, 1),                        # 12
        "[upsample]\nstride=2\n",                # 13  16
        "[route]\nlayers = -1, 5\n",             # 14
        conv_cfg(24, 1, 1, "linear", 0),        # 15
        yolo_cfg("0,1,2"),                      # 16
    ])


ANCHORS_TINY = "10,14, 23,27, 37,58, 81,82, 135,169, 344,319"
ANCHORS = "10,13, 16,30, 33,23, 30,61, 62,45, 59,119, 116,90, 156,198, 373,326"


def _head(mask, anchors, num, classes):
    return [conv_cfg(3 * (classes + 5), 1, 1, "linear", 0),
            f"[yolo]\nmask = {mask}\nanchors = {anchors}\nclasses={classes}\nnum={num}\njitter=.3\nignore_thresh = .7\n"
            "truth_thresh = 1\nrandom=1\n"]


def tiny_cfg(classes=80, width=416, height=416) -> str:
    """yolov3-tiny.cfg's layer list, restated: 24 layers, 13 convolutions, heads at 1/32 and 1/16."""
    pool = "[maxpool]\nsize=2\nstride=2\n"
    body = []
    for f in (16, 32, 64, 128, 256):
        body += [conv_cfg(f, 3), pool]
    body += [conv_cfg(512, 3), "[maxpool]\nsize=2\nstride=1\n", conv_cfg(1024, 3), conv_cfg(256, 1), conv_cfg(512, 3)]
    body += _head("3,4,5", ANCHORS_TINY, 6, classes)
    body += ["[route]\nlayers = -4\n", conv_cfg(128, 1), "[upsample]\nstride=2\n", "[route]\nlayers = -1, 8\n",
             conv_cfg(256, 3)]
    body += _head("0,1,2", ANCHORS_TINY, 6, classes)
    return net_cfg(3, body, width, height)


def full_cfg(classes=80, width=416, height=416) -> str:
    """yolov3.cfg's layer list, restated: Darknet-53 (52 convolutions, 23 shortcuts) and three heads at 1/32,
    1/16 and 1/8; 107 layers, 75 convolutions."""
    res = "[shortcut]\nfrom=-3\nactivation=linear\n"
    body = [conv_cfg(32, 3)]
    for f, blocks in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
        body.append(conv_cfg(f, 3, 2))
        for _ in range(blocks):
            body += [conv_cfg(f // 2, 1), conv_cfg(f, 3), res]
    for f, mask, back in ((512, "6,7,8", None), (256, "3,4,5", 61), (128, "0,1,2", 36)):
        if back is not None:
            body += ["[route]\nlayers = -4\n", conv_cfg(f, 1), "[upsample]\nstride=2\n",
                     f"[route]\nlayers = -1, {back}\n"]
        for _ in range(3):
            body += [conv_cfg(f, 1), conv_cfg(2 * f, 3)]
        body += _head(mask, ANCHORS, 9, classes)
    return net_cfg(3, body, width, height)


def random_raw(layers, seed, gain=1.0, obj_bias=-4.0):
    """Unfolded parameters for write_weights: He-scaled weights (times gain), batch-norm statistics near the
    identity; a head's convolution (the one before a [yolo]) gets its objectness biases shifted by obj_bias so
    that only some rows pass the confidence."""
    rng = np.random.default_rng(seed)
    raw = {}
    for ly in layers:
        if ly["kind"] != dk.CONV:
            continue
        n, c, s = ly["filters"], ly["in_c"], ly["size"]
        w = (rng.standard_normal((n, c, s, s)) * gain * math.sqrt(2.0 / (c * s * s))).astype(np.float32)
        if ly["batch_normalize"]:
            raw[ly["index"]] = ((rng.standard_normal(n) * 0.2).astype(np.float32),
                                (1 + 0.2 * rng.standard_normal(n)).astype(np.float32),
                                (rng.standard_normal(n) * 0.2).astype(np.float32),
                                (0.5 + rng.random(n)).astype(np.float32), w)
        else:
            b = (rng.standard_normal(n) * 0.5).astype(np.float32)
            nxt = layers[ly["index"] + 1] if ly["index"] + 1 < len(layers) else None
            if nxt is not None and nxt["kind"] == dk.YOLO:
                b[4::5 + nxt["classes"]] += np.float32(obj_bias)
            raw[ly["index"]] = (b, w)
    return raw


MINI_SEED = 62          # chosen on the CPU: with MINI_FRAMES it meets the end-to-end test's conditions
MINI_FRAMES = (3, 640, 360, 11)  # make_frames' arguments


def mini_net(seed=MINI_SEED, gain=1.0, obj_bias=-4.0):
    """(cfg text, weights bytes, layers, folded params) of the miniature network for a seed."""
    cfg = mini_cfg()
    _, layers = dk.parse_cfg(cfg)
    blob_ = dk.write_weights(layers, random_raw(layers, seed, gain, obj_bias))
    return cfg, blob_, layers, dk.load_weights(blob_, layers)


def make_frames(n, W, H, seed):
    """n BGR frames [n, H, W, 3]: coarse random blocks plus fine noise."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        coarse = rng.integers(0, 256, (-(-H // 40), -(-W // 40), 3))
        img = np.kron(coarse, np.ones((40, 40, 1), np.int64))[:H, :W]
        out[i] = np.clip(img + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
    return out


def margins_ok(rows, roi_w, roi_h, confidence=0.25, nms_threshold=0.3, eps=1e-3):
    """The end-to-end test's condition on one frame's reference rows (at a confidence lowered by eps, so that
    rows just under it are seen too): no score within eps of the confidence, no candidate pair's IoU within eps
    of the NMS threshold, no box product within eps of an integer."""
    if any(abs(r[8] - confidence) <= eps for r in rows):
        return False
    rows = [r for r in rows if r[8] > confidence]
    for r in rows:
        for v in (r[2] * roi_w, r[3] * roi_h, r[4] * roi_w, r[5] * roi_h):
            if abs(v - round(v)) <= eps:
                return False
    boxes, _, _ = cvlib_loop(rows, roi_w, roi_h)
    for i in range(len(boxes)):
        for j in range(i):
            if abs(iou(boxes[i], boxes[j]) - nms_threshold) <= eps:
                return False
    return True
