"""Darknet files -> flat arrays (the YOLOv3 object stage).

The reference tags every 15th written frame with
`cvlib.detect_common_objects(frame.resized, confidence=0.25, model='yolov3[-tiny]')`
(find_motion.py:733-741), which runs `yolov3[-tiny].cfg` + `.weights` through cv2.dnn.  cvlib keeps
those files and `yolov3_classes.txt` under ~/.cvlib/object_detection/yolo/yolov3/.  This module reads
them: `parse_cfg` the layer list, `load_weights` the convolution parameters with batch norm folded
in, `load_classes` the label names.  Pure Python + numpy; the network runs in `fm_yolo_*`.

Only what yolov3 and yolov3-tiny use is accepted; anything else raises ValueError at load.
"""
from __future__ import annotations

import struct

import numpy as np

CONV, MAXPOOL, UPSAMPLE, ROUTE, SHORTCUT, YOLO = "convolutional", "maxpool", "upsample", "route", "shortcut", "yolo"
BN_EPS = 1e-6       # the epsilon OpenCV's Darknet importer fuses batch norm with (restated, unpinned)
BLOB_SCALE = 0.00392  # cvlib's blobFromImage scale (not 1/255)

# keys of [yolo] that only matter in training (or that the region layer does not read)
_YOLO_IGNORED = {"jitter", "ignore_thresh", "truth_thresh", "random"}


def blob_table() -> np.ndarray:
    """The 256 network-input values of a u8 pixel: (float)((double)v * 0.00392)."""
    return (np.arange(256, dtype=np.float64) * BLOB_SCALE).astype(np.float32)


def _sections(text: str):
    out = []
    for ln, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith("["):
            if not line.endswith("]"):
                raise ValueError(f"line {ln}: malformed section header {raw!r}")
            out.append((line[1:-1].strip(), {}))
            continue
        if "=" not in line or not out:
            raise ValueError(f"line {ln}: expected key=value inside a section, got {raw!r}")
        k, v = line.split("=", 1)
        out[-1][1][k.strip()] = v.strip()
    return out


def _ints(v: str):
    return [int(x) for x in v.replace(" ", "").split(",") if x != ""]


def parse_cfg(text: str):
    """Darknet cfg text -> (net, layers).  `net` is the [net] section as a dict of strings; `layers`
    the ordered layer list, one dict each: `kind`, `index`, `in_c`, `out_c` and the kind's own keys
    (conv: filters size stride pad batch_normalize activation; maxpool: size stride; upsample: stride;
    route: layers (absolute); shortcut: from (absolute); yolo: mask anchors classes num).
    A section this project does not run raises ValueError naming it and its index in the file."""
    secs = _sections(text)
    if not secs or secs[0][0] not in ("net", "network"):
        raise ValueError("section 0: a cfg starts with [net]")
    net = secs[0][1]
    chans = int(net.get("channels", 3))
    layers = []
    for si, (name, kv) in enumerate(secs[1:], 1):
        i = len(layers)

        def bad(why, name=name, si=si):
            return ValueError(f"[{name}] (section {si}, layer {si - 1}): {why}")

        def geti(key, default=None, kv=kv, bad=bad):
            if key not in kv:
                if default is None:
                    raise bad(f"missing {key}")
                return default
            try:
                return int(kv[key])
            except ValueError:
                raise bad(f"{key}={kv[key]!r} is not an integer") from None

        in_c = layers[-1]["out_c"] if layers else chans
        L = {"kind": name, "index": i, "in_c": in_c}
        if name == CONV:
            if geti("groups", 1) != 1:
                raise bad("groups are not supported")
            L["filters"], L["size"], L["stride"] = geti("filters"), geti("size", 1), geti("stride", 1)
            if L["filters"] < 1:
                raise bad(f"filters={L['filters']}")
            if L["size"] not in (1, 3):
                raise bad(f"size={L['size']} (1 or 3)")
            if L["stride"] not in (1, 2):
                raise bad(f"stride={L['stride']} (1 or 2)")
            L["pad"] = L["size"] // 2 if geti("pad", 0) else geti("padding", 0)
            if not 0 <= L["pad"] <= L["size"] // 2:
                raise bad(f"padding={L['pad']}")
            L["batch_normalize"] = geti("batch_normalize", 0)
            L["activation"] = kv.get("activation", "logistic")
            if L["activation"] not in ("leaky", "linear"):
                raise bad(f"activation={L['activation']} (leaky or linear)")
            L["out_c"] = L["filters"]
        elif name == MAXPOOL:
            L["size"], L["stride"] = geti("size", 2), geti("stride", 1)
            if L["size"] != 2:
                raise bad(f"size={L['size']} (2)")
            if L["stride"] not in (1, 2):
                raise bad(f"stride={L['stride']} (1 or 2)")
            L["out_c"] = in_c
        elif name == UPSAMPLE:
            L["stride"] = geti("stride", 2)
            if L["stride"] != 2:
                raise bad(f"stride={L['stride']} (2)")
            L["out_c"] = in_c
        elif name == ROUTE:
            if "groups" in kv and geti("groups", 1) != 1:
                raise bad("groups are not supported")
            try:
                src = _ints(kv.get("layers", ""))
            except ValueError:
                raise bad(f"layers={kv.get('layers')!r}") from None
            if not 1 <= len(src) <= 2:
                raise bad(f"layers={kv.get('layers')!r} (one or two)")
            src = [s + i if s < 0 else s for s in src]
            if any(not 0 <= s < i for s in src):
                raise bad(f"layers={kv.get('layers')!r} reaches outside the layers before it")
            L["layers"] = src
            L["out_c"] = sum(layers[s]["out_c"] for s in src)
        elif name == SHORTCUT:
            f = geti("from")
            f = f + i if f < 0 else f
            if not 0 <= f < i or i == 0:
                raise bad(f"from={kv['from']} reaches outside the layers before it")
            if kv.get("activation", "linear") != "linear":
                raise bad(f"activation={kv['activation']} (linear)")
            if layers[f]["out_c"] != in_c:
                raise bad(f"adds {layers[f]['out_c']} channels to {in_c}")
            L["from"] = f
            L["out_c"] = in_c
        elif name == YOLO:
            for k in kv:
                if k not in _YOLO_IGNORED and k not in ("mask", "anchors", "classes", "num"):
                    raise bad(f"unknown key {k}")
            try:
                L["mask"] = _ints(kv["mask"])
                a = [float(x) for x in kv["anchors"].replace(" ", "").split(",")]
            except (KeyError, ValueError):
                raise bad("needs mask= and anchors= lists") from None
            L["classes"], L["num"] = geti("classes"), geti("num")
            if len(a) != 2 * L["num"]:
                raise bad(f"{len(a)} anchor values for num={L['num']}")
            if not L["mask"] or any(not 0 <= m < L["num"] for m in L["mask"]):
                raise bad(f"mask={kv['mask']} outside num={L['num']}")
            L["anchors"] = [(a[2 * k], a[2 * k + 1]) for k in range(L["num"])]
            if i == 0 or in_c != len(L["mask"]) * (L["classes"] + 5):
                raise bad(f"{in_c} input channels, len(mask) * (classes + 5) = {len(L['mask']) * (L['classes'] + 5)}")
            L["out_c"] = in_c
        else:
            raise bad("this layer kind is not supported")
        layers.append(L)
    if not layers:
        raise ValueError("a cfg without layers")
    return net, layers


def fold_bn(w, beta, gamma, mean, var):
    """Batch norm folded into the convolution in float64, rounded once to float32:
    w' = w * gamma / sqrt(var + 1e-6), b' = beta - mean * gamma / sqrt(var + 1e-6)."""
    s = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + BN_EPS)
    w2 = w.astype(np.float64) * s[:, None, None, None]
    b2 = beta.astype(np.float64) - mean.astype(np.float64) * s
    return w2.astype(np.float32), b2.astype(np.float32)


def load_weights(path, layers):
    """A Darknet .weights file (path or bytes) -> a list as long as `layers`: (w float32 [n, c, size, size],
    b float32 [n]) for each convolution, batch norm folded in, None for every other layer."""
    if isinstance(path, (bytes, bytearray, memoryview)):
        data = bytes(path)
    else:
        with open(path, "rb") as f:
            data = f.read()
    if len(data) < 16:
        raise ValueError("weights file too short for its header")
    major, minor, _rev = struct.unpack_from("<iii", data, 0)
    pos = 12 + (8 if major * 10 + minor >= 2 else 4)
    if len(data) < pos:
        raise ValueError("weights file too short for its header")

    def take(count, what):
        nonlocal pos
        end = pos + 4 * count
        if end > len(data):
            raise ValueError(f"weights file too short: {what} needs {4 * count} bytes at {pos}, {len(data) - pos} left")
        a = np.frombuffer(data, "<f4", count, pos)
        pos = end
        return a

    out = [None] * len(layers)
    for L in layers:
        if L["kind"] != CONV:
            continue
        n, c, s = L["filters"], L["in_c"], L["size"]
        what = f"layer {L['index']}"
        if L["batch_normalize"]:
            beta, gamma, mean, var = (take(n, what) for _ in range(4))
        else:
            bias = take(n, what)
        w = take(n * c * s * s, what).reshape(n, c, s, s)
        out[L["index"]] = fold_bn(w, beta, gamma, mean, var) if L["batch_normalize"] else (
            w.astype(np.float32), bias.astype(np.float32))
    if pos != len(data):
        raise ValueError(f"weights file has {len(data) - pos} bytes left over after the last layer")
    return out


def load_classes(path):
    """yolov3_classes.txt: one name per line."""
    with open(path, "r") as f:
        return [ln.strip() for ln in f.read().splitlines() if ln.strip()]


def write_weights(layers, raw, major=0, minor=2, seen=0) -> bytes:
    """The inverse of load_weights for unfolded parameters (synthetic files for tests and tools):
    `raw[i]` is (beta, gamma, mean, var, w) for a batch-normalised convolution, (bias, w) otherwise."""
    out = [struct.pack("<iii", major, minor, 0),
           struct.pack("<Q" if major * 10 + minor >= 2 else "<i", seen)]
    for L in layers:
        if L["kind"] == CONV:
            out.extend(np.ascontiguousarray(a, "<f4").tobytes() for a in raw[L["index"]])
    return b"".join(out)


# -- the host tail: cvlib's loop over the decoded rows, then cv2.dnn.NMSBoxes ----------------------

def cvlib_boxes(rows, roi_w: int, roi_h: int):
    """cvlib's loop (object_detection.py) over decoded rows [k][9] (head, row, bx, by, bw, bh, obj,
    class, p): (boxes [x, y, w, h] with float x, y and int w, h; class ids; scores)."""
    boxes, ids, scores = [], [], []
    for r in rows:
        cx, cy = int(float(r[2]) * roi_w), int(float(r[3]) * roi_h)
        w, h = int(float(r[4]) * roi_w), int(float(r[5]) * roi_h)
        boxes.append([cx - w / 2, cy - h / 2, w, h])
        ids.append(int(r[7]))
        scores.append(float(r[8]))
    return boxes, ids, scores


def _iou(a, b) -> float:
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    w, h = min(a[0] + a[2], b[0] + b[2]) - x1, min(a[1] + a[3], b[1] + b[3]) - y1
    inter = float(w) * float(h) if w > 0 and h > 0 else 0.0
    total = float(a[2]) * float(a[3]) + float(b[2]) * float(b[3])
    if total <= 2.220446049250313e-16:
        return 1.0  # two empty rectangles: jaccardDistance 0
    return inter / (total - inter)


def nms_boxes(boxes, scores, score_threshold: float, nms_threshold: float):
    """cv2.dnn.NMSBoxes on double rectangles: the candidates with score > score_threshold in a stable
    descending sort by score; one is kept when its IoU with every box kept so far is <= nms_threshold.
    Returns the kept indices in that order."""
    order = sorted((i for i in range(len(scores)) if scores[i] > score_threshold), key=lambda i: -scores[i])
    keep = []
    for i in order:
        if all(_iou(boxes[i], boxes[j]) <= nms_threshold for j in keep):
            keep.append(i)
    return keep


def detections(rows, roi_w: int, roi_h: int, classes, confidence: float = 0.25, nms: float = 0.3):
    """cvlib.detect_common_objects' return value from one frame's decoded rows: (bboxes [x1, y1, x2, y2],
    labels, confs)."""
    boxes, ids, scores = cvlib_boxes(rows, roi_w, roi_h)
    bbox, label, conf = [], [], []
    for i in nms_boxes(boxes, scores, confidence, nms):
        x, y, w, h = boxes[i]
        bbox.append([int(x), int(y), int(x + w), int(y + h)])
        label.append(str(classes[ids[i]]))
        conf.append(scores[i])
    return bbox, label, conf
