"""Full-range content and exact ties for the object-ROI stage (fm_haar.hip), with the probes that read them out.

The Haar stage's only observable is the candidate list: one bit per window.  haar_cases' images (gray levels
30-46 with squares of 190-206) never wrap the squared-sum integral, never meet the sigma = 10 flat-window cut
exactly and never put a feature value or a stage sum on its threshold.  The images here do, and the probe
cascades are built so that the bit is the quantity under test:

  pass_all      one stump whose two leaves are 1 over a stage threshold 0: every window setWindow keeps is a
                candidate, none is rejected by stage 0 (no x-skip), so the list is the setWindow map of every scale
  node_tie      a stump on two equal, even-width rects weighing +1 and -1 with node threshold exactly 0 and leaves
                (-1, +1): a feature value of exactly 0 goes right under `<` and is accepted (stage threshold 0)
  stage_tie     two stumps with leaves (0.25, 0.5) and (0.5, 0.25) under a stage threshold of exactly 0.75: about
                half of the windows sum to exactly 0.75 and pass under `<`
  frac_weights  make_cascade(frac=True): weights uniform in +-[0.3, 3] as float32, two- and three-rect features.
                snap() then puts every node threshold on the float32 feature value the scale-0 windows of a
                period-2 image share, so all of them are node ties of the uncontracted sum; a contracted sum
                (fmaf) lands one ulp off on some nodes and takes the other leaf

Content classes (BGR, 173 x 97 unless the class needs more; image(name) builds one):

  noise         every byte uniform 0..255
  wrap          360 x 270: white with a lattice of 215 and noise in 215..255; the int64 squared sum passes 2^32.
                wrap_white / wrap_black are flat (no candidate at all), wrap_dots is white with single black
                pixels at the four corners and along the last row and column (in no norm rect) and one pixel
                further in (the last pixel of the outermost windows' norm rects)
  vtie / htie   an edge a | a + 20 (vertical for the square windows, horizontal for 14 x 28) placed so that at
                scale 0 one window per row (column) of the ystep grid has its norm rect split exactly in half:
                nf = 100 * area^2, area / sqrt(nf) = 0.1 in exact arithmetic, and the float rounding of
                1 / sqrt(nf) decides (TIE_FLAT).  Steps 19 and 21 are the neighbours on either side
  stripes2      columns alternating 100 / 140: every scale-0 window has the same content (node_tie, snap)
  checker       the 1-px checkerboard in 0 / 255: .5 ties of the resize at every scale
  gray_edges    BGR triples whose gray sum has residue 8191, 8192, 16383 or 0 modulo 16384, in 3-px blocks

General readouts are make_cascade's cascades with node thresholds calibrated on the class (calibrate(): on full-range
content thresholds around 0 send every window the same way); GENERAL holds their searched (seed, tight).

eval_windows_variant(), resize_variant(), integrals_saturating() and gray_truncating() restate oracle/haar.py with
one named mistake switched on; test_haar_content_host.py proves on the CPU that each mistake changes the
candidates of a committed case, i.e. that the GPU module (test_gpu_haar_content.py) would see it.
"""
import dataclasses
import functools

import numpy as np

import pixel_content
from find_motion_amd.cascade import Cascade
from haar_cases import make_cascade
from oracle import haar

SW, SH = 173, 97
LW, LH = 231, 131  # names ending in "@L": room for the 100 x 100 and 60 x 60 windows of the global-memory sweep
WRAP_W, WRAP_H = 360, 270
TIE_X, TIE_Y = 86, 48  # the edge column (even: x + 10, x + 12, x + 30, x + 50 for even x) and the edge row (y + 14)
GROUP_CAP = 2500       # groupRectangles' partition is quadratic: lists longer than this are compared ungrouped only

# the sigma = 10 cut at an exact tie, per window: area * (double)(float)(1 / sqrt(100 * area^2)) < 0.1
TIE_FLAT = {(20, 20): True, (24, 24): True, (14, 28): True, (100, 100): True, (60, 60): False}
# the same with 1 / sqrt(nf) kept in double: 0.09999999999999999 (not flat) or exactly 0.1 (flat)
TIE_FLAT_DOUBLE = {(20, 20): False, (24, 24): False, (14, 28): True, (100, 100): True, (60, 60): True}


# ------------------------------------------------------------------------------------------------------------
# images

def _bgr(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g, np.uint8)[..., None], 3, -1))


def tie_levels(a, step):
    """The two gray levels of an edge image: a | a + step, moved down where a + step would pass 255."""
    lo = min(a, 255 - step)
    return lo, lo + step


def _edge(a, step, axis, w, h):
    lo, hi = tie_levels(a, step)
    g = np.full((h, w), lo, np.uint8)
    if axis == 1:
        g[:, TIE_X:] = hi
    else:
        g[TIE_Y:] = hi
    return g


def _dots(w, h):
    g = np.full((h, w), 255, np.uint8)
    for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]:
        g[y, x] = 0
    g[h - 1, 7:w - 1:23] = 0
    g[5:h - 1:19, w - 1] = 0
    # the image's outermost pixels lie in no window's norm rect (it leaves a 1-px frame): these alone leave every
    # window flat.  One pixel further in they are the last pixel of the norm rect of the outermost windows
    g[1, 1] = g[h - 2, w - 2] = 0
    g[h - 2, 18:w - 2:23] = 0
    g[14:h - 2:19, w - 2] = 0
    return g


def _wrap(seed):
    rng = np.random.default_rng(seed)
    g = np.full((WRAP_H, WRAP_W), 255, np.uint8)
    g[::3, ::3] = 215
    m = rng.random(g.shape) < 0.3
    g[m] = rng.integers(215, 256, int(m.sum()), dtype=np.uint8)
    return g


@functools.lru_cache(maxsize=None)
def image(name):
    """The BGR image of a content class (read-only: shared between the tests)."""
    base, _, size = name.partition("@")
    kind, _, arg = base.partition(":")
    W, H = (LW, LH) if size == "L" else (SW, SH)
    if kind == "noise":
        img = pixel_content.noise(W, H, 1, 1, int(arg or 0))[0, 0]
    elif kind == "white":
        img = _bgr(np.full((H, W), 255))
    elif kind == "black":
        img = _bgr(np.zeros((H, W)))
    elif kind == "white300":
        img = _bgr(np.full((169, 300), 255))
    elif kind == "dots":
        img = _bgr(_dots(W, H))
    elif kind == "checker":
        img = _bgr(pixel_content.checkerboard(H, W))
    elif kind == "stripes2":
        img = _bgr(np.tile(np.array([100, 140], np.uint8), (H, W // 2 + 1))[:, :W])
    elif kind == "gray_edges":
        img = pixel_content.gray_edges(W, H, 1, 1, 11, block=3)[0, 0]
    elif kind in ("vtie", "htie"):
        a, step = (int(v) for v in arg.split(","))
        img = _bgr(_edge(a, step, 1 if kind == "vtie" else 0, W, H))
    elif kind == "wrap":
        img = _bgr(_wrap(3))
    elif kind == "wrap_white":
        img = _bgr(np.full((WRAP_H, WRAP_W), 255))
    elif kind == "wrap_black":
        img = _bgr(np.zeros((WRAP_H, WRAP_W)))
    elif kind == "wrap_dots":
        img = _bgr(_dots(WRAP_W, WRAP_H))
    else:
        raise KeyError(name)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def gray(name):
    g = haar.bgr2gray(image(name))
    g.setflags(write=False)
    return g


TIES = [f"vtie:{a},{s}" for a in (0, 100, 235) for s in (20, 19, 21)]
HTIES = [f"htie:100,{s}" for s in (20, 19, 21)]
# white beside black beside noise: the per-image integral offsets see the extremes next to each other
SMALL = ["white", "black", "noise", "dots", "checker", "stripes2", "gray_edges"] + TIES + HTIES
LARGE = [n + "@L" for n in SMALL if not n.startswith("htie")]
WRAP = ["wrap_white", "wrap_black", "wrap", "wrap_dots"]
GRAY_TWINS = ["noise", "vtie:100,20", "vtie:100,21", "vtie:235,20", "htie:100,20", "black"]  # 1-channel input


# ------------------------------------------------------------------------------------------------------------
# probe cascades

def _stumps(win, feats, stages, tilted=False):
    """feats: [(rects, weights)], stages: [(stage threshold, [(feature, node threshold, left leaf, right leaf)])].
    tilted appends an unused tilted feature: the cascade then carries the tilted integral (has_tilted)."""
    rects = np.zeros((len(feats) + int(tilted), 3, 4), np.int32)
    wts = np.zeros((len(feats) + int(tilted), 3), np.float32)
    tl = np.zeros(len(feats) + int(tilted), np.uint8)
    for i, (rs, ws) in enumerate(feats):
        rects[i, :len(rs)] = rs
        wts[i, :len(ws)] = ws
    if tilted:
        rects[-1, :2] = [[win[0] // 2, 1, 3, 3], [win[0] // 2, 2, 2, 2]]
        wts[-1, :2] = [1, -1]
        tl[-1] = 1
    trees = [t for _, st in stages for t in st]
    return Cascade(win[0], win[1], np.asarray([len(st) for _, st in stages], np.int32),
                   np.asarray([thr for thr, _ in stages], np.float32), np.ones(len(trees), np.int32),
                   np.zeros(len(trees), np.int32), -np.ones(len(trees), np.int32),
                   np.asarray([t[0] for t in trees], np.int32), np.asarray([t[1] for t in trees], np.float32),
                   np.asarray([v for t in trees for v in t[2:]], np.float32), rects, wts, tl)


def _halves(win, axis):
    """Two equal rects side by side (axis 1) or one above the other (axis 0), even in the split direction."""
    w, h = win
    if axis == 1:
        rw = 2 * ((w - 2) // 4)
        return [[1, 1, rw, h - 2], [1 + rw, 1, rw, h - 2]]
    rh = 2 * ((h - 2) // 4)
    return [[1, 1, w - 2, rh], [1, 1 + rh, w - 2, rh]]


def pass_all(win, tilted=False):
    return _stumps(win, [(_halves(win, 1), [1, -1])], [(0.0, [(0, 0.0, 1.0, 1.0)])], tilted)


def node_tie(win, tilted=False):
    return _stumps(win, [(_halves(win, 1), [1, -1])], [(0.0, [(0, 0.0, -1.0, 1.0)])], tilted)


def stage_tie(win, tilted=False):
    return _stumps(win, [(_halves(win, 1), [1, -1]), (_halves(win, 0), [1, -1])],
                   [(0.75, [(0, 0.0, 0.25, 0.5), (1, 0.0, 0.5, 0.25)])], tilted)


def frac_weights(seed, win=(20, 20), tilted=False, **kw):
    kw.setdefault("stages", 3)
    kw.setdefault("trees", 6)
    return make_cascade(seed, win=win, tilted=tilted, frac=True, **kw)


def scale0(cs, g):
    """(S, Q, T, xs, ys) of scale 0 (the image itself) on the ystep-2 grid, as detect_candidates visits it."""
    h, w = g.shape
    geo = haar.scale_geometry(w, h, cs.win_w, cs.win_h, [np.float32(1)])[0]
    S, Q, T = haar.integrals(g, cs.has_tilted)
    gy, gx = np.meshgrid(np.arange(0, geo["ylim"], 2), np.arange(0, geo["ww"], 2), indexing="ij")
    return S, Q, T, gx.ravel(), gy.ravel()


def feature_values(cs, S, Q, T, xs, ys, contracted=False, vnf_double=False, vq_signed=False):
    """(ok, values): setWindow's verdict per window and the float32 value of every feature ([n_features, n]) as
    oracle.haar.eval_windows computes them; contracted: w * s + acc rounded once (fmaf) from the second rect on."""
    area = float((cs.win_w - 2) * (cs.win_h - 2))
    nr = (1, 1, cs.win_w - 2, cs.win_h - 2)
    vs = haar._rect_sum(S, xs, ys, nr, False).astype(np.int64)
    vq = haar._rect_sum(Q, xs, ys, nr, False).astype(np.int64)
    if not vq_signed:
        vq &= 0xFFFFFFFF
    nf = area * vq.astype(np.float64) - vs.astype(np.float64) * vs.astype(np.float64)
    ok = nf > 0
    inv = np.ones(len(xs), np.float64)
    inv[ok] = 1.0 / np.sqrt(nf[ok])
    vnf = inv.astype(np.float32)
    ok &= area * (inv if vnf_double else vnf.astype(np.float64)) < 1e-1
    vals = np.zeros((len(cs.feat_tilted), len(xs)), np.float32)
    for fi in range(len(cs.feat_tilted)):
        tl = bool(cs.feat_tilted[fi])
        acc = None
        for j in range(3):
            wj = cs.feat_weights[fi, j]
            if j == 2 and wj == 0:
                continue
            sj = haar._rect_sum(T if tl else S, xs, ys, cs.feat_rects[fi, j], tl).astype(np.float32)
            if acc is None:
                acc = (np.float32(wj) * sj).astype(np.float32)
            elif contracted:
                acc = (np.float64(wj) * sj.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            else:
                acc = (acc + (np.float32(wj) * sj).astype(np.float32)).astype(np.float32)
        vals[fi] = (acc * vnf).astype(np.float32)
    return ok, vals


def eval_windows_variant(cs, S, Q, T, xs, ys, vnf_double=False, vq_signed=False, node_le=False, stage_le=False,
                         contracted=False, spy=None):
    """oracle.haar.eval_windows restated (with no switch on: the same results, which the host module asserts)
    with one mistake per switch.  spy: a dict that receives the feature values and the stage sums."""
    ok, vals = feature_values(cs, S, Q, T, xs, ys, contracted, vnf_double, vq_signed)
    n = len(xs)
    res = np.full(n, -1, np.int64)
    alive = np.nonzero(ok)[0]
    sums = []
    ti = ni = li = 0
    for si in range(cs.n_stages):
        tot = np.zeros(len(alive), np.float64)
        for _ in range(int(cs.stage_ntrees[si])):
            nn = int(cs.tree_nodes[ti])
            idx = np.zeros(len(alive), np.int64)
            cur = np.ones(len(alive), bool)
            while cur.any():
                k = np.nonzero(cur)[0]
                nd = ni + idx[k]
                v = vals[cs.node_feature[nd], alive[k]].astype(np.float64)
                t = cs.node_threshold[nd].astype(np.float64)
                idx[k] = np.where((v <= t) if node_le else (v < t), cs.node_left[nd], cs.node_right[nd])
                cur[k] = idx[k] > 0
            tot += cs.leaves[li - idx].astype(np.float64)
            ti += 1
            ni += nn
            li += nn + 1
        thr = np.float64(cs.stage_threshold[si])
        fail = (tot <= thr) if stage_le else (tot < thr)
        sums.append((alive.copy(), tot))
        res[alive[fail]] = -si
        alive = alive[~fail]
    res[alive] = 1
    if spy is not None:
        spy.update(ok=ok, vals=vals, sums=sums)
    return res


def snap(cs, name="stripes2"):  # "stripes2@L" for the windows of the global-memory sweep
    """A copy of the all-stump cascade `cs` with every node threshold on the float32 value its feature takes on
    the scale-0 windows of the period-2 image `name` (they all hold the same pixels), and every stage threshold
    just below the sum of the right leaves: under `value < threshold` on the uncontracted float32 sum every such
    window goes right at every node and passes every stage."""
    assert (cs.tree_nodes == 1).all()
    S, Q, T, xs, ys = scale0(cs, gray(name))
    ok, vals = feature_values(cs, S, Q, T, xs[:1], ys[:1])
    assert ok[0]
    nthr = vals[cs.node_feature, 0].astype(np.float32)
    sthr = np.empty(cs.n_stages, np.float32)
    t = 0
    for s in range(cs.n_stages):
        nt = int(cs.stage_ntrees[s])
        tot = 0.0
        for k in range(t, t + nt):
            tot += float(cs.leaves[2 * k + 1])  # the right leaf (node_right -1)
        v = np.float32(tot)
        sthr[s] = v if float(v) <= tot else np.nextafter(v, np.float32(-np.inf), dtype=np.float32)
        t += nt
    return dataclasses.replace(cs, node_threshold=nthr, stage_threshold=sthr)


def calibrate(cs, name):
    """A copy of `cs` with node thresholds taken from image `name` (or from a gray plane given directly): each is
    the median of its feature over the scale-0 windows that setWindow keeps.  Stage 0's stump gets the 75th
    percentile instead, so a quarter of the windows passes it.  Rect sums are not mean-free, so on full-range
    content make_cascade's thresholds around 0 send every window the same way; with these every node splits the
    windows, and the stage thresholds (make_cascade's `tight`) reject a part."""
    S, Q, T, xs, ys = scale0(cs, gray(name) if isinstance(name, str) else name)
    ok, vals = feature_values(cs, S, Q, T, xs, ys)
    nthr = np.median(vals[:, ok], axis=1).astype(np.float32)[cs.node_feature]
    nthr[0] = np.float32(np.percentile(vals[cs.node_feature[0], ok], 75))
    return dataclasses.replace(cs, node_threshold=nthr)


def resize_variant(g, dw, dh, no_round=False, no_clamp=False):
    """oracle.haar.resize_linear_exact restated; no_round drops the + 2^15 of the vertical pass, no_clamp the
    min(v, 255) behind it."""
    sh, sw = g.shape
    if (sw, sh) == (dw, dh):
        return g.copy()
    xo, xc, xlo, xhi = haar.linear_exact_tab(sw, dw)
    yo, yc, ylo, yhi = haar.linear_exact_tab(sh, dh)
    src = g.astype(np.int64)
    xs = np.arange(dw)
    x1 = np.minimum(xo + 1, sw - 1)
    hl = src[:, xo] * (256 - xc) + src[:, x1] * xc
    hl[:, xs < xlo] = src[:, :1] * 256
    if xhi < dw:
        hl[:, xs >= xhi] = src[:, xo[dw - 1]:xo[dw - 1] + 1] * 256
    out = np.empty((dh, dw), np.uint8)
    for d in range(dh):
        if d < ylo:
            out[d] = (hl[0] + 128) >> 8
        elif d >= yhi:
            out[d] = (hl[sh - 1] + 128) >> 8
        else:
            v = (hl[yo[d]] * (256 - yc[d]) + hl[yo[d] + 1] * yc[d] + (0 if no_round else 1 << 15)) >> 16
            out[d] = v if no_clamp else np.minimum(v, 255)  # uint8 assignment wraps an unclamped 256
    return out


_integrals = haar.integrals  # (the host module patches haar.integrals with the function below)


def integrals_saturating(img, tilted):
    """oracle.haar.integrals with sums that stick at the int32 limits instead of wrapping."""
    S, Q, T = _integrals(img, tilted)
    v = img.astype(np.int64)
    q = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    q[1:, 1:] = (v * v).cumsum(0).cumsum(1)
    return S, np.clip(q, -(1 << 31), (1 << 31) - 1).astype(np.int32), T


def gray_truncating(bgr):
    """oracle_np.bgr2gray without the + 8192 in front of >> 14."""
    p = bgr.astype(np.int64)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899) >> 14).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------
# the cascades and the case matrix of the GPU module

def general(name, seed, tight, **kw):
    return calibrate(make_cascade(seed, tight=tight, **kw), name)


CASCADES = {
    # the tiled sweep (k_hdetect) and the bank (k_bdetect)
    "pass20": lambda: pass_all((20, 20)),
    "pass24": lambda: pass_all((24, 24)),
    "pass14x28": lambda: pass_all((14, 28)),
    "node20": lambda: node_tie((20, 20)),
    "stage20": lambda: stage_tie((20, 20)),
    "frac20": lambda: snap(frac_weights(FRAC_SEEDS["frac20"])),
    "frac20t": lambda: snap(frac_weights(FRAC_SEEDS["frac20t"], tilted=True)),
    # general readouts (seed and tight searched on the CPU: GENERAL): depth-2 trees run run_stages and feature(),
    # stumps the record path
    "gen20": lambda: general("noise", *GENERAL["gen20"], depth=2, tilted=True),
    "gen24": lambda: general("noise", *GENERAL["gen24"], win=(24, 24), tilted=True),
    "gen20w": lambda: general("wrap", *GENERAL["gen20w"], depth=2, tilted=True),
    # the global-memory sweep (k_heval / k_heval_tail)
    "pass100": lambda: pass_all((100, 100)),
    "pass60t": lambda: pass_all((60, 60), tilted=True),
    "pass200": lambda: pass_all((200, 200)),
    "node100": lambda: node_tie((100, 100)),
    "stage60t": lambda: stage_tie((60, 60), tilted=True),
    "frac100": lambda: snap(frac_weights(FRAC_SEEDS["frac100"], win=(100, 100)), "stripes2@L"),
    "gen100": lambda: general("noise@L", *GENERAL["gen100"], win=(100, 100), stages=6),
    "gen60t": lambda: general("noise@L", *GENERAL["gen60t"], win=(60, 60), stages=6, depth=2, tilted=True),
    "gen60tw": lambda: general("wrap", *GENERAL["gen60tw"], win=(60, 60), stages=6, depth=2, tilted=True),
}
# seeds searched on the CPU (test_haar_content_host.test_frac_weights_seeds): the contracted sum turns the
# snapped cascade's scale-0 windows of stripes2 from accepted to rejected
FRAC_SEEDS = {"frac20": 0, "frac20t": 0, "frac100": 1}
# (seed, tight) of the general readouts, searched on the CPU for the rule of test_gpu_haar._check_against_live_oracle
GENERAL = {"gen20": (1, 0.38), "gen24": (1, 0.38), "gen20w": (1, 0.38), "gen100": (1, 0.38), "gen60t": (1, 0.38),
           "gen60tw": (1, 0.38)}

TILED = ["pass20", "pass24", "node20", "stage20", "frac20", "frac20t", "gen20", "gen24"]
GLOBAL = ["pass100", "pass60t", "node100", "stage60t", "frac100", "gen100", "gen60t"]
WRAP_TILED = ["pass20", "gen20w"]
WRAP_GLOBAL = ["pass100", "pass200", "gen60tw"]
BANK = ["pass20", "node20", "stage20", "frac20", "pass14x28", "gen24"]  # gen24 is the tilted member
WRAP_BANK = ["pass20", "gen20w", "pass24"]


@functools.lru_cache(maxsize=None)
def cascade(key):
    return CASCADES[key]()


@functools.lru_cache(maxsize=None)
def oracle_candidates(key, name, channels=3):
    """oracle.haar.detect_candidates of cascade `key` on image `name`, once per module run."""
    return [tuple(r) for r in haar.detect_candidates(cascade(key), image(name) if channels == 3 else gray(name), 1.1)]


@functools.lru_cache(maxsize=None)
def oracle_groups(key, name, channels=3):
    return haar.group_rectangles(oracle_candidates(key, name, channels), 3)
