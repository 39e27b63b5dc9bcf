"""The Gaussian-mixture reference: what `fgmask = cv2.createBackgroundSubtractorMOG2(...).apply(frame.blur)` puts
in place of find_diff's running average (fm.py:638-662), restated in float32 numpy from OpenCV 4.x
bgfg_gaussmix2.cpp for one channel and five mixtures, and composed with the stages oracle.oracle already restates
(resize, gray, blur, keep-mask in front; dilation and contours behind).  TEST ONLY.

Per frame: small = imutils.resize(raw, width=box); gray; blur = GaussianBlur(gray); the keep-mask writes 0;
fgmask = apply(blur) (0 background, 127 shadow, 255 foreground); thresh = 255 where fgmask == 255; dilate5 and
find_contours_ext as always.

Two statements of apply(): `apply_scalar` is the C++ loop of one pixel, line for line, on np.float32 scalars;
`Mog2Model.apply` is the same arithmetic over all pixels at once, the loops over modes unrolled and every
data-dependent step a np.where.  numpy rounds every float32 operation separately and fuses nothing, and its
float32 division is correctly rounded: the arithmetic of the spec.  tests/test_mog2_host.py holds the two
together bit for bit.

Both count events per frame (EVENTS), so that a test can assert that its content reaches a branch.
"""
import numpy as np

import oracle
from oracle import oracle as oo

F = np.float32
NM = 5
EVENTS = ("fits", "swaps", "prunes", "replacements", "var_min_clamps", "var_max_clamps", "shadows", "zero_mean_outs")

DEFAULTS = dict(history=500, var_threshold=16.0, var_threshold_gen=9.0, background_ratio=0.9, var_init=15.0,
                var_min=4.0, var_max=75.0, complexity_reduction=0.05, shadow_tau=0.5, detect_shadows=1,
                learning_rate=-1.0)


def params(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def learning_rate(prm, nframes):
    """alphaT of the frame that makes the stream's count `nframes` (>= 1): computed in double, then rounded."""
    lr = prm["learning_rate"]
    lr = float(lr) if (lr >= 0 and nframes > 1) else 1.0 / min(2 * nframes, prm["history"])
    return F(lr)


def work_shape(H, W, box):
    return oo.work_height(H, W, box), box


# ---------------------------------------------------------------------------------------------------------------
# one pixel, as the C++ reads


class PixelModel:
    """nmodes and five modes {weight, mean, var} of one pixel (entries at or above nmodes: don't care)."""

    def __init__(self):
        self.n = 0
        self.w = [F(0)] * NM
        self.m = [F(0)] * NM
        self.v = [F(0)] * NM

    def swap(self, i, j):
        for a in (self.w, self.m, self.v):
            a[i], a[j] = a[j], a[i]


def shadow_scalar(px, d, prm, ev):
    Tb, TB, tau = F(prm["var_threshold"]), F(prm["background_ratio"]), F(prm["shadow_tau"])
    t = F(0)
    for mode in range(px.n):
        num = d * px.m[mode]
        den = px.m[mode] * px.m[mode]
        if den == 0:
            ev["zero_mean_outs"] += 1
            return False
        if num <= den and num >= tau * den:
            a = num / den
            dD = a * px.m[mode] - d
            if dD * dD < Tb * px.v[mode] * a * a:
                return True
        t = t + px.w[mode]
        if t > TB:
            return False
    return False


def apply_scalar(px, d, alphaT, prm, ev):
    """One frame of one pixel; returns the mask value.  ev: a dict of EVENTS counters, added to."""
    d, alphaT = F(d), F(alphaT)
    Tb, Tg, TB = F(prm["var_threshold"]), F(prm["var_threshold_gen"]), F(prm["background_ratio"])
    vmin, vmax, CT = F(prm["var_min"]), F(prm["var_max"]), F(prm["complexity_reduction"])
    alpha1 = F(1) - alphaT
    prune = -alphaT * CT
    background = fits = False
    total = F(0)
    mode = 0
    while mode < px.n:  # nmodes may shrink inside the loop
        w = alpha1 * px.w[mode] + prune
        swaps = 0
        if not fits:
            var = px.v[mode]
            dd = px.m[mode] - d
            dist2 = dd * dd
            if total < TB and dist2 < Tb * var:
                background = True
            if dist2 < Tg * var:
                fits = True
                ev["fits"] += 1
                w = w + alphaT
                k = alphaT / w
                px.m[mode] = px.m[mode] - k * dd
                vn = var + k * (dist2 - var)
                if vn < vmin:
                    vn = vmin
                    ev["var_min_clamps"] += 1
                if vn > vmax:
                    vn = vmax
                    ev["var_max_clamps"] += 1
                px.v[mode] = vn
                i = mode
                while i > 0:
                    if w < px.w[i - 1]:
                        break
                    swaps += 1
                    px.swap(i, i - 1)
                    i -= 1
                ev["swaps"] += swaps
        if w < -prune:
            w = F(0)
            px.n -= 1
            ev["prunes"] += 1
        px.w[mode - swaps] = w
        total = total + w
        mode += 1
    with np.errstate(divide="ignore"):
        inv = F(1) / total
    for mode in range(px.n):
        px.w[mode] = px.w[mode] * inv
    if not fits and alphaT > 0:
        if px.n == NM:
            mode = NM - 1
            ev["replacements"] += 1
        else:
            mode = px.n
            px.n += 1
        if px.n == 1:
            px.w[mode] = F(1)
        else:
            px.w[mode] = alphaT
            for i in range(px.n - 1):
                px.w[i] = px.w[i] * alpha1
        px.m[mode] = d
        px.v[mode] = F(prm["var_init"])
        i = px.n - 1
        while i > 0:
            if alphaT < px.w[i - 1]:
                break
            px.swap(i, i - 1)
            i -= 1
    if background:
        return 0
    if prm["detect_shadows"] and shadow_scalar(px, d, prm, ev):
        ev["shadows"] += 1
        return 127
    return 255


def background_scalar(px, prm):
    TB = F(prm["background_ratio"])
    if px.n == 0:
        return 0
    mv = total = F(0)
    for mode in range(px.n):
        mv = mv + px.w[mode] * px.m[mode]
        total = total + px.w[mode]
        if total > TB:
            break
    return int(np.clip(np.rint(mv * (F(1) / total)), 0, 255))


def run_pixel(seq, prm=None, shadows=None):
    """apply_scalar over a sequence of values of one pixel from an empty model: (masks, events, model)."""
    prm = params() if prm is None else dict(prm)
    if shadows is not None:
        prm["detect_shadows"] = int(shadows)
    px, ev, out = PixelModel(), dict.fromkeys(EVENTS, 0), []
    for n, d in enumerate(seq, 1):
        out.append(apply_scalar(px, d, learning_rate(prm, n), prm, ev))
    return out, ev, px


# ---------------------------------------------------------------------------------------------------------------
# all pixels at once


def _swap_where(c, a, i, j):
    ai, aj = a[i].copy(), a[j].copy()
    a[i] = np.where(c, aj, ai)
    a[j] = np.where(c, ai, aj)


class Mog2Model:
    """The model of N pixels: w, m, v float32 (5, N), n int32 (N,)."""

    def __init__(self, N):
        self.N = N
        self.w = np.zeros((NM, N), F)
        self.m = np.zeros((NM, N), F)
        self.v = np.zeros((NM, N), F)
        self.n = np.zeros(N, np.int32)

    def apply(self, d, alphaT, prm, ev):
        """One frame: d float32 (N,); returns the mask values uint8 (N,).  ev: EVENTS counters, added to."""
        d, alphaT = np.asarray(d, F), F(alphaT)
        w, m, v, n = self.w, self.m, self.v, self.n
        Tb, Tg, TB = F(prm["var_threshold"]), F(prm["var_threshold_gen"]), F(prm["background_ratio"])
        vmin, vmax, CT = F(prm["var_min"]), F(prm["var_max"]), F(prm["complexity_reduction"])
        alpha1 = F(1) - alphaT
        prune = -alphaT * CT
        bgd = np.zeros(self.N, bool)
        fits = np.zeros(self.N, bool)
        total = np.zeros(self.N, F)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for M in range(NM):
                act = M < n
                wg = alpha1 * w[M] + prune
                var = v[M].copy()
                dd = m[M] - d
                dist2 = dd * dd
                look = act & ~fits
                bgd |= look & (total < TB) & (dist2 < Tb * var)
                fit = look & (dist2 < Tg * var)
                fits |= fit
                wg = np.where(fit, wg + alphaT, wg)
                k = alphaT / wg
                mn = m[M] - k * dd
                vn = var + k * (dist2 - var)
                lo = vn < vmin
                vn = np.where(lo, vmin, vn)
                hi = vn > vmax
                vn = np.where(hi, vmax, vn)
                m[M] = np.where(fit, mn, m[M])
                v[M] = np.where(fit, vn, v[M])
                ev["fits"] += int(fit.sum())
                ev["var_min_clamps"] += int((fit & lo).sum())
                ev["var_max_clamps"] += int((fit & hi).sum())
                swaps = np.zeros(self.N, np.int32)
                go = fit.copy()
                for i in range(M, 0, -1):
                    go = go & ~(wg < w[i - 1])
                    swaps += go
                    for a in (w, m, v):
                        _swap_where(go, a, i, i - 1)
                ev["swaps"] += int(swaps.sum())
                pr = act & (wg < -prune)
                wg = np.where(pr, F(0), wg)
                n -= pr
                ev["prunes"] += int(pr.sum())
                dst = M - swaps
                for j in range(M + 1):
                    w[j] = np.where(act & (dst == j), wg, w[j])
                total = np.where(act, total + wg, total)
            inv = F(1) / total
            for j in range(NM):
                w[j] = np.where(j < n, w[j] * inv, w[j])
            nw = ~fits & (alphaT > 0)
            ev["replacements"] += int((nw & (n == NM)).sum())
            slot = np.minimum(n, NM - 1)
            n2 = np.minimum(n + 1, NM)
            n[...] = np.where(nw, n2, n)
            for j in range(NM):
                at, below = nw & (j == slot), nw & (j < slot)
                w[j] = np.where(at, np.where(n2 == 1, F(1), alphaT), np.where(below, w[j] * alpha1, w[j]))
                m[j] = np.where(at, d, m[j])
                v[j] = np.where(at, F(prm["var_init"]), v[j])
            go = nw.copy()
            for i in range(NM - 1, 0, -1):
                here = i <= slot
                sw = go & here & ~(alphaT < w[i - 1])
                go = np.where(here, sw, go)
                for a in (w, m, v):
                    _swap_where(sw, a, i, i - 1)
            shadow = np.zeros(self.N, bool)
            if prm["detect_shadows"]:
                tau = F(prm["shadow_tau"])
                done = bgd.copy()
                t = np.zeros(self.N, F)
                for M in range(NM):
                    act = ~done & (M < n)
                    num = d * m[M]
                    den = m[M] * m[M]
                    z = den == 0
                    ev["zero_mean_outs"] += int((act & z).sum())
                    cand = act & ~z & (num <= den) & (num >= tau * den)
                    a = num / den
                    dD = a * m[M] - d
                    hit = cand & (dD * dD < Tb * v[M] * a * a)
                    shadow |= hit
                    done |= hit | (act & z)
                    t = t + w[M]
                    done |= act & (t > TB)
                ev["shadows"] += int(shadow.sum())
        return np.where(bgd, 0, np.where(shadow, 127, 255)).astype(np.uint8)

    def background(self, prm):
        TB = F(prm["background_ratio"])
        mv = np.zeros(self.N, F)
        total = np.zeros(self.N, F)
        done = np.zeros(self.N, bool)
        for M in range(NM):
            act = ~done & (M < self.n)
            mv = np.where(act, mv + self.w[M] * self.m[M], mv)
            total = np.where(act, total + self.w[M], total)
            done |= act & (total > TB)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.rint(mv * (F(1) / total))
        return np.where(self.n == 0, 0, np.clip(np.nan_to_num(q), 0, 255)).astype(np.uint8)

    def pixel(self, i):
        px = PixelModel()
        px.n = int(self.n[i])
        px.w, px.m, px.v = (list(a[:, i]) for a in (self.w, self.m, self.v))
        return px


class Mog2Stream:
    """One stream: the model of its h x w work pixels (row-major), nframes and the keep-mask."""

    def __init__(self, H, W, box, ksize, prm=None, keep=None):
        self.H, self.W, self.box, self.ksize = H, W, box, ksize
        self.prm = params() if prm is None else dict(prm)
        self.h, self.w = work_shape(H, W, box)
        self.model = Mog2Model(self.h * self.w)
        self.nframes = 0
        self.keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        self.events = dict.fromkeys(EVENTS, 0)  # summed over the stream's frames

    def reset(self):
        self.model = Mog2Model(self.h * self.w)
        self.nframes = 0

    def blur(self, bgr):
        assert bgr.shape == (self.H, self.W, 3) and bgr.dtype == np.uint8
        small = np.ascontiguousarray(bgr) if self.box == self.W else oo.resize_area_bgr(bgr, self.box)
        blur = oo.gauss_blur(oo.bgr2gray(small), self.ksize)
        if self.keep is not None:
            blur[self.keep == 0] = 0
        return np.ascontiguousarray(blur)

    def apply(self, blur):
        """fgmask of a blurred work image, and the frame's event counters."""
        self.nframes += 1
        ev = dict.fromkeys(EVENTS, 0)
        fg = self.model.apply(blur.reshape(-1).astype(F), learning_rate(self.prm, self.nframes), self.prm, ev)
        for k in EVENTS:
            self.events[k] += ev[k]
        return fg.reshape(self.h, self.w), ev

    def step(self, bgr, with_points=False):
        blur = self.blur(bgr)
        fg, ev = self.apply(blur)
        thresh = np.ascontiguousarray(np.where(fg == 255, 255, 0).astype(np.uint8))
        mask = oo.dilate5(thresh)
        cont = oo.find_contours_ext(mask, with_points=with_points)
        return {"blur": blur, "fgmask": fg, "thresh": thresh, "mask": mask, "count": len(cont),
                "boxes": [c["bbox"] for c in cont], "origins": [c["origin"] for c in cont], "contours": cont,
                "events": ev}

    def background_image(self):
        return self.model.background(self.prm).reshape(self.h, self.w)

    # the model in the ABI's layout: (5, h, w) float32 with zeros at mode >= nmodes, (h, w) uint8
    def arrays(self):
        live = np.arange(NM)[:, None] < self.model.n[None, :]
        out = [np.where(live, a, F(0)).reshape(NM, self.h, self.w) for a in (self.model.w, self.model.m, self.model.v)]
        return out + [self.model.n.astype(np.uint8).reshape(self.h, self.w)]

    def set_arrays(self, weight, mean, var, nmodes, nframes):
        for dst, src in ((self.model.w, weight), (self.model.m, mean), (self.model.v, var)):
            dst[...] = np.asarray(src, F).reshape(NM, -1)
        self.model.n[...] = np.asarray(nmodes).reshape(-1)
        self.nframes = int(nframes)


def threshold_bits(thresh):
    """The engine's layout of the undilated threshold plane (fm_read_threshold_bits): uint64 [ntiles][64], tile in
    raster order, word c = column c of the tile, bit r = row r."""
    h, w = thresh.shape
    ntx, nty = (w + 63) // 64, (h + 63) // 64
    p = np.zeros((nty * 64, ntx * 64), np.uint64)
    p[:h, :w] = thresh != 0
    t = p.reshape(nty, 64, ntx, 64).transpose(0, 2, 3, 1)  # [ty][tx][c][r]
    return (t << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64).reshape(nty * ntx, 64)


# ---------------------------------------------------------------------------------------------------------------
# content


def gray_frames(levels):
    """uint8 levels [...][H][W] as BGR frames [...][H][W][3] whose gray is the level ((16384 v + 8192) >> 14 = v)."""
    return np.ascontiguousarray(np.repeat(np.asarray(levels, np.uint8)[..., None], 3, axis=-1))


# the single-pixel sequences of tests/test_mog2_host.py (the last three at history = 6)
SEQ_FLICKER = [60, 140] * 20
SEQ_SHADOW = [200] * 20 + [120] * 3 + [200] * 3
SEQ_DARK = [100] * 20 + [30] * 3
SEQ_PRUNE = [100] * 3 + [200] + [100] * 30
SEQ_VARMAX = [100, 111] * 4 + [100, 118] * 4 + [100, 125] * 6
SEQ_ZERO = [0] * 5 + [50] + [0] * 3
SEQUENCES = (SEQ_FLICKER, SEQ_SHADOW, SEQ_DARK, SEQ_PRUNE, SEQ_VARMAX, SEQ_ZERO)
PALETTE = (0, 40, 90, 140, 190, 250)  # six levels, at least 40 apart: six values for five modes

FLICKER_W, FLICKER_H, FLICKER_N, FLICKER_MOVER_AT = 96, 80, 24, 12


def flicker_clip(n=FLICKER_N):
    """A 20 x 16 block that alternates 60 / 140 every frame on a level-30 ground, and from frame FLICKER_MOVER_AT a
    10 x 10 block of 220 that moves 5 px a frame along a row through the flickering block; [n][80][96][3]."""
    lv = np.full((n, FLICKER_H, FLICKER_W), 30, np.uint8)
    for t in range(n):
        lv[t, 30:46, 40:60] = 60 if t % 2 == 0 else 140
        if t >= FLICKER_MOVER_AT:
            x = 5 + 5 * (t - FLICKER_MOVER_AT)
            if x + 10 <= FLICKER_W:
                lv[t, 33:43, x:x + 10] = 220
    return gray_frames(lv)


def seq_clip(W, H, S, n, seed):
    """Stream 0: a 3 x 2 grid of cells, each playing one of SEQUENCES over and over (so each pixel of a cell's
    interior sees that sequence through the blur, and the cells' borders see mixtures of two).  The other streams:
    a grid of 11 x 10 cells, each a seeded PALETTE level per frame.  The four last columns of every stream play
    SEQUENCES as single columns.  Levels [n][S][H][W] as BGR frames [n][S][H][W][3]."""
    rng = np.random.default_rng(seed)
    lv = np.zeros((n, S, H, W), np.uint8)
    cw, ch = -(-W // 3), -(-H // 2)
    gx, gy = -(-W // 11), -(-H // 10)
    for t in range(n):
        for q, seq in enumerate(SEQUENCES):
            cy, cx = divmod(q, 3)
            lv[t, 0, cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw] = seq[t % len(seq)]
        for s in range(1, S):
            cells = rng.choice(PALETTE, size=(gy, gx)).astype(np.uint8)
            lv[t, s] = np.kron(cells, np.ones((10, 11), np.uint8))[:H, :W]
        for s in range(S):
            for q in range(min(4, W)):
                seq = SEQUENCES[(q + 2 * s) % len(SEQUENCES)]
                lv[t, s, :, W - 1 - q] = seq[t % len(seq)]
    return gray_frames(lv)


TAIL_W, TAIL_H, TAIL_SEED = 66, 70, 2025
TAIL_SIZES = [1, 7, 65] + [3] * 7  # batches of the GPU test, as many as the engine keeps in flight
TAIL_HISTORY = 6
# (name, ksize, parameter overrides) of the GPU test's runs over tail_clip()
TAIL_CONFIGS = (("k1", 1, {}), ("k5", 5, {}), ("k21", 21, {}), ("k5_noshadow", 5, {"detect_shadows": 0}),
                ("k5_lr", 5, {"learning_rate": 0.05}))
TAIL_KEEP_POLY = [[(8, 6), (50, 12), (40, 60), (12, 44)]]


def tail_clip():
    """The GPU test's content at 66 x 70, two streams, frames [94][2][70][66][3]."""
    return seq_clip(TAIL_W, TAIL_H, 2, sum(TAIL_SIZES), TAIL_SEED)


def noise_clip(W, H, S, n, seed):
    """Seeded PALETTE cells of about a sixth of the image each per frame, with per-pixel noise of +-2 and one
    moving bright block per stream; [n][S][H][W][3]."""
    rng = np.random.default_rng(seed)
    ch, cw = max(1, -(-H // 3)), max(1, -(-W // 2))
    fr = np.empty((n, S, H, W), np.int64)
    for t in range(n):
        for s in range(S):
            cells = rng.choice(PALETTE, size=(-(-H // ch), -(-W // cw)))
            f = np.kron(cells, np.ones((ch, cw), np.int64))[:H, :W] + rng.integers(-2, 3, size=(H, W))
            bw, bh = max(1, W // 5), max(1, H // 4)
            x, y = (7 * t + 23 * s) % max(1, W - bw + 1), (5 * t + 11 * s) % max(1, H - bh + 1)
            f[y:y + bh, x:x + bw] = 255 - 20 * (t % 3)
            fr[t, s] = f
    return gray_frames(np.clip(fr, 0, 255))


def gray_counts(frames, box, ksize, thresh=12, alpha=0.1):
    """The average chain's contour count of each frame of one stream [n][H][W][3] (the oracle)."""
    cfg = oracle.OracleConfig(H=frames.shape[1], W=frames.shape[2], box=box, ksize=ksize, thresh=thresh, alpha=alpha)
    st = oracle.OracleStream(cfg)
    return [st.step(f)["count"] for f in frames]


# One pixel that plays SEQ_ALL from an empty model at history = 3 reaches every event counter (asserted in
# tests/test_mog2_host.py): zeros, a var_max ramp, a shadow, six palette levels in a row, then a long rest.
SEQ_ALL = [0, 0, 50, 100, 100, 111, 100, 118, 100, 125, 100, 125, 100, 125, 200, 200, 200, 200, 120,
           0, 40, 90, 140, 190, 250, 40, 100, 100, 100, 100, 100, 100]
ALL_HISTORY = 3


def band_clip(W, H, S, n=len(SEQ_ALL), bands=8):
    """`bands` vertical bands, band b of stream s playing SEQ_ALL from position b + 3 s on: the interior of a band
    sees the sequence itself through the resize and the blur, the borders see blends of two phases; and band 0
    starts the sequence at its beginning.  [n][S][H][W][3]."""
    lv = np.zeros((n, S, H, W), np.uint8)
    band = (np.arange(W) * bands) // W
    for t in range(n):
        for s in range(S):
            lv[t, s] = np.asarray(SEQ_ALL, np.uint8)[(t + band + 3 * s) % len(SEQ_ALL)][None, :]
    return gray_frames(lv)


# The clips of tests/test_gpu_mog2.py by name: (source W, H, box, ksize, streams, bands, parameter overrides).
# tests/test_mog2_host.py asserts from the restatement alone that each reaches every event counter.
BAND_CASES = {
    "1x1": (4, 4, 1, 5, 1, 1, {}),
    "2x2": (4, 4, 2, 5, 1, 1, {}),
    "3x2": (6, 4, 3, 5, 1, 1, {}),
    "100x56": (1920, 1080, 100, 5, 1, 8, {}),
    "64x129": (64, 129, 64, 5, 1, 8, {}),
    "200x130": (200, 130, 200, 5, 1, 8, {}),
    "reset": (66, 70, 66, 3, 2, 8, {}),
    "written": (66, 70, 66, 5, 1, 8, {"history": 12}),  # a rate of 1 / 12: written weights next to TB stay below 1
}


def band_case(name):
    """(frames [n][S][H][W][3], Mog2Stream arguments (H, W, box, ksize, prm), S) of a BAND_CASES entry."""
    W, H, box, k, S, bands, ov = BAND_CASES[name]
    return band_clip(W, H, S, bands=bands), (H, W, box, k, params(**{"history": ALL_HISTORY, **ov})), S
