"""Extreme pixel content for the per-pixel chain and the INTER_AREA resize, with the conditions that prove it.

The seeded streams of find_motion_amd.synthetic are one kind of picture: a smooth gradient, +-3 noise and four
flat rectangles.  The generators here return [T][S][H][W][3] uint8 frames of the kinds that picture never
shows, and each has a check that reads, from the CPU oracle's planes alone, that the content reaches the edge
it is for.  test_pixel_content_host.py asserts every check at every shape and parameter set that
test_gpu_pixel_content.py runs, so the GPU module's inputs are proven without a GPU.

  noise        every byte uniform over 0..255 (independent channels into BGR->gray; blur sums of full-range
               terms).  Later frames redraw one window only, so that a mask is neither full nor empty.
  cells        random 0 / 255 cells of 16 px with a solid white and a solid black square at least ksize wide
               (a horizontal blur sum of 255 * 256 = 65,280, a vertical accumulator of 255 * 65,536; blur 0),
               mixed with a 1-px checkerboard frame and 2-px stripe frames in both directions
  white        all white, all black, white with single black pixels and black with single white ones at the
               corners, on every image edge and on both sides of each 64-px tile seam
  gray_edges   BGR triples whose 1868 B + 9617 G + 4899 R is 8191, 8192, 16383 or 0 modulo 16384 (the rounding
               edge of `+ 8192 >> 14` and the carry into the next gray level), interleaved with random triples
  delta_sweep  a frame black in one half and white in the other over a written background whose values run
               0..255 (with crafted_plane's fractional parts on a band of rows): every delta 0..255 occurs,
               so a threshold t in [0, 254] has pixels at t (not set) and at t + 1 (set)

pixel_cases() lists the matrix (path x content / threshold / alpha), build_case() makes a case's frames and
settings, and run_case() drives it: on the oracle alone, asserting the conditions, or beside an engine, comparing
every batch bit for bit as well.  run_frames() is run_case() on a geometry and frames given directly
(ksize_sweep.py's cases, which are not registered in CASES).
"""
import functools

import numpy as np

import oracle
from test_gpu_engine_state import PATHS as STATE_PATHS, crafted_plane

# name -> (W, H, box, k, keep_planes, the steady launch fm_kernel_times shows, the first-frame launch)
CASES = dict(STATE_PATHS)
CASES.update({
    "wide51":       (328, 136, 328, 51, False, "wide_scan", "wide_scan_init"),  # fm_wide.hip, its smallest shape
    "pix3":         (200, 136, 200, 3, False, "pix", "pix_init"),               # k_pix<3> without planes
    "pix7":         (200, 136, 200, 7, False, "pix", "pix_init"),               # k_pix<7> without planes
    # k_pix5's tile layouts (test_gpu_pix5_loop.LAYOUTS), each at its smallest shape past the small-image path
    # (200 x 136 is "pix5" above)
    "pix5_8":       (8, 2056, 8, 5, False, "pix", "pix_init"),
    "pix5_64":      (64, 264, 64, 5, False, "pix", "pix_init"),
    "pix5_68":      (68, 248, 68, 5, False, "pix", "pix_init"),
    "pix5_196":     (196, 135, 196, 5, False, "pix", "pix_init"),
})
PIXEL_PATH = {"small_scan": "small", "pix": "pix", "fused": "fused", "pixel": "pixel", "wide_scan": "wide"}
STEADY_LAUNCHES = set(PIXEL_PATH)

S, T, NB = 2, 3, 2          # streams, frames per batch, batches of every pixel case
THRESH, ALPHA = 12, 0.1     # the content axis
THRESHOLDS = (-5, -1, 0, 1, 127, 254, 255, 300)
ALPHAS = (0.0, 0.02, 0.5, 1.0, 1.5)
FULL, EMPTY = (-5, -1), (255, 300)  # thresholds whose mask is full / empty whatever the frame shows

# Blurred noise is nearly flat: the standard deviation of a full-range gray pixel is ~49, of its blur
# 49 / (2 sqrt(pi) sigma) per axis pair, i.e. ~13 (k 5), ~7 (k 11), ~4 (k 21) and ~1.7 (k 51); behind the 6.4 x
# INTER_AREA of "small_d" it is ~2.  A difference of two such blurs seldom (k 21: 1 to 4 % of the mask at 12) or
# never passes 12, so `noise` and `gray_edges` run there at the threshold below, chosen from the oracle's masks:
# at it the steady frames' masks cover 4 to 42 % (k 21), 8 to 32 % (k 51) and 13 to 38 % (small_d) of the image,
# and nothing at 6 (k 51) or 12 (small_d).  The host module asserts the mask condition at these values.
NOISE_THRESH = {"pix21": 4, "pixel51": 2, "wide51": 2, "small_d": 4}


def noise_thresh(name):
    return NOISE_THRESH.get(name, THRESH)


def geometry(name):
    W, H, box, k = CASES[name][:4]
    return W, H, box, k, oracle.work_height(H, W, box)


# ------------------------------------------------------------------------------------------------------------
# generators

def _window(rng, H, W, unit=1):
    """A random window of about a third of the width and half the height, aligned to `unit`."""
    ww = min(W, max(unit, W // 3 // unit * unit))
    wh = min(H, max(unit, H // 2 // unit * unit))
    x = int(rng.integers(0, max(1, (W - ww) // unit + 1))) * unit
    y = int(rng.integers(0, max(1, (H - wh) // unit + 1))) * unit
    return y, x, wh, ww


def noise(W, H, S, n, seed):
    """Every byte of every frame uniform over 0..255.  A stream's frame i > 0 is its frame i - 1 with one window
    redrawn: outside it (and the blur's reach) the delta is that of an unchanged scene."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, S, H, W, 3), np.uint8)
    for s in range(S):
        out[0, s] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for i in range(1, n):
            out[i, s] = out[i - 1, s]
            y, x, wh, ww = _window(rng, H, W)
            out[i, s, y:y + wh, x:x + ww] = rng.integers(0, 256, (wh, ww, 3), dtype=np.uint8)
    return out


CELL = 16


def _cell_plane(rng, H, W):
    ny, nx = -(-H // CELL), -(-W // CELL)
    c = rng.integers(0, 2, (ny, nx), dtype=np.uint8) * 255
    return np.repeat(np.repeat(c, CELL, 0), CELL, 1)[:H, :W]


def checkerboard(H, W):
    yy, xx = np.mgrid[:H, :W]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def stripes(H, W, axis):
    """2-px stripes: rows (axis 0) or columns (axis 1) 0, 1 white, 2, 3 black, ..."""
    yy, xx = np.mgrid[:H, :W]
    return ((((yy if axis == 0 else xx) >> 1) & 1) * 255).astype(np.uint8) ^ 255


def cells(W, H, S, n, seed, block):
    """Frames 0 and 1 of a stream are random 0 / 255 cells (frame 1 redraws one window of frame 0's cells), then
    the checkerboard, cells, row stripes and column stripes follow, in an order rotated by the stream.  Every
    cells frame carries the stream's solid white square and solid black square of `block` px (clipped to the
    frame), which do not move."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, S, H, W, 3), np.uint8)
    rest = ["checker", "cells", "rows", "cols"]
    for s in range(S):
        by, bx = max(1, H // block), max(1, W // block)  # whole squares (clipped only where the frame is narrower)
        assert by * bx >= 2, "no room for two squares"
        a, b = rng.choice(by * bx, 2, replace=False)
        sq = [(int(v) // bx * block, int(v) % bx * block) for v in (a, b)]
        plane = None
        for i in range(n):
            kind = "cells" if i < 2 else rest[(i - 2 + s) % 4]
            if kind == "cells":
                if plane is None:
                    plane = _cell_plane(rng, H, W)
                else:
                    y, x, wh, ww = _window(rng, H, W, CELL)
                    plane = plane.copy()
                    plane[y:y + wh, x:x + ww] = _cell_plane(rng, wh, ww)
                img = plane.copy()
                for (y, x), v in zip(sq, (255, 0)):
                    img[y:y + block, x:x + block] = v
            elif kind == "checker":
                img = checkerboard(H, W)
            else:
                img = stripes(H, W, 0 if kind == "rows" else 1)
            out[i, s] = img[..., None]
    return out


def cells_block(k, scale):
    """Side of `cells`' solid squares in source px, in whole cells: at least k + 9 work pixels, so that (behind a
    resize, whose squares do not start on a work pixel) k + 8 whole ones are solid and the blur is 0 / 255 on at
    least 8 x 8 of them."""
    return int(-(-((k + 9) * scale) // CELL)) * CELL


def dot_positions(H, W):
    """The four corners, a pixel on every image edge, and both sides of each 64-px tile seam (columns and rows
    63 | 64, 127 | 128, ...) on the edges and where seams cross."""
    xs = sorted({0, W - 1, W // 2} | {x for m in range(64, W, 64) for x in (m - 1, m)})
    ys = sorted({0, H - 1, H // 2} | {y for m in range(64, H, 64) for y in (m - 1, m)})
    seam_x = [x for x in xs if x not in (0, W - 1, W // 2)]
    seam_y = [y for y in ys if y not in (0, H - 1, H // 2)]
    pts = {(y, x) for y in (0, H - 1) for x in xs} | {(y, x) for y in ys for x in (0, W - 1)}
    pts |= {(y, x) for y in seam_y for x in seam_x}                       # seam crossings
    pts |= {(H // 2, x) for x in seam_x} | {(y, W // 2) for y in seam_y}  # a seam away from the other axis' seams
    return sorted(pts)


def white(W, H, S, n):
    """Stream 0: black, white (delta 255 everywhere), white with black dots, black, black with white dots, white;
    stream s starts s kinds later in the same cycle (the others' first frame is not black)."""
    kinds = [(0, False), (255, False), (255, True), (0, False), (0, True), (255, False)]
    pts = dot_positions(H, W)
    out = np.empty((n, S, H, W, 3), np.uint8)
    for s in range(S):
        for i in range(n):
            v, dots = kinds[(i + s) % len(kinds)]
            out[i, s] = v
            if dots:
                for y, x in pts:
                    out[i, s, y, x] = 255 - v
    return out


GRAY_RESIDUES = (8191, 8192, 16383, 0)


@functools.lru_cache(None)
def gray_edge_triples():
    """For each residue of GRAY_RESIDUES, the (B, G, R) triples whose 1868 B + 9617 G + 4899 R has it modulo
    16384: R = (residue - 1868 B - 9617 G) / 4899 in Z / 16384 (4899 is odd), kept where it is a byte."""
    inv = pow(4899, -1, 16384)
    b, g = np.mgrid[:256, :256]
    out = []
    for res in GRAY_RESIDUES:
        r = ((res - 1868 * b - 9617 * g) * inv) % 16384
        ok = r < 256
        tri = np.stack([b[ok], g[ok], r[ok]], -1).astype(np.uint8)
        assert ((tri.astype(np.int64) * [1868, 9617, 4899]).sum(-1) % 16384 == res).all()
        out.append(tri)
    return out


def gray_edges(W, H, S, n, seed, block=1):
    """Every block x block square of a frame holds one triple: half of them random, the others drawn from the
    four residue classes in turn.  As in `noise`, a stream's later frames redraw one window of the one before."""
    rng = np.random.default_rng(seed)
    tri = gray_edge_triples()

    def draw(ny, nx):
        img = rng.integers(0, 256, (ny, nx, 3), dtype=np.uint8)
        pick = rng.integers(0, 8, (ny, nx))
        for c in range(4):
            m = pick == c
            img[m] = tri[c][rng.integers(0, len(tri[c]), int(m.sum()))]
        return img

    ny, nx = -(-H // block), -(-W // block)
    out = np.empty((n, S, H, W, 3), np.uint8)
    for s in range(S):
        img = draw(ny, nx)
        for i in range(n):
            if i:
                y, x, wh, ww = _window(rng, ny, nx)
                img = img.copy()
                img[y:y + wh, x:x + ww] = draw(wh, ww)
            out[i, s] = np.repeat(np.repeat(img, block, 0), block, 1)[:H, :W]
    return out


def gray_edges_block(W, box):
    """1 without a resize.  Behind INTER_AREA the squares are whole work pixels: 640 -> 100 maps 32 source px
    onto exactly 5, and a constant square resizes to its own value."""
    if W == box:
        return 1
    assert (W, box) == (640, 100)
    return 32


def halves(W, H, S, n):
    """delta_sweep's frames: stream s frame i is black in its first half and white in its second for even i + s,
    the other way round for odd.  The halves are left and right, or top and bottom where the frame is taller than
    wide (at 8 px of width a blur at the seam would reach every column)."""
    out = np.zeros((n, S, H, W, 3), np.uint8)
    second = np.mgrid[:H, :W][1] >= W // 2 if W >= H else np.mgrid[:H, :W][0] >= H // 2
    for i in range(n):
        for s in range(S):
            out[i, s][second == ((i + s) % 2 == 0)] = 255
    return out


SWEEP_EDGE_VALUES = (0, 1, 2, 126, 127, 128, 129, 253, 254, 255)


def sweep_plane(h, w, seed, white_second=True):
    """The written background of delta_sweep, in four bands of rows.  Values (x + 37 y) mod 256 run 0..255 along
    every row and column of the first three: the first adds crafted_plane's fractional parts (.5 ties, values just
    off them, quarters; its first row keeps crafted_plane's negative and oversized values), the second cycles
    through the values next to the tested thresholds instead, so that small images hold enough of each, the third
    is the plain ramp.  The last band equals the sweep frame itself (0 under its black half, 255 under the white
    one): delta 0, so that the mask is not full at the thresholds every other delta passes."""
    yy, xx = np.mgrid[:h, :w]
    p = ((xx + 37 * yy) % 256).astype(np.float64)
    q = max(2, h // 4)
    crafted = crafted_plane(np.zeros((h, w), np.uint8), seed)
    p[:q] += crafted[:q] - np.floor(crafted[:q])
    p[0, :8] = crafted[0, :8]
    p[q:2 * q] = np.asarray(SWEEP_EDGE_VALUES, np.float64)[(xx + 3 * yy) % len(SWEEP_EDGE_VALUES)][q:2 * q]
    second = xx >= w // 2 if w >= h else yy >= h // 2  # as `halves`
    p[3 * q:] = np.where(second == white_second, 255.0, 0.0)[3 * q:]
    return p


# ------------------------------------------------------------------------------------------------------------
# conditions, on the oracle's planes

def mask_fraction(ref):
    return float((ref["mask"] != 0).mean())


def longest_run(plane, value, axis):
    """The longest run of `value` along rows (axis 1) or columns (axis 0)."""
    m = (plane == value)
    if axis == 0:
        m = m.T
    best = 0
    run = np.zeros(m.shape[0], np.int64)
    for j in range(m.shape[1]):
        run = np.where(m[:, j], run + 1, 0)
        best = max(best, int(run.max(initial=0)))
    return best


def residue_counts(small):
    """How often each of GRAY_RESIDUES occurs among the pixels BGR->gray reads (the resized frame)."""
    v = (small.astype(np.int64) * [1868, 9617, 4899]).sum(-1) % 16384
    return [int((v == r).sum()) for r in GRAY_RESIDUES]


def delta_counts(ref, t):
    d = ref["delta"]
    return int((d == t).sum()), int((d == t + 1).sum())


# ------------------------------------------------------------------------------------------------------------
# the cases of the GPU module: (path name, axis, value) -> settings, frames and a background to write

def pixel_cases():
    out = []
    for name in CASES:
        out += [(name, "content", c) for c in ("noise", "cells", "white", "gray_edges")]
        out += [(name, "threshold", t) for t in THRESHOLDS]
        out += [(name, "alpha", a) for a in ALPHAS]
    return out


def case_id(case):
    return "-".join(str(v) for v in case)


def _seed(name, axis, value):
    return [list(CASES).index(name), ("content", "threshold", "alpha").index(axis)] + [ord(ch) for ch in str(value)]


def build_case(name, axis, value):
    """-> dict(thresh, alpha, frames [NB * T][S][H][W][3], write: None or (batch index, [S] planes written through
    set_background before that batch), expect: "partial" | "full" | "empty" | None for the mask condition)."""
    W, H, box, k, h = geometry(name)
    n = NB * T
    seed = _seed(name, axis, value)
    thresh, alpha, write, expect = THRESH, ALPHA, None, "partial"
    if axis == "content":
        if value == "noise":
            thresh = noise_thresh(name)
            fr = noise(W, H, S, n, seed)
        elif value == "cells":
            fr = cells(W, H, S, n, seed, cells_block(k, W / box))
        elif value == "white":
            fr = white(W, H, S, n)
            expect = "white"
        else:
            thresh = noise_thresh(name)
            fr = gray_edges(W, H, S, n, seed, gray_edges_block(W, box))
    elif axis == "threshold":
        thresh = value
        fr = np.concatenate([noise(W, H, S, T, seed), halves(W, H, S, n - T)])
        write = (1, [sweep_plane(h, box, 11 + s, white_second=s % 2 == 0) for s in range(S)])
        expect = "full" if value in FULL else "empty" if value in EMPTY else "partial"
    else:
        alpha = value
        fr = cells(W, H, S, n, seed, cells_block(k, W / box))
    return dict(thresh=thresh, alpha=alpha, frames=fr, write=write, expect=expect)


def run_case(name, axis, value, eng=None):
    """One case on the oracle: NB batches of T frames on S streams, every condition of its content asserted from
    the oracle's planes.  With an engine (created by the caller with the case's settings) the same frames go
    through it and every batch is compared bit for bit: masks, counts, boxes, origins, the float64 background,
    and gray / blur / delta where the engine keeps planes.  Returns the measures the conditions were read from."""
    content = value if axis == "content" else "delta_sweep" if axis == "threshold" else "cells"
    return run_frames(case_id((name, axis, value)), CASES[name][:5], build_case(name, axis, value), content, eng=eng)


def run_frames(cid, geom, c, content, eng=None, T=T, NB=NB):
    """run_case on a geometry (W, H, box, k, keep_planes) that need not be registered in CASES and a build_case
    dict whose frames are [NB * T][S][H][W][3] (any S); `cid` names the case in messages.  The content `patches`
    (ksize_sweep.py: gray_edges in squares of a quarter of the kernel) has two conditions: a steady frame whose
    mask is partial, as the others, and a blur plane that spans at least 40 levels on every steady frame."""
    from find_motion_amd._native import PLANE_BLUR, PLANE_DELTA, PLANE_GRAY

    W, H, box, k, planes = geom
    fr, thresh, alpha = c["frames"], c["thresh"], c["alpha"]
    S = fr.shape[1]
    assert fr.shape[0] == NB * T
    cfg = oracle.OracleConfig(H=H, W=W, box=box, ksize=k, thresh=thresh, alpha=alpha)
    orc = [oracle.OracleStream(cfg) for _ in range(S)]
    if eng is not None:
        assert eng.work_shape == (cfg.h, cfg.w)
        assert (eng.params.threshold, eng.params.avg, eng.keep_planes) == (thresh, alpha, planes)
    m = dict(fractions=[], blur255=0, blur0=0, run_row=0, run_col=0, ties=0, negative=0, above=0,
             residues=None, deltas=None, blur_span=None)
    for b in range(NB):
        if c["write"] and c["write"][0] == b:
            for s, plane in enumerate(c["write"][1]):
                orc[s].set_background(plane)
                if eng is not None:
                    eng.set_background(s, plane)
                    assert np.array_equal(eng.background(s), plane)
        bfr = fr[b * T:(b + 1) * T]
        if eng is not None:
            eng.submit(bfr)
            eng.wait()
            counts = eng.counts()
        for t in range(T):
            for s in range(S):
                first = not orc[s].initialized
                bg_before = orc[s].bg.copy()
                ref = orc[s].step(bfr[t, s])
                at = f"{cid}: batch {b} frame {t} stream {s}"
                assert ref["count"] <= 4096, at
                if eng is not None:
                    if eng.keep_planes:
                        for which, key in ((PLANE_GRAY, "gray"), (PLANE_BLUR, "blur"), (PLANE_DELTA, "delta")):
                            np.testing.assert_array_equal(eng.plane(which, t, s), ref[key], err_msg=f"{key} {at}")
                    np.testing.assert_array_equal(eng.mask(t, s), ref["mask"], err_msg="mask " + at)
                    assert counts[t, s] == ref["count"], at
                    got = eng.contours(t, s)
                    assert [g.bbox for g in got] == ref["boxes"], at
                    assert [g.origin for g in got] == ref["origins"], at
                # --- the conditions ---
                frac = mask_fraction(ref)
                if c["expect"] == "full":
                    assert frac == 1.0, at
                elif c["expect"] == "empty":
                    assert frac == 0.0, at
                if first:
                    continue
                sweep = content == "delta_sweep" and b == 1 and t == 0
                if content != "delta_sweep" or b == 1:
                    m["fractions"].append(frac)
                n255, n0 = int((ref["blur"] == 255).sum()), int((ref["blur"] == 0).sum())
                if content == "white":  # the all-white and the all-black frame: each extreme in a frame of its own
                    m["blur255"], m["blur0"] = max(m["blur255"], n255), max(m["blur0"], n0)
                if content == "cells":  # both extremes, and the runs of 255 that make them, in one frame
                    if min(n255, n0) > min(m["blur255"], m["blur0"]):
                        m["blur255"], m["blur0"] = n255, n0
                        m["run_row"] = longest_run(ref["gray"], 255, 1)
                        m["run_col"] = longest_run(ref["gray"], 255, 0)
                    m["ties"] = max(m["ties"], int((np.abs(bg_before - np.floor(bg_before) - 0.5) == 0).sum()))
                    neg, above = int((bg_before < 0).sum()), int((bg_before > 255).sum())
                    if min(neg, above) > min(m["negative"], m["above"]):
                        m["negative"], m["above"] = neg, above
                if content == "white" and (b, t, s) == (0, 1, 0):  # white after black
                    assert (ref["delta"] == 255).all() and frac == 1.0, at
                if sweep and 0 <= thresh <= 254:
                    lo, hi = delta_counts(ref, thresh)
                    m["deltas"] = (lo, hi) if m["deltas"] is None else (min(lo, m["deltas"][0]), min(hi, m["deltas"][1]))
                if content == "patches":
                    span = int(ref["blur"].max()) - int(ref["blur"].min())
                    m["blur_span"] = span if m["blur_span"] is None else min(span, m["blur_span"])
                if content == "gray_edges":
                    rc = residue_counts(oracle.resize_area_bgr(bfr[t, s], box) if W != box else bfr[t, s])
                    m["residues"] = rc if m["residues"] is None else [min(p, q) for p, q in zip(rc, m["residues"])]
        if eng is not None:
            for s in range(S):
                bg = eng.background(s)
                assert np.array_equal(bg, orc[s].bg), \
                    f"{cid}: batch {b}: background stream {s}: " \
                    f"{int((bg != orc[s].bg).sum())} values differ"
    # --- what the case must have shown ---
    if c["expect"] == "partial":
        assert any(0.02 <= f <= 0.98 for f in m["fractions"]), f"{cid}: mask fractions {m['fractions']}"
    if content in ("cells", "white"):
        assert m["blur255"] >= 50 and m["blur0"] >= 50, f"{cid}: blur == 255 on {m['blur255']}, == 0 on {m['blur0']}"
    if content == "cells":
        assert min(m["run_row"], m["run_col"]) >= k, f"{cid}: runs of 255: {m['run_row']}, {m['run_col']} < {k}"
        if alpha == 0.5:
            assert m["ties"] >= 100, f"{cid}: {m['ties']} background values on a .5 tie"
        if alpha == 1.5:
            assert min(m["negative"], m["above"]) >= 100, f"{cid}: {m['negative']} negative, {m['above']} above 255"
    if content == "gray_edges":
        assert min(m["residues"]) >= 200, f"{cid}: residues {GRAY_RESIDUES} occur {m['residues']} times"
    if content == "patches":
        assert m["blur_span"] >= 40, f"{cid}: a steady frame's blur plane spans {m['blur_span']} levels"
    if content == "delta_sweep" and 0 <= thresh <= 254:
        assert min(m["deltas"]) >= 50, f"{cid}: {m['deltas']} pixels at delta {thresh} and {thresh + 1}"
    return m
