"""Every Gaussian size on every pixel path: the cases of test_gpu_ksize_sweep.py, provable without a GPU.

The size k is box_size / blur_scale forced odd (make_gaussian), so every odd k from 1 to 255 is a configuration a
user reaches from the command line, and every pixel kernel's geometry is a function of it: the LDS layout, the
halo, how many taps a lane packs, where REFLECT_101 folds and which kernel runs at all.  A case here is

    (W, H, k, keep_planes, expected pixel_path, expected steady launch name)

with box = W (no resize).  light_cases() holds every size once per path at S = 1, T = 2 and two batches (a
first-frame launch, a steady frame, then a steady batch) on `patches`; full_cases() is the subset at the class
edges of each kernel, run at pixel_content's S = 2, T = 3, NB = 2 on `noise` at threshold 0, `white` and `patches`.

  patches   pixel_content.gray_edges in squares of max(1, k // 4) px: random full-range triples and the
            gray-rounding edge triples, a quarter of the kernel wide.  Per-pixel noise under a wide kernel leaves a
            blur plane of four levels (126..129 at k >= 171) that a wrong tap hardly moves; this does not.
            Conditions, from the oracle's planes: some steady frame's mask covers 2 .. 98 % of the image, and every
            steady frame's blur plane spans at least 40 levels.  Threshold 4, alpha 0.1.
  noise     pixel_content.noise at threshold 0 (steady masks lie between 13 % and 100 %): some frame partial
  white     pixel_content.white with its conditions

run() drives a case through pixel_content.run_frames: on the oracle alone, asserting the conditions, or beside an
engine, comparing masks, counts, boxes, origins, the float64 background after every batch (on a first-frame batch
the blur plane itself) and the kept planes bit for bit.
"""
import pixel_content as pc

ODD_SMALL = tuple(range(1, 50, 2))      # the sizes k_fused, k_pix and k_small_blur take
ODD_WIDE = tuple(range(51, 256, 2))     # the sizes k_wide_blur and k_pixel take
PIX_K = (3, 5, 7, 21)                   # k_pix's instantiations
PIXEL_K = (51, 53, 99, 155, 157, 253, 255)  # k_pixel: both ends, and both sides of 64 KiB of dynamic LDS

LAUNCH = {"small": "small_scan", "pix": "pix", "fused": "fused", "wide": "wide_scan", "pixel": "pixel"}
PATCH_THRESH, NOISE_THRESH = 4, 0
LIGHT_S, LIGHT_T, LIGHT_NB = 1, 2, 2
CONTENTS = ("noise", "white", "patches")


def _case(W, H, k, path, planes=False):
    return (W, H, k, planes, path, LAUNCH[path])


def _tile_path(k):
    return "pix" if k in PIX_K else "fused"


def light_cases():
    out = [_case(100, 56, k, "small") for k in ODD_SMALL]
    out += [_case(200, 136, k, _tile_path(k)) for k in ODD_SMALL]
    out += [_case(328, 136, k, "wide") for k in ODD_WIDE]
    out += [_case(W, H, k, "pixel") for W, H in ((256, 200), (100, 56)) for k in PIXEL_K]
    return out


def full_cases():
    out = [_case(200, 136, k, "fused") for k in (1, 9, 13, 19, 23, 35, 49)]
    out += [_case(200, 136, k, "fused", planes=True) for k in (1, 9, 13, 33, 49)]
    # span = 3 (mod 4) with an odd rp on 256 threads (53, 99), the last size on 256 threads and the first on 128
    # (171, 173), and the largest
    out += [_case(328, 136, k, "wide") for k in (53, 99, 171, 173, 255)]
    out += [_case(256, 200, k, "pixel", planes=True) for k in (51, 157, 255)]
    # the small path's LDS limit: 65,528 of 65,536 B at k 27, past it at k 29
    out += [_case(113, 114, 27, "small"), _case(113, 114, 29, "fused")]
    # a radius past the image: REFLECT_101 folds more than once
    out += [_case(8, 2056, 7, "pix"), _case(8, 2056, 21, "pix"), _case(12, 1400, 21, "pix")]
    out += [_case(W, H, k, "fused") for W, H in ((20, 900), (900, 20)) for k in (23, 49)]
    out += [_case(8, 2056, 255, "wide"), _case(100, 56, 255, "pixel")]
    return [(c, content) for c in out for content in CONTENTS]


def case_id(case):
    W, H, k, planes, path = case[:5]
    return f"{path}-{W}x{H}-k{k}" + ("-planes" if planes else "")


def full_id(item):
    return f"{case_id(item[0])}-{item[1]}"


# A case whose content misses its conditions at seed 0 gets another one here (never another bound), keyed by
# (case id, content, light).  All are 100 x 56 under a kernel wider than the image, where `patches` is a few
# squares of 38 (k 155) to 63 px (k 255) and most draws leave a blur plane of under 40 levels.
SEEDS = {
    ("pixel-100x56-k155", "patches", True): 1,
    ("pixel-100x56-k253", "patches", True): 70,
    ("pixel-100x56-k255", "patches", True): 28,
    ("pixel-100x56-k255", "patches", False): 2701,
}


def build(case, content, S, n, light=False):
    """pixel_content.build_case's dict for a sweep case: settings, [n][S][H][W][3] frames, the mask condition."""
    W, H, k, planes = case[:4]
    seed = [W, H, k, int(planes), CONTENTS.index(content), SEEDS.get((case_id(case), content, light), 0)]
    thresh, expect = pc.THRESH, "partial"
    if content == "noise":
        thresh, fr = NOISE_THRESH, pc.noise(W, H, S, n, seed)
    elif content == "white":
        fr, expect = pc.white(W, H, S, n), "white"
    else:
        thresh, fr = PATCH_THRESH, pc.gray_edges(W, H, S, n, seed, block=max(1, k // 4))
    return dict(thresh=thresh, alpha=pc.ALPHA, frames=fr, write=None, expect=expect)


def settings(case, content, light):
    """-> (S, T, NB, threshold, alpha) of a case, for the engine's constructor."""
    S, T, NB = (LIGHT_S, LIGHT_T, LIGHT_NB) if light else (pc.S, pc.T, pc.NB)
    thresh = {"noise": NOISE_THRESH, "white": pc.THRESH, "patches": PATCH_THRESH}[content]
    return S, T, NB, thresh, pc.ALPHA


def run(case, content, light, eng=None):
    W, H, k, planes = case[:4]
    S, T, NB = settings(case, content, light)[:3]
    c = build(case, content, S, NB * T, light)
    cid = ("light-" if light else "") + full_id((case, content))
    return pc.run_frames(cid, (W, H, W, k, planes), c, content, eng=eng, T=T, NB=NB)
