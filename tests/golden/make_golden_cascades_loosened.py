#!/usr/bin/env python3
"""Fixture for the object-ROI stage on every cascade the drop-in can load, with loosened stage
thresholds (tests/golden/cascades_loosened.npz).

Run from the repository root (CPU only; about three minutes with one process per cascade):

    python tests/golden/make_golden_cascades_loosened.py

With their trained thresholds the nine cascades of CASCADE_LOOKUP give no candidate on the
synthetic test images (almost every window dies in stages 0-3), so a parity test would compare
empty lists.  tests/haar_cases.loosen lowers each stage threshold by lam times the stage's leaf
spread; features, node thresholds, trees and leaves stay the reference's.  For each cascade and
each of two images -- roi = make_image(2) (300x169, the product's ROI shape) and
small = make_image(2, w=128, h=80), regenerated from the seed by the tests -- the fixture holds
lam, the loosened stage thresholds, oracle/haar.py's candidates at scale factor 1.1 and the
grouped detections at minNeighbors 3.

lam is the first value of 0.04, 0.05, ..., 0.12 for which the roi image gives
20 <= candidates <= 1000 (below the device candidate lists' capacity), at least one grouped
detection, and at least 100 windows rejected in stages >= 4 (after the head / tail split of the
device sweep); the small image must then give at least 4 candidates.  All of it is asserted here.

Chosen values (candidates / detections / windows rejected in stages >= 4), as main() prints them:

    frontalcatface           lam 0.05  roi  109 /  4 / 11964   small   27 /  1 /  2030
    frontalcatface_extended  lam 0.05  roi  121 /  5 /  9850   small   17 /  1 /  1790
    frontalface_alt          lam 0.04  roi  330 / 11 /  6442   small   74 /  4 /  1289
    frontalface_alt2         lam 0.04  roi  175 / 10 /  5305   small   43 /  2 /  1049
    frontalface_alt_tree     lam 0.06  roi   60 /  3 /  5898   small   10 /  1 /  1296
    frontalface_default      lam 0.04  roi   50 /  3 /  3402   small   13 /  1 /   593
    fullbody                 lam 0.04  roi   43 /  1 /  8436   small    8 /  0 /  1038
    lowerbody                lam 0.04  roi   77 /  4 / 12095   small    7 /  1 /  1540
    profileface              lam 0.04  roi  189 /  7 / 10069   small   61 /  2 /  2036

(lam 0.04 left frontalcatface with 9 and frontalcatface_extended with 11 candidates, and
frontalface_alt_tree without a grouped detection up to 0.05.)

Parity vs OpenCV itself stays unpinned (cv2 is absent); this pins the GPU path to the
restatement on the reference's real features, trees and stage sizes.
"""
import io
import os
import sys
import zipfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from find_motion_amd import cascade  # noqa: E402
from golden_cases import cascade_xml  # noqa: E402
from haar_cases import candidates_and_results, loosen, make_image  # noqa: E402
from oracle import haar  # noqa: E402

LADDER = [k / 100 for k in range(4, 13)]
SPLIT = 4  # the device sweep's head runs stages [0, 4)


def images():
    return {"roi": make_image(2), "small": make_image(2, w=128, h=80)}


def run(cs, img):
    cand, res = candidates_and_results(cs, img, 1.1)
    return cand, haar.group_rectangles(cand, 3), int((res <= -SPLIT).sum())


def choose(name):
    """The first lam of the ladder that meets the conditions on the roi image, and both images' results."""
    base = cascade.parse(cascade_xml(name))
    imgs = images()
    for lam in LADDER:
        cs = loosen(base, lam)
        cand, det, late = run(cs, imgs["roi"])
        print(f"{name} lam {lam:.2f} roi: {len(cand)} candidates, {len(det)} detections, {late} rejected late",
              flush=True)
        if 20 <= len(cand) <= 1000 and len(det) >= 1 and late >= 100:
            break
    else:
        raise AssertionError(f"{name}: no lam of the ladder meets the conditions; refine the ladder for it")
    out = {"lam": lam, "stage_threshold": cs.stage_threshold, "roi": (cand, det, late)}
    out["small"] = run(cs, imgs["small"])
    assert len(out["small"][0]) >= 4, (name, len(out["small"][0]))
    return name, out


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that a rerun gives the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def main():
    names = list(cascade.CASCADE_LOOKUP)
    with ProcessPoolExecutor(max_workers=min(len(names), os.cpu_count() or 1)) as ex:
        done = dict(ex.map(choose, names))
    arrays = {}
    for name in names:
        d = done[name]
        arrays[f"{name}__lam"] = np.float64(d["lam"])
        arrays[f"{name}__stage_threshold"] = d["stage_threshold"]
        for im in ("roi", "small"):
            cand, det, late = d[im]
            arrays[f"{name}__{im}_candidates"] = np.asarray(cand, np.int32).reshape(-1, 4)
            arrays[f"{name}__{im}_detections"] = np.asarray(det, np.int32).reshape(-1, 4)
            arrays[f"{name}__{im}_late"] = np.int32(late)
        print(f"    {name:24s} lam {d['lam']:.2f}  roi {len(d['roi'][0]):4d} / {len(d['roi'][1]):2d} / {d['roi'][2]:5d}"
              f"   small {len(d['small'][0]):4d} / {len(d['small'][1]):2d} / {d['small'][2]:5d}")
    write_npz(os.path.join(HERE, "cascades_loosened.npz"), arrays)


if __name__ == "__main__":
    main()
