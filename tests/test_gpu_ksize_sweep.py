"""GPU: every Gaussian size on every pixel path, bit for bit against the oracle.

The other parity modules run k = 1, 3, 5, 11, 21, 51 and 97 (and 9, 33, 65, 255 once or on one path).  Every odd
k from 1 to 255 is a configuration make_gaussian reaches, and each kernel's geometry follows from it: Layout(r),
nchunks against the fixed chunks per thread and cfl[64] in k_fused<0>; span, rp, the trimmed zero ends and the
switch from 256 to 128 threads between k 171 and 173 in k_wide_blur; the LDS limit that sends 113 x 114 to the
small path at k 27 and past it at k 29; k_pixel's dynamic LDS above 64 KiB from k 157 on; and REFLECT_101 folding
more than once where the radius passes the image.  ksize_sweep.py lists the cases and
test_ksize_sweep_host.py proves their content on the oracle.

  light   every size once per path (small and fused / pix: every odd k to 49; wide: every odd k from 51 to 255;
          pixel: seven sizes on two shapes), S = 1, T = 2, two batches, `patches`
  full    the class edges of each kernel at S = 2, T = 3, two batches on `noise` at threshold 0, `white` and
          `patches`, with the gray, blur and delta planes compared where they are kept

Every test asserts the engine's pixel_path, runs the case beside the engine (masks, counts, boxes, origins, the
float64 background after every batch, kept planes: all exact) and asserts from the engine's own launch timing that
the case's steady launch ran and no other path's did.
"""
import pytest

import ksize_sweep as ks
import pixel_content as pc
from find_motion_amd import MotionEngine

pytestmark = pytest.mark.gpu

STEADY = set(ks.LAUNCH.values())


def _run(case, content, light):
    W, H, k, planes, path, launch = case
    S, T, NB, thresh, alpha = ks.settings(case, content, light)
    eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=W, ksize=k, threshold=thresh, avg=alpha,
                       max_batch=T, keep_planes=planes, profile="pix")
    try:
        assert eng.pixel_path == path == pc.PIXEL_PATH[launch], (ks.case_id(case), eng.pixel_path)
        ks.run(case, content, light, eng=eng)
        times = eng.kernel_times()
    finally:
        eng.close()
    names = {n for n, (ms, cnt) in times.items() if cnt > 0}
    assert times[launch][1] > 0 and names & STEADY == {launch}, names


@pytest.mark.parametrize("case", ks.light_cases(), ids=ks.case_id)
def test_every_size_vs_oracle(case):
    _run(case, "patches", light=True)


@pytest.mark.parametrize("item", ks.full_cases(), ids=ks.full_id)
def test_class_edges_vs_oracle(item):
    _run(item[0], item[1], light=False)
