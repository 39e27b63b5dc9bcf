"""GPU: every product pixel path on extreme pixel content, thresholds and alphas, bit for bit against the oracle.

The other parity modules feed the kernels the seeded synthetic streams (a smooth gradient, +-3 noise, four flat
rectangles) at threshold 12 and alpha 0.1.  The arithmetic that is only correct inside a value range never meets
its range there: the u16 horizontal blur sums (255 * 256 = 65,280, 255 short of wrapping), the udot2 vertical
pass whose byte 2 is the blur (acc < 2^24), k_pix's v_sad_u8 threshold with its clamp of t to [-1, 255] and
d + bias at d = 255, the udot2 BGR->gray with its coefficients scaled by 4, and convertScaleAbs on negative and
oversized backgrounds.  pixel_content.py makes the content that does, and test_pixel_content_host.py proves on
the oracle that it does.

Paths (pixel_content.CASES): the eight shapes of test_gpu_engine_state.PATHS, the wide path at 328 x 136 k 51,
k_pix<3> and k_pix<7> without planes at 200 x 136, and k_pix5's tile layouts of test_gpu_pix5_loop.py at their
smallest shapes past the small-image path.  Every case: S = 2 with different content per stream, T = 3, two
batches (a first-frame launch, then steady ones); after every batch masks, counts, boxes, origins and the
float64 background are compared exactly, and gray, blur and delta where the path keeps planes.

  content    noise, cells, white, gray_edges at threshold 12 (noise and gray_edges lower where the blur flattens
             them: pixel_content.NOISE_THRESH), alpha 0.1
  threshold  delta_sweep at -5, -1, 0, 1, 127, 254, 255, 300: a new engine per threshold; batch 0 is noise, then a
             background with every value 0..255 is written and the half-black, half-white frames follow
  alpha      cells at 0.0, 0.02, 0.5, 1.0, 1.5 (.5 ties in the background at 0.5; negative values and values
             above 255 at 1.5, where the alpha above 1 overshoots)
"""
import pytest

import pixel_content as pc
from find_motion_amd import MotionEngine

pytestmark = pytest.mark.gpu


def _engine(name, thresh, alpha, **kw):
    W, H, box, k, planes = pc.CASES[name][:5]
    eng = MotionEngine(n_streams=pc.S, src_w=W, src_h=H, box_size=box, ksize=k, threshold=thresh, avg=alpha,
                       max_batch=pc.T, keep_planes=planes, **kw)
    assert eng.pixel_path == pc.PIXEL_PATH[pc.CASES[name][5]], (name, eng.pixel_path)
    return eng


@pytest.mark.parametrize("case", pc.pixel_cases(), ids=pc.case_id)
def test_pixel_case_vs_oracle(case):
    c = pc.build_case(*case)
    eng = _engine(case[0], c["thresh"], c["alpha"])
    try:
        pc.run_case(*case, eng=eng)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(pc.CASES))
def test_shapes_run_the_kernel_they_name(name):
    """Each shape selects the pixel path it stands for on this content too, read from the engine's own launch
    timing: the steady launch, no other path's, and the first-frame launch where the path has one."""
    case = (name, "content", "noise")
    c = pc.build_case(*case)
    launch, init_launch = pc.CASES[name][5:7]
    eng = _engine(name, c["thresh"], c["alpha"], profile="pix")
    try:
        pc.run_case(*case, eng=eng)
        names = {n for n, (ms, cnt) in eng.kernel_times().items() if cnt > 0}
    finally:
        eng.close()
    assert names & pc.STEADY_LAUNCHES == {launch}, names
    if init_launch:
        assert init_launch in names, names
