"""Contour points (FM_FLAG_CONTOUR_POINTS) on a machine without a GPU: the two new entry points are
exported, fm_contour keeps its layout with npts where reserved1 was, Contour converts to cv2's
(n, 1, 2) array only when its points were traced, and the option reaches VideoMotion and the CLI
(default off).  The traced points themselves are checked in tests/test_gpu_contour_points.py.
"""
import ctypes as C
import os
import re
from argparse import ArgumentParser

import numpy as np
import pytest

from fake_engine import OracleEngine
from find_motion_amd import _native, cli, motion, videoio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_point_getter_and_the_trace_stats():
    L = _native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "find_motion_amd.h")).read(), flags=re.S)
    for n in ("fm_get_contour_points", "fm_last_trace_stats"):
        assert re.search(r"^\s*int\s+%s\s*\(" % n, header, flags=re.M), n
        assert n in _native.EXPORTED
        assert hasattr(L, n), n
    assert re.search(r"#define\s+FM_FLAG_CONTOUR_POINTS\s+0x10u", header)
    assert _native.FM_FLAG_CONTOUR_POINTS == 0x10
    # null contexts fail cleanly, *total is always set
    total = C.c_size_t(77)
    assert L.fm_get_contour_points(None, 0, 0, None, 0, C.byref(total)) == _native.FM_EINVAL
    assert total.value == 0
    assert L.fm_last_trace_stats(None, None, None, None) == _native.FM_EINVAL


def test_fm_contour_layout_is_unchanged():
    assert C.sizeof(_native.FMContour) == 32
    assert _native.FMContour.npts.offset == 28 and _native.FMContour.npts.size == 4
    assert _native.FMContour.area2.offset == 24
    header = open(os.path.join(ROOT, "include", "find_motion_amd.h")).read()
    body = re.search(r"typedef struct fm_contour \{(.*?)\} fm_contour;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for d in re.findall(r"int32_t\s+([^;]+);", body) for f in d.split(",")]
    assert fields == ["x", "y", "w", "h", "origin_x", "origin_y", "area2", "npts"]
    assert fields == [f[0] for f in _native.FMContour._fields_]


def test_contour_converts_to_cv2_layout_only_with_points():
    pts = np.array([[3, 4], [3, 9], [8, 9], [8, 4]], np.int32).reshape(4, 1, 2)
    c = _native.Contour(3, 4, 6, 6, (3, 4), 25.0, pts)
    a = np.asarray(c)
    assert a.shape == (4, 1, 2) and a.dtype == np.int32
    np.testing.assert_array_equal(a, pts)
    assert np.asarray(c, dtype=np.float32).dtype == np.float32
    np.testing.assert_array_equal(np.array(c), pts)
    bare = _native.Contour(3, 4, 6, 6, (3, 4))
    assert bare.points is None and bare.area is None
    with pytest.raises(TypeError, match="contour_points=True"):
        np.asarray(bare)
    if videoio.cv2 is not None:  # what callers of findContours do with an element of frame.contours
        assert videoio.cv2.contourArea(np.asarray(c)) == 25.0
        assert tuple(videoio.cv2.boundingRect(np.asarray(c))) == c.bbox


def test_option_reaches_video_motion_and_the_cli_and_defaults_off(tmp_path):
    parser = ArgumentParser()
    cli.get_args(parser)
    args = parser.parse_args(["x.avi"])
    assert args.contour_points is False and cli._job_kwargs(args)["contour_points"] is False
    args = parser.parse_args(["x.avi", "--contour-points"])
    assert args.contour_points is True and cli._job_kwargs(args)["contour_points"] is True
    W, H = 192, 108
    for kw, want in (({}, False), ({"contour_points": True}, True)):
        eng = OracleEngine(n_streams=1, src_w=W, src_h=H, box_size=100, ksize=5, threshold=12, avg=0.1, max_batch=4)
        vm = motion.VideoMotion(filename=str(tmp_path / "v"), capture=videoio.SyntheticCapture(W, H, 8, 0), engine=eng,
                                batch=4, box_size=100, threshold=12, outdir=str(tmp_path), **kw)
        assert vm.contour_points is want
        vm.cleanup()
    import inspect

    assert inspect.signature(_native.MotionEngine.__init__).parameters["contour_points"].default is False
    assert inspect.signature(motion.VideoMotion.__init__).parameters["contour_points"].default is False
