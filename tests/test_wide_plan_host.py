"""fm_plan on a machine without a GPU: what fm_create would set up for a set of parameters, by the same code.

The query touches no device, so the selection of the pixel path -- in particular of the wide-Gaussian path
(fm_wide.hip: ksize above 49, more than 16 and at most 8,192 tiles, no kept planes) -- is pinned here for the
shapes the GPU tests and the measurement tool use, and so are the refusals fm_create makes before its first
HIP call.
"""
import ctypes as C
import logging
import os
import re

import pytest

import find_motion_amd
from fake_engine import OracleEngine
from find_motion_amd import _native, motion, videoio
from find_motion_amd._native import FM_EINVAL, FM_ENOTSUP, FM_FLAG_KEEP_PLANES, FM_OK, FMError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(**kw):
    p = dict(device=0, n_streams=1, src_w=1920, src_h=1080, box_size=1920, ksize=97, threshold=12, avg=0.1,
             max_batch=4, max_contours=4096, flags=0)
    p.update(kw)
    return _native.FMParams(*p.values())


def test_declared_exported_and_listed():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "find_motion_amd.h")).read(), flags=re.S)
    assert re.search(r"^\s*int\s+fm_plan\s*\(\s*const\s+fm_params\s*\*", src, flags=re.M)
    m = re.search(r"struct\s+fm_plan\s*\{(.*?)\}", src, flags=re.S)
    assert m and [f for f in re.findall(r"(\w+)\s*(?:\[\d+\])?\s*[,;]", m.group(1))] == \
        ["work_h", "work_w", "tiles", "max_inflight", "pixel_path"]
    assert "fm_plan" in _native.EXPORTED
    L = _native.load()
    assert hasattr(L, "fm_plan")
    assert L.fm_abi_version() == 1
    assert C.sizeof(_native.FMPlan) == 32


def test_null_arguments():
    L = _native.load()
    out = _native.FMPlan()
    p = params()
    assert L.fm_plan(None, C.byref(out)) == FM_EINVAL
    assert L.fm_plan(C.byref(p), None) == FM_EINVAL
    assert L.fm_plan(None, None) == FM_EINVAL
    assert L.fm_last_error(None)
    assert L.fm_plan(C.byref(p), C.byref(out)) == FM_OK


# source W x H, box, k, flags -> pixel_path, work (h, w), tiles, max_inflight (None: not pinned)
TABLE = [
    (1920, 1080, 1920, 97, 0, "wide", (1080, 1920), 510, ">=2"),
    (3840, 2160, 3840, 193, 0, "wide", (2160, 3840), 2040, ">=2"),
    (328, 136, 328, 51, 0, "wide", (136, 328), 18, ">=2"),
    (256, 200, 256, 51, 0, "pixel", (200, 256), 16, 1),
    (1920, 1080, 1920, 97, FM_FLAG_KEEP_PLANES, "pixel", (1080, 1920), 510, 1),
    (1920, 1080, 100, 5, 0, "small", (56, 100), 2, None),
    (1920, 1080, 1920, 5, 0, "pix", (1080, 1920), 510, None),
    (640, 480, 640, 11, 0, "fused", (480, 640), 80, None),
    (1100, 72, 1100, 255, 0, "wide", (72, 1100), 36, ">=2"),
    (72, 1100, 72, 255, 0, "wide", (1100, 72), 36, ">=2"),
    (1280, 720, 1280, 65, 0, "wide", (720, 1280), 240, ">=2"),      # -B 1280 -b 20
    (656, 272, 328, 51, 0, "wide", (136, 328), 18, ">=2"),          # a resize in front
    (1920, 1080, 1920, 49, 0, "fused", (1080, 1920), 510, None),    # the last k of k_fused
    (1920, 1080, 1920, 51, 0, "wide", (1080, 1920), 510, ">=2"),    # the first k past it
]


@pytest.mark.parametrize("W,H,box,k,flags,path,work,tiles,depth", TABLE)
def test_selection_table(W, H, box, k, flags, path, work, tiles, depth):
    L = _native.load()
    out = _native.FMPlan()
    p = params(src_w=W, src_h=H, box_size=box, ksize=k, flags=flags)
    assert L.fm_plan(C.byref(p), C.byref(out)) == FM_OK, L.fm_last_error(None)
    assert out.pixel_path.decode() == path
    assert (out.work_h, out.work_w) == work == (find_motion_amd.work_height(H, W, box), box)
    assert out.tiles == tiles == ((work[0] + 63) // 64) * ((work[1] + 63) // 64)
    if depth == ">=2":
        assert out.max_inflight >= 2
    elif depth is not None:
        assert out.max_inflight == depth
    assert out.max_inflight >= 1
    # the Python binding says the same
    got = _native.plan(src_w=W, src_h=H, box_size=box, ksize=k, keep_planes=bool(flags & FM_FLAG_KEEP_PLANES),
                       max_batch=4)
    assert got == {"work_shape": work, "tiles": tiles, "max_inflight": out.max_inflight, "pixel_path": path}


# The paths that flags select, and what they refuse: source W x H, box, k, max_batch, flags -> return code,
# pixel_path, max_inflight.  A colour slot's blur scratch is 3 B per pixel-frame with the rows padded to whole
# tiles: 1080p at 42 frames is 3 * 1920 * 1088 * 42 = 263,208,960 B, under the 256 MiB above which a context
# keeps 4 slots, and at 43 frames 269,475,840 B, over it.
COLOUR, MOG2, PLANES = _native.FM_FLAG_COLOUR_MOTION, _native.FM_FLAG_MOG2, FM_FLAG_KEEP_PLANES
FLAG_TABLE = [
    (1920, 1080, 1920, 5, 42, COLOUR, FM_OK, "rgb", 10),
    (1920, 1080, 1920, 5, 43, COLOUR, FM_OK, "rgb", 4),
    (1920, 1080, 100, 5, 4, COLOUR, FM_OK, "rgb", 10),             # (the small path's shape: colour takes it over)
    (1920, 1080, 1920, 49, 4, COLOUR, FM_OK, "rgb", 10),
    (1920, 1080, 1920, 51, 4, COLOUR, FM_ENOTSUP, "", 0),           # colour takes ksize up to 49
    (1920, 1080, 100, 5, 4, MOG2, FM_OK, "mog2", 4),               # k_small_blur in front
    (1920, 1080, 1920, 5, 4, MOG2, FM_OK, "mog2", 4),              # k_wide_blur in front
    (328, 136, 328, 5, 4, MOG2, FM_OK, "mog2", 4),
    (1920, 1080, 1920, 97, 4, MOG2, FM_OK, "mog2", 4),
    (1920, 1080, 1920, 5, 4, MOG2 | COLOUR, FM_ENOTSUP, "", 0),
    (1920, 1080, 1920, 5, 4, MOG2 | PLANES, FM_ENOTSUP, "", 0),
    (1920, 1080, 1920, 5, 4, COLOUR | PLANES, FM_ENOTSUP, "", 0),
    (1920, 1080, 100, 5, 4, 0, FM_OK, "small", 10),
    (1920, 1080, 100, 5, 4, PLANES, FM_OK, "pix", 10),             # kept planes: k_pix writes them
    (1920, 1080, 1920, 5, 4, 0, FM_OK, "pix", 10),
    (640, 480, 640, 11, 4, 0, FM_OK, "fused", 10),
    (1920, 1080, 1920, 97, 4, 0, FM_OK, "wide", 4),
    (1920, 1080, 1920, 97, 4, PLANES, FM_OK, "pixel", 1),
]


@pytest.mark.parametrize("W,H,box,k,batch,flags,code,path,depth", FLAG_TABLE)
def test_flag_selection_table(W, H, box, k, batch, flags, code, path, depth):
    L = _native.load()
    out = _native.FMPlan()
    p = params(src_w=W, src_h=H, box_size=box, ksize=k, max_batch=batch, flags=flags)
    assert L.fm_plan(C.byref(p), C.byref(out)) == code, L.fm_last_error(None)
    assert (out.pixel_path.decode(), out.max_inflight) == (path, depth)
    if code != FM_OK:
        assert L.fm_last_error(None)
        h = C.c_void_p()
        assert L.fm_create(C.byref(h), C.byref(p)) == code and not h.value


def test_every_odd_ksize_above_49_fits():
    """The wide kernels' LDS need fits for every odd k from 51 to 255 (the ring of row sums shrinks the strip
    from 512 to 256 columns where it has to)."""
    for k in range(51, 256, 2):
        assert _native.plan(src_w=1920, src_h=1080, box_size=1920, ksize=k)["pixel_path"] == "wide", k
        assert _native.plan(src_w=328, src_h=136, box_size=328, ksize=k)["pixel_path"] == "wide", k
        assert _native.plan(src_w=256, src_h=200, box_size=256, ksize=k)["pixel_path"] == "pixel", k


def test_tile_count_bounds():
    """More than 16 tiles and at most 8,192: 17 tiles is in, 8,192 is in, the next tile column is out."""
    assert _native.plan(src_w=1088, src_h=64, box_size=1088, ksize=51)["tiles"] == 17
    assert _native.plan(src_w=1088, src_h=64, box_size=1088, ksize=51)["pixel_path"] == "wide"
    assert _native.plan(src_w=1024, src_h=64, box_size=1024, ksize=51)["pixel_path"] == "pixel"  # 16 tiles
    big = _native.plan(src_w=8192, src_h=4096, box_size=8192, ksize=51)
    assert (big["tiles"], big["pixel_path"]) == (8192, "wide")
    over = _native.plan(src_w=8256, src_h=4096, box_size=8256, ksize=51)
    assert over["tiles"] > 8192 and over["pixel_path"] == "pixel" and over["max_inflight"] == 1


BAD = [
    (dict(ksize=4), FM_EINVAL), (dict(ksize=0), FM_EINVAL), (dict(ksize=257), FM_EINVAL), (dict(ksize=-3), FM_EINVAL),
    (dict(n_streams=0), FM_EINVAL), (dict(box_size=0), FM_EINVAL), (dict(max_batch=0), FM_EINVAL),
    (dict(max_contours=0), FM_EINVAL), (dict(src_w=0), FM_EINVAL), (dict(src_h=0), FM_EINVAL),
    (dict(avg=float("nan")), FM_EINVAL),
    (dict(src_w=1920, src_h=1, box_size=100), FM_EINVAL),        # work height 0
    (dict(src_w=64, src_h=48, box_size=128), FM_ENOTSUP),        # box > width: INTER_AREA upscaling
]


@pytest.mark.parametrize("kw,code", BAD)
def test_bad_parameters_are_refused_with_fm_create_codes(kw, code):
    """Each refusal is made by the code fm_create runs before its first HIP call, so fm_create itself can be
    asked on a machine without a GPU: both return the same code, and neither leaves a result."""
    L = _native.load()
    p = params(**kw)
    out = _native.FMPlan()
    out.tiles = 77
    assert L.fm_plan(C.byref(p), C.byref(out)) == code
    assert L.fm_last_error(None)
    assert (out.tiles, out.max_inflight, out.pixel_path) == (0, 0, b"")
    h = C.c_void_p()
    assert L.fm_create(C.byref(h), C.byref(p)) == code and not h.value
    with pytest.raises(FMError) as e:
        _native.plan(**{**dict(src_w=1920, src_h=1080, box_size=1920, ksize=97), **kw})
    assert e.value.code == code


class _PathEngine(OracleEngine):
    def __init__(self, path, tiles, **kw):
        super().__init__(**kw)
        self.pixel_path, self.tiles = path, tiles
        self.max_inflight = 1 if path == "pixel" else 4


def _video(tmp_path, path, tiles, W=192, H=108, box=192, **kw):
    k = motion.make_gaussian_size(box, 2)
    eng = _PathEngine(path, tiles, n_streams=1, src_w=W, src_h=H, box_size=box, ksize=k, threshold=12, avg=0.1,
                      keep_planes=kw.get("keep_planes", False))
    return motion.VideoMotion(filename=str(tmp_path / "vid"), capture=videoio.SyntheticCapture(W, H, 4, 0), engine=eng,
                              box_size=box, blur_scale=2, outdir=str(tmp_path), threshold=12, **kw)


def test_video_motion_logs_the_path(tmp_path, caplog):
    """One INFO line per video naming the path; a WARNING on the per-frame path that says which condition put
    the video there."""
    with caplog.at_level(logging.INFO, logger="find_motion_amd.VideoMotion"):
        _video(tmp_path, "wide", 40)  # (the constructor loads the video)
    info = [r for r in caplog.records if r.levelno == logging.INFO and "pixel path" in r.getMessage()]
    assert len(info) == 1 and "'wide'" in info[0].getMessage()
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="find_motion_amd.VideoMotion"):
        _video(tmp_path, "pixel", 6)
    warn = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warn) == 1 and "6 tiles" in warn[0] and "more than 16" in warn[0]
    assert len([r for r in caplog.records if r.levelno == logging.INFO and "'pixel'" in r.getMessage()]) == 1
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="find_motion_amd.VideoMotion"):
        vm = _video(tmp_path, "pixel", 40)
        caplog.clear()
        vm.keep_planes = True
        vm._log_pixel_path()
    warn = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warn) == 1 and "planes are kept" in warn[0]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="find_motion_amd.VideoMotion"):
        _video(tmp_path, "pixel", 9000)
    warn = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warn) == 1 and "9000 tiles" in warn[0] and "8192" in warn[0]
