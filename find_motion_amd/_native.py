"""ctypes binding of include/find_motion_amd.h (libfm_hip.so, built in-tree).

This is the only way the package reaches the hot path: there is no CPU
fallback.  If the HIP library is missing, importing the engine raises
NativeLibraryMissing with the build command.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libfm_hip.so")
# development override: an alternative build of the same library (A/B kernel variants)
LIB_PATH = os.environ.get("FM_HIP_LIB") or LIB_PATH  # unset or empty: the in-tree product library

FM_OK, FM_EINVAL, FM_EHIP, FM_ENOMEM, FM_ESTATE, FM_ENOTSUP = 0, -1, -2, -3, -4, -5
FM_FLAG_KEEP_PLANES, FM_FLAG_PROFILE, FM_FLAG_PROFILE_PIX, FM_FLAG_CONTOUR_AREA = 0x1, 0x2, 0x4, 0x8
FM_FLAG_CONTOUR_POINTS = 0x10
FM_FLAG_AREA_UPSCALE = 0x20
FM_FLAG_COLOUR_MOTION = 0x40
FM_FLAG_MOG2 = 0x80
RESIZE_IDENTITY, RESIZE_FAST, RESIZE_GENERAL, RESIZE_UP = 0, 1, 2, 3
RESIZE_NAMES = ("identity", "area_fast", "area", "area_up")
PLANE_GRAY, PLANE_BLUR, PLANE_DELTA, PLANE_SMALL = 0, 1, 2, 3

EXPORTED = (
    "fm_abi_version", "fm_create", "fm_destroy", "fm_last_error", "fm_work_size", "fm_set_mask",
    "fm_reset_stream", "fm_submit", "fm_wait", "fm_get_counts", "fm_get_contours", "fm_read_mask",
    "fm_read_plane", "fm_read_background", "fm_write_background", "fm_set_hip_stream",
    "fm_kernel_times", "fm_kernel_time_spread", "fm_kernel_time_busy", "fm_kernel_time_stats", "fm_reset_kernel_times", "fm_rasterize_masks", "fm_max_inflight",
    "fm_host_alloc", "fm_host_free", "fm_last_fallbacks", "fm_last_ccl_stats",
    "fm_haar_create", "fm_haar_destroy", "fm_haar_last_error", "fm_haar_window", "fm_haar_detect",
    "fm_haar_candidates", "fm_haar_last_ms", "fm_haar_detect_frames",
    "fm_mjpeg_create", "fm_mjpeg_destroy", "fm_mjpeg_last_error", "fm_mjpeg_decode", "fm_mjpeg_last_ms",
    "fm_submit_jpeg", "fm_read_frame", "fm_mjpeg_tune", "fm_frame_device", "fm_mjpeg_geometry",
    "fm_submit_streams", "fm_footprint", "fm_haar_detect_frame_list", "fm_haar_detect_frame_list_async",
    "fm_haar_collect", "fm_haar_last_sweep",
    "fm_jpeg_header", "fm_mjpeg_enc_create", "fm_mjpeg_enc_destroy", "fm_mjpeg_enc_last_error", "fm_mjpeg_encode",
    "fm_mjpeg_encode_frame_list", "fm_mjpeg_enc_get", "fm_mjpeg_enc_coefficients", "fm_mjpeg_enc_last_ms",
    "fm_get_contour_points", "fm_last_trace_stats",
    "fm_yuv_frame_bytes", "fm_submit_yuv", "fm_submit_yuv_list",
    "fm_yolo_create", "fm_yolo_destroy", "fm_yolo_last_error", "fm_yolo_layer_shape", "fm_yolo_detect_frames",
    "fm_yolo_detect_frame_list", "fm_yolo_forward", "fm_yolo_decode", "fm_yolo_layer_output",
    "fm_yolo_route_in_place", "fm_yolo_last_ms", "fm_yolo_create_precision", "fm_yolo_precision",
    "fm_plan", "fm_read_threshold_bits",
    "fm_resize_kind", "fm_area_up_taps", "fm_haar_set_roi_upscale", "fm_yolo_set_roi_upscale",
    "fm_gaussian_taps",
    "fm_haar_bank_create", "fm_haar_bank_destroy", "fm_haar_bank_last_error", "fm_haar_bank_size",
    "fm_haar_bank_detect", "fm_haar_bank_set_roi_upscale", "fm_haar_bank_detect_frames",
    "fm_haar_bank_detect_frame_list", "fm_haar_bank_detect_frame_list_async", "fm_haar_bank_collect",
    "fm_haar_bank_candidates", "fm_haar_bank_last_ms",
    "fm_retain_reserve", "fm_retain_frames", "fm_release_frames", "fm_read_retained", "fm_retained_count",
    "fm_background_channels",
    "fm_mog2_defaults", "fm_create_mog2", "fm_mog2_read_model", "fm_mog2_write_model", "fm_mog2_background",
)
YOLO_CONV, YOLO_MAXPOOL, YOLO_UPSAMPLE, YOLO_ROUTE, YOLO_SHORTCUT, YOLO_HEAD = range(6)
YOLO_CAND = 9  # floats per decoded row: head, row, bx, by, bw, bh, obj, class, p
YOLO_PRECISIONS = {"f32": 0, "f16": 1}  # FM_YOLO_F32, FM_YOLO_F16
# fm_yuv_layout.format (FM_YUV_*), by fourcc
YUV_NV12, YUV_I420, YUV_YUY2, YUV_UYVY = 0, 1, 2, 3
YUV_FORMATS = {"NV12": YUV_NV12, "I420": YUV_I420, "IYUV": YUV_I420, "YUY2": YUV_YUY2, "YUYV": YUV_YUY2,
               "UYVY": YUV_UYVY}


class NativeLibraryMissing(ImportError):
    pass


class FMError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"find_motion_amd error {code}: {msg}")
        self.code = code


class FMParams(C.Structure):
    _fields_ = [("device", C.c_int), ("n_streams", C.c_int), ("src_w", C.c_int), ("src_h", C.c_int),
                ("box_size", C.c_int), ("ksize", C.c_int), ("threshold", C.c_int), ("avg", C.c_double),
                ("max_batch", C.c_int), ("max_contours", C.c_int), ("flags", C.c_uint)]


class Mog2Params(C.Structure):
    """fm_mog2_params: BackgroundSubtractorMOG2's parameters (five mixtures).  Mog2Params() holds OpenCV's defaults;
    keyword arguments override them."""
    _fields_ = [("history", C.c_int), ("var_threshold", C.c_float), ("var_threshold_gen", C.c_float),
                ("background_ratio", C.c_float), ("var_init", C.c_float), ("var_min", C.c_float),
                ("var_max", C.c_float), ("complexity_reduction", C.c_float), ("shadow_tau", C.c_float),
                ("detect_shadows", C.c_int), ("learning_rate", C.c_double)]
    DEFAULTS = dict(history=500, var_threshold=16.0, var_threshold_gen=9.0, background_ratio=0.9, var_init=15.0,
                    var_min=4.0, var_max=75.0, complexity_reduction=0.05, shadow_tau=0.5, detect_shadows=1,
                    learning_rate=-1.0)

    def __init__(self, **kw):
        unknown = set(kw) - set(self.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown MOG2 parameter(s): {sorted(unknown)}")
        vals = dict(self.DEFAULTS, **kw)
        vals["detect_shadows"] = int(bool(vals["detect_shadows"]))
        super().__init__(**vals)

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


def mog2_params(mog2) -> "Mog2Params | None":
    """MotionEngine's mog2 argument as parameters: None / False = off, True = the defaults, a dict of overrides,
    or a Mog2Params."""
    if mog2 is None or mog2 is False:
        return None
    if mog2 is True:
        return Mog2Params()
    if isinstance(mog2, Mog2Params):
        return mog2
    if isinstance(mog2, dict):
        return Mog2Params(**mog2)
    raise TypeError("mog2 must be None, True, a dict or a Mog2Params")


class FMPlan(C.Structure):
    _fields_ = [("work_h", C.c_int32), ("work_w", C.c_int32), ("tiles", C.c_int32), ("max_inflight", C.c_int32),
                ("pixel_path", C.c_char * 16)]


class FMHaarDesc(C.Structure):
    _fields_ = [("win_w", C.c_int32), ("win_h", C.c_int32), ("n_stages", C.c_int32), ("n_trees", C.c_int32),
                ("n_nodes", C.c_int32), ("n_leaves", C.c_int32), ("n_features", C.c_int32),
                ("stage_ntrees", C.c_void_p), ("stage_threshold", C.c_void_p), ("tree_nodes", C.c_void_p),
                ("node_left", C.c_void_p), ("node_right", C.c_void_p), ("node_feature", C.c_void_p),
                ("node_threshold", C.c_void_p), ("leaves", C.c_void_p), ("feat_rects", C.c_void_p),
                ("feat_weights", C.c_void_p), ("feat_tilted", C.c_void_p)]


class FMYoloLayer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("filters", C.c_int32), ("size", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("leaky", C.c_int32), ("src", C.c_int32 * 2), ("weight_ofs", C.c_int64),
                ("bias_ofs", C.c_int64), ("n_mask", C.c_int32), ("anchor_ofs", C.c_int32)]


class FMYoloDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("layers", C.POINTER(FMYoloLayer)), ("weights", C.c_void_p),
                ("n_weights", C.c_int64), ("biases", C.c_void_p), ("n_biases", C.c_int64), ("anchors", C.c_void_p),
                ("n_anchors", C.c_int32), ("channels", C.c_int32), ("net_w", C.c_int32), ("net_h", C.c_int32),
                ("classes", C.c_int32), ("max_frames", C.c_int32), ("zero_thresh", C.c_float)]


class FMYuvLayout(C.Structure):
    _fields_ = [("format", C.c_int), ("pitch", C.c_int), ("chroma_offset", C.c_int), ("frame_stride", C.c_size_t)]


class FMContour(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("origin_x", C.c_int32), ("origin_y", C.c_int32), ("area2", C.c_int32),
                ("npts", C.c_int32)]


_lib = None


def load() -> C.CDLL:
    """Load libfm_hip.so (raises NativeLibraryMissing if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found: build the HIP extension with "
            f"`make -C {os.path.join(_PKG, 'csrc')}` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    vp, i32, u8p = C.c_void_p, C.c_int, C.c_void_p
    L.fm_abi_version.restype = i32
    L.fm_create.argtypes = [C.POINTER(vp), C.POINTER(FMParams)]
    L.fm_destroy.argtypes = [vp]
    L.fm_destroy.restype = None
    L.fm_last_error.argtypes = [vp]
    L.fm_last_error.restype = C.c_char_p
    L.fm_work_size.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.fm_set_mask.argtypes = [vp, i32, u8p]
    L.fm_reset_stream.argtypes = [vp, i32]
    L.fm_submit.argtypes = [vp, vp, i32, i32]
    L.fm_wait.argtypes = [vp]
    L.fm_get_counts.argtypes = [vp, vp]
    L.fm_get_contours.argtypes = [vp, i32, i32, vp, i32]
    L.fm_read_mask.argtypes = [vp, i32, i32, vp]
    L.fm_read_threshold_bits.argtypes = [vp, i32, i32, vp]
    L.fm_read_plane.argtypes = [vp, i32, i32, i32, vp]
    L.fm_read_background.argtypes = [vp, i32, vp]
    L.fm_write_background.argtypes = [vp, i32, vp]
    L.fm_set_hip_stream.argtypes = [vp, vp]
    L.fm_kernel_times.argtypes = [vp, vp, vp, vp, i32]
    L.fm_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.fm_host_free.argtypes = [vp, vp]
    L.fm_kernel_time_spread.argtypes = [vp, vp, i32]
    L.fm_kernel_time_busy.argtypes = [vp, vp, i32]
    L.fm_kernel_time_stats.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.fm_reset_kernel_times.argtypes = [vp]
    L.fm_rasterize_masks.argtypes = [i32, i32, C.c_double, vp, vp, i32, vp]
    L.fm_max_inflight.argtypes = [vp]
    L.fm_plan.argtypes = [C.POINTER(FMParams), C.POINTER(FMPlan)]
    L.fm_resize_kind.argtypes = [C.POINTER(FMParams), C.POINTER(i32)]
    L.fm_area_up_taps.argtypes = [i32, i32, vp, vp, vp, vp]
    L.fm_gaussian_taps.argtypes = [i32, vp]
    L.fm_haar_set_roi_upscale.argtypes = [vp, i32]
    L.fm_yolo_set_roi_upscale.argtypes = [vp, i32]
    L.fm_last_fallbacks.argtypes = [vp]
    L.fm_last_ccl_stats.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.fm_get_contour_points.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fm_last_trace_stats.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.fm_footprint.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.fm_haar_create.argtypes = [i32, C.POINTER(FMHaarDesc), C.POINTER(vp)]
    L.fm_haar_destroy.argtypes = [vp]
    L.fm_haar_destroy.restype = None
    L.fm_haar_last_error.argtypes = [vp]
    L.fm_haar_last_error.restype = C.c_char_p
    L.fm_haar_window.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.fm_haar_detect.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_double, i32, i32, i32, i32, i32, vp, i32, vp]
    L.fm_haar_candidates.argtypes = [vp, vp, i32]
    L.fm_haar_detect_frames.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_double, i32, vp, i32, vp, vp]
    L.fm_haar_detect_frame_list.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, i32, vp, i32, vp, vp]
    L.fm_haar_detect_frame_list_async.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, i32, vp]
    L.fm_haar_collect.argtypes = [vp, vp, i32, vp, i32]
    L.fm_haar_last_ms.argtypes = [vp]
    L.fm_haar_last_ms.restype = C.c_double
    L.fm_haar_last_sweep.argtypes = [vp]
    L.fm_haar_bank_create.argtypes = [i32, C.POINTER(FMHaarDesc), i32, C.POINTER(vp)]
    L.fm_haar_bank_destroy.argtypes = [vp]
    L.fm_haar_bank_destroy.restype = None
    L.fm_haar_bank_last_error.argtypes = [vp]
    L.fm_haar_bank_last_error.restype = C.c_char_p
    L.fm_haar_bank_size.argtypes = [vp]
    L.fm_haar_bank_detect.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_double, i32, vp, i32, vp]
    L.fm_haar_bank_set_roi_upscale.argtypes = [vp, i32]
    L.fm_haar_bank_detect_frames.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_double, i32, vp, i32, vp, vp]
    L.fm_haar_bank_detect_frame_list.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, i32, vp, i32, vp, vp]
    L.fm_haar_bank_detect_frame_list_async.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, i32, vp]
    L.fm_haar_bank_collect.argtypes = [vp, vp, i32, vp, i32]
    L.fm_haar_bank_candidates.argtypes = [vp, i32, vp, i32]
    L.fm_haar_bank_last_ms.argtypes = [vp]
    L.fm_haar_bank_last_ms.restype = C.c_double
    L.fm_mjpeg_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.fm_mjpeg_destroy.argtypes = [vp]
    L.fm_mjpeg_destroy.restype = None
    L.fm_mjpeg_last_error.argtypes = [vp]
    L.fm_mjpeg_last_error.restype = C.c_char_p
    L.fm_mjpeg_decode.argtypes = [vp, vp, vp, i32, vp, i32]
    L.fm_mjpeg_last_ms.argtypes = [vp]
    L.fm_mjpeg_last_ms.restype = C.c_double
    L.fm_submit_jpeg.argtypes = [vp, vp, vp, vp, i32]
    L.fm_read_frame.argtypes = [vp, i32, i32, vp]
    L.fm_frame_device.argtypes = [vp, i32, i32, C.POINTER(C.c_void_p)]
    L.fm_mjpeg_tune.argtypes = [vp, i32, i32]
    L.fm_mjpeg_geometry.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.fm_submit_streams.argtypes = [vp, vp, i32, i32]
    L.fm_yuv_frame_bytes.argtypes = [i32, i32, C.POINTER(FMYuvLayout), C.POINTER(C.c_size_t)]
    L.fm_submit_yuv.argtypes = [vp, vp, i32, C.POINTER(FMYuvLayout), i32]
    L.fm_submit_yuv_list.argtypes = [vp, vp, i32, C.POINTER(FMYuvLayout)]
    L.fm_jpeg_header.argtypes = [i32, i32, i32, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fm_mjpeg_enc_create.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.fm_mjpeg_enc_destroy.argtypes = [vp]
    L.fm_mjpeg_enc_destroy.restype = None
    L.fm_mjpeg_enc_last_error.argtypes = [vp]
    L.fm_mjpeg_enc_last_error.restype = C.c_char_p
    L.fm_mjpeg_encode.argtypes = [vp, vp, i32, i32]
    L.fm_mjpeg_encode_frame_list.argtypes = [vp, vp, i32]
    L.fm_mjpeg_enc_get.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fm_mjpeg_enc_coefficients.argtypes = [vp, i32, vp, C.c_size_t]
    L.fm_mjpeg_enc_last_ms.argtypes = [vp]
    L.fm_mjpeg_enc_last_ms.restype = C.c_double
    L.fm_yolo_create.argtypes = [i32, C.POINTER(FMYoloDesc), C.POINTER(vp)]
    L.fm_yolo_create_precision.argtypes = [i32, C.POINTER(FMYoloDesc), i32, C.POINTER(vp)]
    L.fm_yolo_precision.argtypes = [vp]
    L.fm_yolo_destroy.argtypes = [vp]
    L.fm_yolo_destroy.restype = None
    L.fm_yolo_last_error.argtypes = [vp]
    L.fm_yolo_last_error.restype = C.c_char_p
    L.fm_yolo_layer_shape.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.fm_yolo_detect_frames.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_float, vp, i32, vp, vp]
    L.fm_yolo_detect_frame_list.argtypes = [vp, vp, i32, i32, i32, i32, C.c_float, vp, i32, vp, vp]
    L.fm_yolo_forward.argtypes = [vp, vp, i32]
    L.fm_yolo_decode.argtypes = [vp, i32, C.c_float, vp, i32, vp]
    L.fm_yolo_layer_output.argtypes = [vp, i32, vp, C.c_size_t]
    L.fm_yolo_route_in_place.argtypes = [vp, i32]
    L.fm_yolo_last_ms.argtypes = [vp, vp]
    L.fm_yolo_last_ms.restype = C.c_double
    L.fm_retain_reserve.argtypes = [vp, i32]
    L.fm_retain_frames.argtypes = [vp, vp, i32, vp]
    L.fm_release_frames.argtypes = [vp, vp, i32]
    L.fm_read_retained.argtypes = [vp, vp, vp]
    L.fm_retained_count.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.fm_background_channels.argtypes = [vp, C.POINTER(i32)]
    L.fm_mog2_defaults.argtypes = [C.POINTER(Mog2Params)]
    L.fm_create_mog2.argtypes = [C.POINTER(vp), C.POINTER(FMParams), C.POINTER(Mog2Params)]
    L.fm_mog2_read_model.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(C.c_int64)]
    L.fm_mog2_write_model.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(C.c_int64)]
    L.fm_mog2_background.argtypes = [vp, i32, vp]
    for name in EXPORTED:
        if name not in ("fm_yolo_destroy", "fm_yolo_last_error", "fm_yolo_last_ms", "fm_destroy", "fm_last_error", "fm_abi_version", "fm_haar_destroy", "fm_haar_last_error",
                        "fm_haar_last_ms", "fm_haar_bank_destroy", "fm_haar_bank_last_error", "fm_haar_bank_last_ms", "fm_mjpeg_destroy", "fm_mjpeg_last_error", "fm_mjpeg_last_ms",
                        "fm_mjpeg_enc_destroy", "fm_mjpeg_enc_last_error", "fm_mjpeg_enc_last_ms"):
            getattr(L, name).restype = i32
    _lib = L
    return L


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def rasterize_masks(h: int, w: int, scale: float, polygons) -> np.ndarray:
    """mask_off_areas (fm.py:611-636) rasterised once: keep-mask (1 = keep, 0 = masked)."""
    L = load()
    polys = [list(p) for p in (polygons or [])]
    keep = np.empty((h, w), np.uint8)
    npts = np.array([len(p) for p in polys], np.int32)
    xy = np.array([c for p in polys for pt in p for c in pt], np.int32) if polys else np.zeros(2, np.int32)
    rc = L.fm_rasterize_masks(h, w, float(scale), _ptr(xy), _ptr(npts) if polys else None, len(polys), _ptr(keep))
    if rc != FM_OK:
        raise FMError(rc, "invalid mask polygons (each needs >= 2 points)")
    return keep


def yuv_format(fmt) -> int:
    """FM_YUV_* of a fourcc name ("NV12", "I420" / "IYUV", "YUY2" / "YUYV", "UYVY") or of the value itself."""
    if isinstance(fmt, (bytes, bytearray)):
        fmt = bytes(fmt).decode("ascii", "replace")
    if isinstance(fmt, str):
        try:
            return YUV_FORMATS[fmt.strip().upper()]
        except KeyError:
            raise ValueError(f"unknown YUV format {fmt!r}") from None
    return int(fmt)


def yuv_layout(fmt, pitch: int = 0, chroma_offset: int = 0, frame_stride: int = 0) -> FMYuvLayout:
    return FMYuvLayout(yuv_format(fmt), int(pitch), int(chroma_offset), int(frame_stride))


def yuv_frame_bytes(width: int, height: int, fmt, pitch: int = 0, chroma_offset: int = 0, frame_stride: int = 0) -> int:
    """Bytes one width x height frame occupies in this layout (fm_yuv_frame_bytes: host only); frames of a batch
    lie frame_stride (0: this many) bytes apart.  FMError(FM_EINVAL) for a layout the engine refuses."""
    L = load()
    n = C.c_size_t()
    lay = yuv_layout(fmt, pitch, chroma_offset, frame_stride)
    rc = L.fm_yuv_frame_bytes(int(width), int(height), C.byref(lay), C.byref(n))
    if rc != FM_OK:
        raise FMError(rc, L.fm_last_error(None).decode())
    return int(n.value)


def engine_flags(keep_planes=False, profile=False, contour_area=False, contour_points=False,
                 area_upscale=False, colour_motion=False, mog2=None) -> int:
    """fm_params.flags of MotionEngine's keyword arguments."""
    return ((FM_FLAG_KEEP_PLANES if keep_planes else 0) | (FM_FLAG_CONTOUR_AREA if contour_area else 0) |
            (FM_FLAG_COLOUR_MOTION if colour_motion else 0) | (FM_FLAG_MOG2 if mog2_params(mog2) is not None else 0) |
            (FM_FLAG_CONTOUR_POINTS if contour_points else 0) | (FM_FLAG_AREA_UPSCALE if area_upscale else 0) |
            (FM_FLAG_PROFILE_PIX if profile == "pix" else FM_FLAG_PROFILE if profile else 0))


def plan(*, n_streams: int = 1, src_w: int, src_h: int, box_size: int, ksize: int, threshold: int = 12,
         avg: float = 0.1, max_batch: int = 1, max_contours: int = 4096, keep_planes: bool = False,
         profile: bool | str = False, device: int = 0, contour_area: bool = False,
         contour_points: bool = False, area_upscale: bool = False, colour_motion: bool = False,
         mog2=None) -> dict:
    """What MotionEngine(**params) would set up, asked of the library without touching a device (fm_plan: the
    same validation and selection as fm_create): work_shape (h, w), tiles, max_inflight and pixel_path, one of
    "small", "pix", "fused", "wide", "rgb" (colour_motion), "mog2" (mog2: the flag alone decides the plan, the
    parameters are checked by MotionEngine) and "pixel" (the per-frame path: one batch in flight).  FMError as
    MotionEngine raises it for parameters the engine refuses."""
    L = load()
    p = FMParams(device, n_streams, src_w, src_h, box_size, ksize, int(threshold), float(avg), max_batch,
                 max_contours,
                 engine_flags(keep_planes, profile, contour_area, contour_points, area_upscale, colour_motion, mog2))
    out = FMPlan()
    rc = L.fm_plan(C.byref(p), C.byref(out))
    if rc != FM_OK:
        raise FMError(rc, L.fm_last_error(None).decode())
    return {"work_shape": (out.work_h, out.work_w), "tiles": out.tiles, "max_inflight": out.max_inflight,
            "pixel_path": out.pixel_path.decode()}


def resize_kind(*, n_streams: int = 1, src_w: int, src_h: int, box_size: int, ksize: int, threshold: int = 12,
                avg: float = 0.1, max_batch: int = 1, max_contours: int = 4096, keep_planes: bool = False,
                profile: bool | str = False, device: int = 0, contour_area: bool = False,
                contour_points: bool = False, area_upscale: bool = False, colour_motion: bool = False) -> int:
    """The resize MotionEngine(**params) would put in front of the pixel chain (fm_resize_kind: no device is
    touched): RESIZE_IDENTITY, RESIZE_FAST, RESIZE_GENERAL, or RESIZE_UP for a box wider than the frame, which
    needs area_upscale=True.  FMError as plan() raises it."""
    L = load()
    p = FMParams(device, n_streams, src_w, src_h, box_size, ksize, int(threshold), float(avg), max_batch,
                 max_contours,
                 engine_flags(keep_planes, profile, contour_area, contour_points, area_upscale, colour_motion))
    kind = C.c_int32(-1)
    rc = L.fm_resize_kind(C.byref(p), C.byref(kind))
    if rc != FM_OK:
        raise FMError(rc, L.fm_last_error(None).decode())
    return int(kind.value)


def area_up_taps(ssize: int, dsize: int):
    """The enlarging resize's taps of one axis as the library builds them (fm_area_up_taps: host only):
    int32 arrays s0, s1, a0, a1 of dsize values."""
    L = load()
    out = [np.zeros(max(int(dsize), 1), np.int32) for _ in range(4)]
    rc = L.fm_area_up_taps(int(ssize), int(dsize), *[_ptr(a) for a in out])
    if rc != FM_OK:
        raise FMError(rc, L.fm_last_error(None).decode())
    return tuple(out)


def gaussian_taps(ksize: int) -> np.ndarray:
    """The fixed-point Gaussian taps of an odd ksize in [1, 255] as the library builds them for every pixel path
    (fm_gaussian_taps: host only): int32, ksize values that sum to 256.  FMError(FM_EINVAL) for any other ksize."""
    L = load()
    out = np.zeros(max(int(ksize), 1), np.int32)
    rc = L.fm_gaussian_taps(int(ksize), _ptr(out))
    if rc != FM_OK:
        raise FMError(rc, L.fm_last_error(None).decode())
    return out


@dataclass
class Contour:
    """One external contour of VideoFrame.contours (fm.py:269-276).

    bbox is cv2.boundingRect's (x, y, w, h) (fm.py:792); origin is the border
    start (the component's raster-first pixel); area is cv2.contourArea of the
    CHAIN_APPROX_SIMPLE contour (fm.py:679), None unless the engine traces it; points is
    that contour as cv2.findContours returns it, an (n, 1, 2) int32 array of (x, y) in trace
    order from the start pixel, None unless the engine has contour_points=True.
    np.asarray(contour) is points, so cv2.drawContours / contourArea / boundingRect /
    convexHull / pointPolygonTest take a Contour where the reference had the array."""
    x: int
    y: int
    w: int
    h: int
    origin: tuple
    area: float | None = None
    points: np.ndarray | None = None

    def __array__(self, dtype=None, copy=None):
        if self.points is None:
            raise TypeError("this Contour carries no points: create the engine with contour_points=True")
        a = self.points if dtype is None else self.points.astype(dtype, copy=False)
        return a.copy() if copy else a

    @property
    def bbox(self):
        return (self.x, self.y, self.w, self.h)


class MotionEngine:
    """One fm_ctx: n_streams background models on one HIP device."""

    def __init__(self, *, n_streams: int, src_w: int, src_h: int, box_size: int, ksize: int,
                 threshold: int, avg: float, max_batch: int = 1, max_contours: int = 4096,
                 keep_planes: bool = False, profile: bool | str = False, device: int = 0,
                 contour_area: bool = False, contour_points: bool = False, area_upscale: bool = False,
                 colour_motion: bool = False, mog2=None):
        # mog2: None, True (OpenCV's defaults), a dict of overrides or a Mog2Params: the Gaussian-mixture background
        # model in place of the running average (FM_FLAG_MOG2); threshold and avg are then unused, there is no
        # background() but mog2_background() / mog2_model(), and no planes
        # area_upscale: a box wider than the frame enlarges it, as imutils.resize does (else FM_ENOTSUP)
        # colour_motion: the chain per colour channel (FM_FLAG_COLOUR_MOTION): the background is (h, w, 3), a pixel
        # is set where any channel's delta exceeds the threshold; no planes (keep_planes with it: FM_ENOTSUP)
        # profile: True = every kernel timed with HIP events, "pix" = pixel-stream kernels only
        self._L = load()
        p = FMParams(device, n_streams, src_w, src_h, box_size, ksize, int(threshold), float(avg),
                     max_batch, max_contours,
                     engine_flags(keep_planes, profile, contour_area, contour_points, area_upscale, colour_motion, mog2))
        h = C.c_void_p()
        self.mog2 = mog2_params(mog2)  # the parameters in force, or None
        if self.mog2 is not None:
            rc = self._L.fm_create_mog2(C.byref(h), C.byref(p), C.byref(self.mog2))
        else:
            rc = self._L.fm_create(C.byref(h), C.byref(p))
        if rc != FM_OK:
            raise FMError(rc, self._L.fm_last_error(None).decode())
        self._h = h
        self.params = p
        hh, ww = C.c_int(), C.c_int()
        self._check(self._L.fm_work_size(h, C.byref(hh), C.byref(ww)))
        self.work_shape = (hh.value, ww.value)
        ch = C.c_int(1)
        if self.mog2 is None:
            self._check(self._L.fm_background_channels(h, C.byref(ch)))
        self.colour_motion = ch.value == 3
        self.background_shape = self.work_shape + ((3,) if self.colour_motion else ())
        self.max_inflight = self._L.fm_max_inflight(h)
        pl = FMPlan()   # the selection fm_create just made (the same function): which kernels run the pixel chain
        self._check(self._L.fm_plan(C.byref(p), C.byref(pl)))
        self.pixel_path = pl.pixel_path.decode()
        self.tiles = pl.tiles
        kind = C.c_int32(-1)
        self._check(self._L.fm_resize_kind(C.byref(p), C.byref(kind)))
        self.resize_kind = int(kind.value)  # RESIZE_*
        self.n_streams = n_streams
        self.src_shape = (src_h, src_w, 3)
        self.device = int(device)
        self.max_batch = max_batch
        self.max_contours = max_contours
        self.last_batch = 0
        self.keep_planes = bool(keep_planes)
        self.contour_points = bool(contour_points)
        self.generation = 0    # bumped at every wait(): results of older batches are gone
        self._init = [False] * n_streams
        self._inflight = []    # (n_frames, host frames kept alive) per submitted, not yet waited batch

    # -- plumbing ------------------------------------------------------------
    def _check(self, rc: int) -> int:
        if rc < 0:
            raise FMError(rc, self._L.fm_last_error(self._h).decode())
        return rc

    def close(self) -> None:
        if getattr(self, "_h", None):
            for buf in getattr(self, "_host_bufs", []):
                self._L.fm_host_free(self._h, buf)
            self._host_bufs = []
            self._L.fm_destroy(self._h)
            self._h = None

    def host_buffer(self, n_frames: int) -> np.ndarray:
        """Page-locked uint8 [n_frames][n_streams][H][W][3] array for frame batches: submit()
        of it is an asynchronous DMA on the engine's input stream, overlapped with the
        previous batches' kernels.  Freed by close(); keep it unchanged until wait() returns
        for a batch submitted from it."""
        shape = (n_frames, self.n_streams) + self.src_shape
        nbytes = int(np.prod(shape))
        p = C.c_void_p()
        self._check(self._L.fm_host_alloc(self._h, nbytes, C.byref(p)))
        if not hasattr(self, "_host_bufs"):
            self._host_bufs = []
        self._host_bufs.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,)).reshape(shape)

    def host_buffer_yuv(self, n_frames: int, fmt, pitch: int = 0, chroma_offset: int = 0,
                        frame_stride: int = 0) -> np.ndarray:
        """host_buffer for YUV batches: page-locked uint8 [n_frames][n_streams][stride], stride = frame_stride or
        the frame's bytes in this layout (yuv_frame_bytes); submit_yuv of it is an asynchronous DMA."""
        H, W = self.src_shape[:2]
        stride = int(frame_stride) or yuv_frame_bytes(W, H, fmt, pitch, chroma_offset)
        shape = (int(n_frames), self.n_streams, stride)
        nbytes = int(np.prod(shape))
        p = C.c_void_p()
        self._check(self._L.fm_host_alloc(self._h, nbytes, C.byref(p)))
        if not hasattr(self, "_host_bufs"):
            self._host_bufs = []
        self._host_bufs.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,)).reshape(shape)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state ---------------------------------------------------------------
    def set_mask(self, stream: int, keep: np.ndarray | None) -> None:
        if keep is None:
            self._check(self._L.fm_set_mask(self._h, stream, None))
            return
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.shape != self.work_shape:
            raise ValueError(f"keep-mask shape {keep.shape} != work shape {self.work_shape}")
        self._check(self._L.fm_set_mask(self._h, stream, _ptr(keep)))

    def reset(self, stream: int) -> None:
        self._check(self._L.fm_reset_stream(self._h, stream))
        self._init[stream] = False

    def initialized(self, stream: int) -> bool:
        """True once the stream's background exists (after its first frame, fm.py:651-652)."""
        return self._init[stream]

    def mog2_model(self, stream: int) -> dict:
        """The stream's Gaussian-mixture model: weight, mean, var float32 (5, h, w), nmodes uint8 (h, w), nframes.
        Entries at mode >= nmodes are 0."""
        h, w = self.work_shape
        wt, mean, var = (np.zeros((5, h, w), np.float32) for _ in range(3))
        nm = np.zeros((h, w), np.uint8)
        nf = C.c_int64()
        self._check(self._L.fm_mog2_read_model(self._h, stream, _ptr(wt), _ptr(mean), _ptr(var), _ptr(nm), C.byref(nf)))
        return {"weight": wt, "mean": mean, "var": var, "nmodes": nm, "nframes": int(nf.value)}

    def set_mog2_model(self, stream: int, weight, mean, var, nmodes, nframes: int) -> None:
        h, w = self.work_shape
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (weight, mean, var)]
        nm = np.ascontiguousarray(nmodes, dtype=np.uint8)
        if any(a.shape != (5, h, w) for a in arrs) or nm.shape != (h, w):
            raise ValueError(f"model arrays must be (5, {h}, {w}) and nmodes ({h}, {w})")
        nf = C.c_int64(int(nframes))
        self._check(self._L.fm_mog2_write_model(self._h, stream, *[_ptr(a) for a in arrs], _ptr(nm), C.byref(nf)))
        self._init[stream] = True

    def mog2_background(self, stream: int) -> np.ndarray:
        """cv2's getBackgroundImage of the stream's model: uint8 (h, w), 0 where a pixel has no mode yet."""
        out = np.zeros(self.work_shape, np.uint8)
        self._check(self._L.fm_mog2_background(self._h, stream, _ptr(out)))
        return out

    def background(self, stream: int) -> np.ndarray:
        if self.mog2 is not None:
            raise FMError(FM_ESTATE, "a mog2 engine has no running average: use mog2_background() or mog2_model()")
        out = np.empty(self.background_shape, np.float64)
        self._check(self._L.fm_read_background(self._h, stream, _ptr(out)))
        return out

    def set_background(self, stream: int, bg: np.ndarray) -> None:
        bg = np.ascontiguousarray(bg, dtype=np.float64)
        if bg.shape != self.background_shape:
            raise ValueError(f"background shape {bg.shape} != {self.background_shape}")
        self._check(self._L.fm_write_background(self._h, stream, _ptr(bg)))
        self._init[stream] = True

    def set_hip_stream(self, stream_handle: int | None) -> None:
        self._check(self._L.fm_set_hip_stream(self._h, stream_handle))

    # -- hot path ------------------------------------------------------------
    def submit(self, frames: np.ndarray) -> None:
        """frames: uint8 [n][n_streams][H][W][3] (or [n_streams][H][W][3] for n = 1), host memory."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.ndim == 4:
            f = f[None]
        if f.shape[1:] != (self.n_streams,) + self.src_shape:
            raise ValueError(f"frames shape {f.shape} != [n][{self.n_streams}]{self.src_shape}")
        self._check(self._L.fm_submit(self._h, _ptr(f), f.shape[0], 0))
        self._inflight.append((f.shape[0], f))

    def submit_streams(self, frames, on_device: bool = False, n_frames: int | None = None) -> None:
        """One buffer per stream (fm_submit_streams): frames[s] = stream s's frames [n][H][W][3] -- host
        arrays, or device addresses (ints) with on_device and n_frames.  Same results as submit() of the
        frames gathered into [n][n_streams] order, without the host-side gather."""
        if len(frames) != self.n_streams:
            raise ValueError(f"{len(frames)} stream buffers for {self.n_streams} streams")
        if on_device:
            if n_frames is None:
                raise ValueError("n_frames is required for device buffers")
            ptrs = np.array([int(p) for p in frames], np.uint64)
            self._check(self._L.fm_submit_streams(self._h, _ptr(ptrs), int(n_frames), 1))
            self._inflight.append((int(n_frames), None))
            return
        arrs = []
        for f in frames:
            a = np.asarray(f)
            if a.dtype != np.uint8 or not a.flags.c_contiguous:
                a = np.ascontiguousarray(a, dtype=np.uint8)
            if a.ndim == 3:
                a = a[None]
            if a.shape[1:] != self.src_shape:
                raise ValueError(f"stream buffer shape {a.shape} != [n]{self.src_shape}")
            if arrs and a.shape[0] != arrs[0].shape[0]:
                raise ValueError("every stream buffer must hold the same number of frames")
            arrs.append(a)
        ptrs = np.array([a.ctypes.data for a in arrs], np.uint64)
        self._check(self._L.fm_submit_streams(self._h, _ptr(ptrs), arrs[0].shape[0], 0))
        self._inflight.append((arrs[0].shape[0], arrs))

    def submit_device(self, ptr: int, n_frames: int) -> None:
        """Frames already in device memory (e.g. a torch CUDA tensor's data_ptr()).

        Up to two batches may be in flight (submit batch i+1 before wait() for
        batch i): the contour pass of one overlaps the pixel kernel of the next."""
        self._check(self._L.fm_submit(self._h, C.c_void_p(ptr), n_frames, 1))
        self._inflight.append((n_frames, None))

    def submit_jpeg(self, decoder: "MJpegDecoder", jpegs) -> None:
        """Compressed frames (the decode side, fm.py:497-506): jpegs = n_frames x n_streams JPEG byte
        strings in [t][s] order (a flat sequence), decoded on the GPU into the batch, then processed
        as submit().  The byte strings may be dropped once this returns."""
        n = len(jpegs)
        if n % self.n_streams:
            raise ValueError(f"{n} JPEGs is not a multiple of n_streams={self.n_streams}")
        ptrs, sizes, keep = _jpeg_arrays(jpegs)
        self._check(self._L.fm_submit_jpeg(self._h, decoder._h, _ptr(ptrs), _ptr(sizes), n // self.n_streams))
        del keep
        self._inflight.append((n // self.n_streams, None))

    def submit_yuv(self, frames, fmt, pitch: int = 0, chroma_offset: int = 0, frame_stride: int = 0,
                   n_frames: int | None = None) -> None:
        """YUV frames in host memory (fm_submit_yuv): a uint8 array holding n x n_streams frames in [t][s] order,
        frame_stride (0: the frame's bytes) apart, converted to BGR on the GPU in front of the hot path
        (cv2.cvtColor COLOR_YUV2BGR_*).  fmt: "NV12", "I420", "YUY2", "UYVY" (or FM_YUV_*).  n_frames: taken
        from the array when not given (its first axis, or its size for a flat one).  Keep the array unchanged
        until wait() returns for the batch; read_frame() gives the converted BGR frame."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        H, W = self.src_shape[:2]
        extent = yuv_frame_bytes(W, H, fmt, pitch, chroma_offset, frame_stride)
        stride = int(frame_stride) or extent
        if n_frames is None:
            n_frames = f.shape[0] if f.ndim >= 3 else (f.size + stride - extent) // (stride * self.n_streams)
        n = int(n_frames)
        if n >= 1 and f.size < (n * self.n_streams - 1) * stride + extent:
            raise ValueError(f"{f.size} bytes for {n} x {self.n_streams} frames of {extent} bytes, {stride} apart")
        lay = yuv_layout(fmt, pitch, chroma_offset, frame_stride)
        self._check(self._L.fm_submit_yuv(self._h, _ptr(f), n, C.byref(lay), 0))
        self._inflight.append((n, f))

    def submit_yuv_device(self, ptr: int, n_frames: int, fmt, pitch: int = 0, chroma_offset: int = 0,
                          frame_stride: int = 0) -> None:
        """YUV frames already in device memory at ptr, [n_frames][n_streams] frames frame_stride apart, read in
        place (keep them until wait() returns for the batch)."""
        lay = yuv_layout(fmt, pitch, chroma_offset, frame_stride)
        self._check(self._L.fm_submit_yuv(self._h, C.c_void_p(int(ptr)), int(n_frames), C.byref(lay), 1))
        self._inflight.append((int(n_frames), None))

    def submit_yuv_list(self, ptrs, fmt, pitch: int = 0, chroma_offset: int = 0) -> None:
        """n x n_streams YUV frames in device memory at separate addresses, ptrs[t * n_streams + s] (a decoder's
        surfaces: fm_submit_yuv_list), converted where they lie."""
        ptrs = [int(p) for p in ptrs]
        if not ptrs or len(ptrs) % self.n_streams:
            raise ValueError(f"{len(ptrs)} frame addresses is not a multiple of n_streams={self.n_streams}")
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        lay = yuv_layout(fmt, pitch, chroma_offset, 0)
        n = len(ptrs) // self.n_streams
        self._check(self._L.fm_submit_yuv_list(self._h, C.cast(arr, C.c_void_p), n, C.byref(lay)))
        self._inflight.append((n, None))

    def wait(self) -> None:
        """Complete the oldest batch in flight; its results become readable."""
        self._check(self._L.fm_wait(self._h))
        if self._inflight:
            self.last_batch = self._inflight.pop(0)[0]
        self.generation += 1
        self._init = [True] * self.n_streams

    def fallbacks(self) -> int:
        """Frames of the last waited batch relabelled by the pixel-level fallback (diagnostics)."""
        return self._check(self._L.fm_last_fallbacks(self._h))

    def ccl_stats(self) -> dict:
        """Contour pass of the last waited batch: nodes taken from the shared pool, heavy tiles."""
        a, b = C.c_int32(), C.c_int32()
        self._check(self._L.fm_last_ccl_stats(self._h, C.byref(a), C.byref(b)))
        return {"shared_nodes": a.value, "heavy_tiles": b.value}

    def footprint(self) -> dict:
        """Bytes the context holds: device memory and page-locked host memory (fm_footprint)."""
        d, p = C.c_size_t(), C.c_size_t()
        self._check(self._L.fm_footprint(self._h, C.byref(d), C.byref(p)))
        return {"device_bytes": d.value, "pinned_bytes": p.value}

    def counts(self) -> np.ndarray:
        out = np.zeros((self.last_batch, self.n_streams), np.int32)
        self._check(self._L.fm_get_counts(self._h, _ptr(out)))
        return out

    def contours(self, frame: int, stream: int) -> list:
        """Every external contour of (frame, stream), in raster order of their start pixels.

        max_contours only sizes the first fetch: a frame with more contours is fetched
        whole, so len() is always the true count find_movement needs (fm.py:674-694)."""
        cap = self.max_contours
        while True:
            buf = (FMContour * cap)()
            n = self._check(self._L.fm_get_contours(self._h, frame, stream, C.cast(buf, C.c_void_p), cap))
            if n <= cap:
                out = [Contour(c.x, c.y, c.w, c.h, (c.origin_x, c.origin_y), c.area2 / 2 if c.area2 >= 0 else None)
                       for c in buf[:n]]
                if self.contour_points:
                    xy = self.contour_points_xy(frame, stream)
                    ends = np.cumsum([c.npts for c in buf[:n]])
                    if n and int(ends[-1]) != len(xy):
                        raise FMError(FM_ESTATE, f"{len(xy)} points for records that count {int(ends[-1])}")
                    for c, e, k in zip(out, ends, [c.npts for c in buf[:n]]):
                        c.points = xy[e - k:e].reshape(k, 1, 2)
                return out
            cap = n

    def contour_points_xy(self, frame: int, stream: int) -> np.ndarray:
        """Every contour point of (frame, stream) as one (total, 2) int32 array of (x, y), the contours
        back to back in contours() order (fm_get_contour_points: one host copy)."""
        total = C.c_size_t(0)
        rc = self._L.fm_get_contour_points(self._h, frame, stream, None, 0, C.byref(total))
        if rc != FM_OK and not (rc == FM_EINVAL and total.value > 0):
            self._check(rc)
        xy = np.empty((total.value, 2), np.int32)
        if total.value:
            self._check(self._L.fm_get_contour_points(self._h, frame, stream, _ptr(xy), total.value, C.byref(total)))
        return xy

    def trace_stats(self) -> dict:
        """Contour trace of the last waited batch (contour_points=True): contours walked on a staged
        window (registers or LDS), contours walked unstaged (larger boxes: global memory behind a
        sliding window), border steps walked."""
        a, b, st = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._L.fm_last_trace_stats(self._h, C.byref(a), C.byref(b), C.byref(st)))
        return {"staged": a.value, "unstaged": b.value, "steps": st.value}

    def mask(self, frame: int, stream: int) -> np.ndarray:
        out = np.empty(self.work_shape, np.uint8)
        self._check(self._L.fm_read_mask(self._h, frame, stream, _ptr(out)))
        return out

    def threshold_bits(self, frame: int, stream: int) -> np.ndarray:
        """Diagnostics: the undilated threshold bits as the tile pixel paths store them, uint64 [ntiles][64]:
        tile (raster order), column word c, bit r = pixel (row r, column c) of the 64 x 64 tile."""
        h, w = self.work_shape
        out = np.empty((((h + 63) // 64) * ((w + 63) // 64), 64), np.uint64)
        self._check(self._L.fm_read_threshold_bits(self._h, frame, stream, _ptr(out)))
        return out

    def read_frame(self, frame: int, stream: int) -> np.ndarray:
        """The source frame (BGR) of (frame, stream) of the last waited batch, from the device."""
        out = np.empty(self.src_shape, np.uint8)
        self._check(self._L.fm_read_frame(self._h, frame, stream, _ptr(out)))
        return out

    def frame_device_ptr(self, frame: int, stream: int) -> int:
        """Device address of the source frame (BGR [H][W][3]) of (frame, stream) of the last waited
        batch, left in HBM (valid until the next wait)."""
        p = C.c_void_p()
        self._check(self._L.fm_frame_device(self._h, frame, stream, C.byref(p)))
        return int(p.value)

    # -- retained source frames (fm_retain_*): frames kept in HBM after their batch slot is reused ----------
    def reserve_retained(self, n: int) -> None:
        """Size the pool of retained frames to n entries of one source frame each (0 frees it)."""
        self._check(self._L.fm_retain_reserve(self._h, int(n)))

    def retain(self, pairs) -> list:
        """Copy the (frame, stream) source frames of the last waited batch into free pool entries, all in one
        kernel launch, complete on return; their device addresses, in the order of `pairs`."""
        fs = np.ascontiguousarray([tuple(p) for p in pairs], dtype=np.int32).reshape(-1, 2)
        n = fs.shape[0]
        out = (C.c_void_p * max(n, 1))()
        self._check(self._L.fm_retain_frames(self._h, _ptr(fs), n, C.cast(out, C.c_void_p)))
        return [int(out[i]) for i in range(n)]

    def release(self, ptrs) -> None:
        """Free retained frames (all of them, or, if one is not a retained frame, none: FM_EINVAL)."""
        ptrs = [int(p) for p in ptrs]
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        self._check(self._L.fm_release_frames(self._h, C.cast(arr, C.c_void_p), len(ptrs)))

    def read_retained(self, ptr: int) -> np.ndarray:
        """A retained frame (BGR [H, W, 3]) copied to the host."""
        out = np.empty(self.src_shape, np.uint8)
        self._check(self._L.fm_read_retained(self._h, C.c_void_p(int(ptr)), _ptr(out)))
        return out

    @property
    def retained(self) -> tuple:
        """(entries in use, the pool's size)."""
        a, b = C.c_int(), C.c_int()
        self._check(self._L.fm_retained_count(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def plane(self, which: int, frame: int, stream: int) -> np.ndarray:
        """gray / blur / frame_delta (h, w), or PLANE_SMALL: the resized BGR frame (h, w, 3) (fm.py:490)."""
        out = np.empty(self.work_shape + ((3,) if which == PLANE_SMALL else ()), np.uint8)
        self._check(self._L.fm_read_plane(self._h, which, frame, stream, _ptr(out)))
        return out

    def kernel_time_stats(self) -> dict:
        """{kernel: {ms, launches, stamped, ms_sq, busy_ms}} plus {"_unstamped": n}, from ONE fold of the launch
        stamps (fm_kernel_time_stats), so every figure covers the same launches."""
        N = 32
        names = (C.c_char_p * N)()
        ms, sms, sq, busy = (C.c_double * N)(), (C.c_double * N)(), (C.c_double * N)(), (C.c_double * N)()
        nl, ns = (C.c_int64 * N)(), (C.c_int64 * N)()
        un = C.c_int64(0)
        v = [C.cast(x, C.c_void_p) for x in (names, ms, nl, sms, ns, sq, busy)]
        n = self._check(self._L.fm_kernel_time_stats(self._h, *v, C.byref(un), N))
        out = {names[i].decode(): {"ms": ms[i], "launches": nl[i], "stamped_ms": sms[i], "stamped": ns[i],
                                   "ms_sq": sq[i], "busy_ms": busy[i]} for i in range(min(n, N))}
        out["_unstamped"] = int(un.value)
        return out

    def kernel_times(self) -> dict:
        """{kernel: (ms, launches)} since the last reset."""
        return {k: (v["ms"], v["launches"]) for k, v in self.kernel_time_stats().items() if k != "_unstamped"}

    def kernel_time_busy(self) -> dict:
        """{kernel: ms during which at least one of its stamped launches ran}."""
        return {k: v["busy_ms"] for k, v in self.kernel_time_stats().items() if k != "_unstamped"}

    def kernel_time_std(self) -> dict:
        """{kernel: standard deviation of its launch time in ms} over its stamped launches only (the pixel kernel
        and the resize; event-timed launches add to ms but not to ms_sq, so they are left out of both)."""
        out = {}
        for name, v in self.kernel_time_stats().items():
            if name == "_unstamped" or v["stamped"] < 1 or v["ms_sq"] <= 0:
                continue
            cnt = v["stamped"]
            out[name] = max(v["ms_sq"] / cnt - (v["stamped_ms"] / cnt) ** 2, 0.0) ** 0.5
        return out

    def reset_kernel_times(self) -> None:
        self._check(self._L.fm_reset_kernel_times(self._h))


class CascadeClassifier:
    """cv2.CascadeClassifier for HAAR cascades on the GPU (find_motion.py:396, :722-731).

    `CascadeClassifier(path)` reads the XML (find_motion_amd.cascade); `detectMultiScale`
    keeps OpenCV's signature and returns an (N, 4) int32 array of (x, y, w, h), or an
    empty tuple when nothing is found, as cv2 does.  `detect_batch` runs many images of
    one size in one call (the ROI frames of many streams)."""

    def __init__(self, path_or_cascade, device: int = 0, roi_upscale: bool = False):
        # roi_upscale: detect_frames enlarges frames narrower than roi_w, as imutils.resize does (else FM_ENOTSUP)
        from .cascade import Cascade, parse
        cs = path_or_cascade if isinstance(path_or_cascade, Cascade) else parse(path_or_cascade)
        self.cascade = cs
        L = load()
        self._keep = [np.ascontiguousarray(a) for a in (
            cs.stage_ntrees, cs.stage_threshold, cs.tree_nodes, cs.node_left, cs.node_right, cs.node_feature,
            cs.node_threshold, cs.leaves, cs.feat_rects, cs.feat_weights, cs.feat_tilted)]
        k = self._keep
        d = FMHaarDesc(cs.win_w, cs.win_h, len(cs.stage_ntrees), len(cs.tree_nodes), len(cs.node_left),
                       len(cs.leaves), len(cs.feat_tilted), *[_ptr(a) for a in k])
        h = C.c_void_p()
        rc = L.fm_haar_create(int(device), C.byref(d), C.byref(h))
        self._h = h
        if rc != FM_OK:
            msg = L.fm_haar_last_error(h).decode() if h else ""
            L.fm_haar_destroy(h)
            self._h = None
            raise FMError(rc, f"fm_haar_create: {msg}")
        if roi_upscale:
            self.set_roi_upscale(True)

    def set_roi_upscale(self, on: bool) -> None:
        load().fm_haar_set_roi_upscale(self._h, int(bool(on)))

    def empty(self) -> bool:
        return self._h is None

    def detect_batch(self, images: np.ndarray, scaleFactor=1.1, minNeighbors=5, minSize=(0, 0), maxSize=(0, 0),
                     cap: int = 256):
        """images: [n, H, W, 3] BGR or [n, H, W] gray u8 -> list of (k, 4) int32 arrays."""
        L = load()
        imgs = np.ascontiguousarray(images, np.uint8)
        ch = 3 if imgs.ndim == 4 else 1
        n, H, W = imgs.shape[:3]
        while True:
            rects = np.zeros((n, cap, 4), np.int32)
            counts = np.zeros(n, np.int32)
            rc = L.fm_haar_detect(self._h, _ptr(imgs), n, H, W, ch, 0, float(scaleFactor), int(minNeighbors),
                                  int(minSize[0]), int(minSize[1]), int(maxSize[0]), int(maxSize[1]),
                                  _ptr(rects), cap, _ptr(counts))
            if rc != FM_OK:
                raise FMError(rc, f"fm_haar_detect: {L.fm_haar_last_error(self._h).decode()}")
            if counts.max(initial=0) <= cap:
                return [rects[i, :counts[i]].copy() for i in range(n)]
            cap = int(counts.max())

    def detect_frames(self, frames: np.ndarray, roi_w: int = 300, scaleFactor=1.1, minNeighbors=5, cap: int = 256):
        """find_objects on raw BGR frames [n, H, W, 3]: INTER_AREA to width roi_w on the device, then
        detectMultiScale; rects are in ROI coordinates (as find_motion.py:724-729 stores them).
        `frames` is a host array, a contiguous uint8 torch tensor already on the detector's GPU
        (frames resident in HBM: no host round trip; torch's current stream is synchronised first),
        or a tuple (device address, n, H, W) of frames the engine left in HBM (fm_frame_device)."""
        L = load()
        if isinstance(frames, tuple):  # (device address, n, H, W): frames left in HBM by the engine
            ptr, n, H, W = frames
            return self._detect_frames(L, C.c_void_p(ptr), int(n), int(H), int(W), 1, roi_w, scaleFactor,
                                       minNeighbors, cap)
        if getattr(frames, "is_cuda", False):
            import torch
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
                raise ValueError("device frames must be a contiguous uint8 tensor [n, H, W, 3]")
            torch.cuda.current_stream(frames.device).synchronize()
            fr, ptr, on_dev = frames, C.c_void_p(frames.data_ptr()), 1
        else:
            fr = np.ascontiguousarray(frames, np.uint8)
            ptr, on_dev = _ptr(fr), 0
        n, H, W = (int(v) for v in fr.shape[:3])
        return self._detect_frames(L, ptr, n, H, W, on_dev, roi_w, scaleFactor, minNeighbors, cap)

    def detect_frame_list(self, ptrs, H: int, W: int, roi_w: int = 300, scaleFactor=1.1, minNeighbors=5,
                          cap: int = 256):
        """find_objects on raw BGR frames already in device memory at separate addresses (e.g. the ROI frames
        of many streams left in an engine's ring or input slots): `ptrs` = their device addresses, each
        frame [H, W, 3].  The resize reads them in place (fm_haar_detect_frame_list); rects in ROI
        coordinates.  The frames must be complete on the device (the caller synchronises its streams)."""
        L = load()
        n = len(ptrs)
        arr = (C.c_void_p * n)(*[int(p) for p in ptrs])
        rh = C.c_int32()
        while True:
            rects = np.zeros((n, cap, 4), np.int32)
            counts = np.zeros(n, np.int32)
            rc = L.fm_haar_detect_frame_list(self._h, C.cast(arr, C.c_void_p), n, int(H), int(W), int(roi_w),
                                             float(scaleFactor), int(minNeighbors), _ptr(rects), cap, _ptr(counts),
                                             C.byref(rh))
            if rc != FM_OK:
                raise FMError(rc, f"fm_haar_detect_frame_list: {L.fm_haar_last_error(self._h).decode()}")
            if counts.max(initial=0) <= cap:
                return [rects[i, :counts[i]].copy() for i in range(n)]
            cap = int(counts.max())

    def detect_frame_list_async(self, ptrs, H: int, W: int, roi_w: int = 300, scaleFactor=1.1, minNeighbors=5) -> int:
        """detect_frame_list queued on the detector's own stream without waiting (fm_haar_detect_frame_list_async);
        `collect` returns its results.  One detection in flight per detector; the frames must stay in place
        until it is collected.  Returns the number of frames queued."""
        L = load()
        n = len(ptrs)
        arr = (C.c_void_p * n)(*[int(p) for p in ptrs])
        rh = C.c_int32()
        rc = L.fm_haar_detect_frame_list_async(self._h, C.cast(arr, C.c_void_p), n, int(H), int(W), int(roi_w),
                                               float(scaleFactor), int(minNeighbors), C.byref(rh))
        if rc != FM_OK:
            raise FMError(rc, f"fm_haar_detect_frame_list_async: {L.fm_haar_last_error(self._h).decode()}")
        return n

    def collect(self, n: int, cap: int = 256):
        """The queued detection's results (waits for it): a list of [k, 4] rect arrays, one per frame."""
        L = load()
        while True:
            rects = np.zeros((n, cap, 4), np.int32)
            counts = np.zeros(n, np.int32)
            rc = L.fm_haar_collect(self._h, _ptr(rects), cap, _ptr(counts), int(n))
            if rc != FM_OK:
                raise FMError(rc, f"fm_haar_collect: {L.fm_haar_last_error(self._h).decode()}")
            if counts.max(initial=0) <= cap:
                return [rects[i, :counts[i]].copy() for i in range(n)]
            cap = int(counts.max())

    def _detect_frames(self, L, ptr, n, H, W, on_dev, roi_w, scaleFactor, minNeighbors, cap):
        rh = C.c_int32()
        while True:
            rects = np.zeros((n, cap, 4), np.int32)
            counts = np.zeros(n, np.int32)
            rc = L.fm_haar_detect_frames(self._h, ptr, n, H, W, on_dev, int(roi_w), float(scaleFactor),
                                         int(minNeighbors), _ptr(rects), cap, _ptr(counts), C.byref(rh))
            if rc != FM_OK:
                raise FMError(rc, f"fm_haar_detect_frames: {L.fm_haar_last_error(self._h).decode()}")
            if counts.max(initial=0) <= cap:
                return [rects[i, :counts[i]].copy() for i in range(n)]
            cap = int(counts.max())

    def detectMultiScale(self, image, scaleFactor=1.1, minNeighbors=5, flags=0, minSize=(0, 0), maxSize=(0, 0)):
        r = self.detect_batch(np.asarray(image)[None], scaleFactor, minNeighbors, minSize or (0, 0),
                              maxSize or (0, 0))[0]
        return r if len(r) else ()

    def candidates(self) -> np.ndarray:
        """Ungrouped candidates of image 0 of the last call (parity tests)."""
        L = load()
        n = L.fm_haar_candidates(self._h, None, 0)
        out = np.zeros((max(n, 1), 4), np.int32)
        L.fm_haar_candidates(self._h, _ptr(out), n)
        return out[:n]

    def last_ms(self) -> float:
        return float(load().fm_haar_last_ms(self._h))

    def last_sweep(self) -> int:
        """The window sweep of the last call (fm_haar_last_sweep): 0 none yet or no window, 1 the tiled
        sweep on LDS patches, 2 the global-memory sweep of cascades whose patches do not fit in LDS."""
        return int(load().fm_haar_last_sweep(self._h))

    def close(self):
        if self._h:
            load().fm_haar_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def haar_desc(cs):
    """A cascade.Cascade as (FMHaarDesc, keep-alive list of its arrays)."""
    keep = [np.ascontiguousarray(a) for a in (
        cs.stage_ntrees, cs.stage_threshold, cs.tree_nodes, cs.node_left, cs.node_right, cs.node_feature,
        cs.node_threshold, cs.leaves, cs.feat_rects, cs.feat_weights, cs.feat_tilted)]
    d = FMHaarDesc(cs.win_w, cs.win_h, len(cs.stage_ntrees), len(cs.tree_nodes), len(cs.node_left),
                   len(cs.leaves), len(cs.feat_tilted), *[_ptr(a) for a in keep])
    return d, keep


class CascadeBank:
    """Several HAAR cascades over the same frames in one GPU pass (fm_haar_bank_*): the frames are uploaded
    and resized once, one pyramid and one set of integral images serve every member, and one launch sweeps
    all their windows.  Each member's results are those of a CascadeClassifier built from the same cascade.

    `CascadeBank(cascades)` takes 1..32 XML paths or cascade.Cascade objects.  The methods mirror
    CascadeClassifier's (default min and max sizes) and return a list per member of lists per image of
    (k, 4) int32 arrays.  A cascade whose window does not fit the tiled sweep is refused (FM_ENOTSUP):
    keep a CascadeClassifier for it."""

    def __init__(self, cascades, device: int = 0, roi_upscale: bool = False):
        from .cascade import Cascade, parse
        self.cascades = [c if isinstance(c, Cascade) else parse(c) for c in cascades]
        self._h = None
        L = load()
        descs, self._keep = (FMHaarDesc * max(len(self.cascades), 1))(), []
        for i, cs in enumerate(self.cascades):
            descs[i], keep = haar_desc(cs)
            self._keep.append(keep)
        h = C.c_void_p()
        rc = L.fm_haar_bank_create(int(device), descs, len(self.cascades), C.byref(h))
        if rc != FM_OK:
            msg = L.fm_haar_bank_last_error(h).decode() if h else ""
            L.fm_haar_bank_destroy(h)
            raise FMError(rc, f"fm_haar_bank_create: {msg}")
        self._h = h
        if roi_upscale:
            self.set_roi_upscale(True)

    def __len__(self) -> int:
        return len(self.cascades)

    def set_roi_upscale(self, on: bool) -> None:
        load().fm_haar_bank_set_roi_upscale(self._h, int(bool(on)))

    def _results(self, what: str, n: int, cap: int, call):
        """call(rects, cap, counts) -> rc, repeated with a larger cap while some count exceeds it."""
        L, M = load(), len(self.cascades)
        while True:
            rects = np.zeros((M, n, cap, 4), np.int32)
            counts = np.zeros((M, n), np.int32)
            rc = call(_ptr(rects), cap, _ptr(counts))
            if rc != FM_OK:
                raise FMError(rc, f"{what}: {L.fm_haar_bank_last_error(self._h).decode()}")
            if counts.max(initial=0) <= cap:
                return [[rects[m, i, :counts[m, i]].copy() for i in range(n)] for m in range(M)]
            cap = int(counts.max())

    def detect_batch(self, images: np.ndarray, scaleFactor=1.1, minNeighbors=5, cap: int = 256):
        """images: [n, H, W, 3] BGR or [n, H, W] gray u8 -> per member, per image, (k, 4) int32 rects."""
        L = load()
        imgs = np.ascontiguousarray(images, np.uint8)
        if imgs.ndim not in (3, 4) or (imgs.ndim == 4 and imgs.shape[3] != 3):
            raise ValueError("images must be [n, H, W, 3] BGR or [n, H, W] gray")
        ch = 3 if imgs.ndim == 4 else 1
        n, H, W = imgs.shape[:3]
        return self._results("fm_haar_bank_detect", n, cap, lambda r, c, k: L.fm_haar_bank_detect(
            self._h, _ptr(imgs), n, H, W, ch, 0, float(scaleFactor), int(minNeighbors), r, c, k))

    def detect_frames(self, frames, roi_w: int = 300, scaleFactor=1.1, minNeighbors=5, cap: int = 256):
        """CascadeClassifier.detect_frames for every member: raw BGR frames [n, H, W, 3] as a host array, a
        contiguous uint8 torch tensor on the bank's GPU, or a tuple (device address, n, H, W); one INTER_AREA
        resize to width roi_w, rects in ROI coordinates."""
        L = load()
        if isinstance(frames, tuple):
            ptr, n, H, W = frames
            fr, ptr, on_dev = None, C.c_void_p(ptr), 1
        elif getattr(frames, "is_cuda", False):
            import torch
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
                raise ValueError("device frames must be a contiguous uint8 tensor [n, H, W, 3]")
            torch.cuda.current_stream(frames.device).synchronize()
            fr, ptr, on_dev = frames, C.c_void_p(frames.data_ptr()), 1
            n, H, W = frames.shape[:3]
        else:
            fr = np.ascontiguousarray(frames, np.uint8)
            if fr.ndim != 4 or fr.shape[3] != 3:
                raise ValueError("frames must be [n, H, W, 3] BGR")
            ptr, on_dev = _ptr(fr), 0
            n, H, W = fr.shape[:3]
        n, H, W = int(n), int(H), int(W)
        rh = C.c_int32()
        return self._results("fm_haar_bank_detect_frames", n, cap, lambda r, c, k: L.fm_haar_bank_detect_frames(
            self._h, ptr, n, H, W, on_dev, int(roi_w), float(scaleFactor), int(minNeighbors), r, c, k, C.byref(rh)))

    def detect_frame_list(self, ptrs, H: int, W: int, roi_w: int = 300, scaleFactor=1.1, minNeighbors=5,
                          cap: int = 256):
        """detect_frames over frames already in device memory at separate addresses `ptrs` (each [H, W, 3])."""
        L = load()
        n = len(ptrs)
        arr = (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
        rh = C.c_int32()
        return self._results("fm_haar_bank_detect_frame_list", n, cap, lambda r, c, k: L.fm_haar_bank_detect_frame_list(
            self._h, C.cast(arr, C.c_void_p), n, int(H), int(W), int(roi_w), float(scaleFactor), int(minNeighbors),
            r, c, k, C.byref(rh)))

    def detect_frame_list_async(self, ptrs, H: int, W: int, roi_w: int = 300, scaleFactor=1.1, minNeighbors=5) -> int:
        """detect_frame_list queued on the bank's stream without waiting; `collect` returns its results.  One
        detection in flight per bank; the frames stay in place until it is collected.  Returns the frame count."""
        L = load()
        n = len(ptrs)
        arr = (C.c_void_p * max(n, 1))(*[int(p) for p in ptrs])
        rh = C.c_int32()
        rc = L.fm_haar_bank_detect_frame_list_async(self._h, C.cast(arr, C.c_void_p), n, int(H), int(W), int(roi_w),
                                                    float(scaleFactor), int(minNeighbors), C.byref(rh))
        if rc != FM_OK:
            raise FMError(rc, f"fm_haar_bank_detect_frame_list_async: {L.fm_haar_bank_last_error(self._h).decode()}")
        return n

    def collect(self, n: int, cap: int = 256):
        """The queued detection's results (waits for it), as detect_frame_list returns them."""
        L = load()
        return self._results("fm_haar_bank_collect", int(n), cap,
                             lambda r, c, k: L.fm_haar_bank_collect(self._h, r, c, k, int(n)))

    def candidates(self, member: int) -> np.ndarray:
        """Ungrouped candidates of image 0 of the last call, for one member (parity tests)."""
        L = load()
        if not 0 <= int(member) < len(self.cascades):
            raise IndexError(f"member {member} of {len(self.cascades)}")
        n = L.fm_haar_bank_candidates(self._h, int(member), None, 0)
        out = np.zeros((max(n, 1), 4), np.int32)
        L.fm_haar_bank_candidates(self._h, int(member), _ptr(out), n)
        return out[:n]

    def last_ms(self) -> float:
        return float(load().fm_haar_bank_last_ms(self._h))

    def close(self):
        if self._h:
            load().fm_haar_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def yolo_desc(layers, params, net_w=416, net_h=416, max_frames=1, zero_thresh=0.2, channels=None):
    """darknet.parse_cfg's layer list + darknet.load_weights' parameters -> (FMYoloDesc, keep-alive list).
    The description is passed on as parsed: fm_yolo_create does the checking."""
    from . import darknet as dk
    kinds = {dk.CONV: YOLO_CONV, dk.MAXPOOL: YOLO_MAXPOOL, dk.UPSAMPLE: YOLO_UPSAMPLE, dk.ROUTE: YOLO_ROUTE,
             dk.SHORTCUT: YOLO_SHORTCUT, dk.YOLO: YOLO_HEAD}
    arr = (FMYoloLayer * max(len(layers), 1))()
    ws, bs, anchors = [], [], []
    nw = nb = 0
    classes = 0
    for i, ly in enumerate(layers):
        q = arr[i]
        q.kind = kinds.get(ly["kind"], -1)
        q.src[0] = q.src[1] = -1
        if ly["kind"] == dk.CONV:
            w, b = params[i]
            w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
            q.filters, q.size, q.stride, q.pad = ly["filters"], ly["size"], ly["stride"], ly["pad"]
            q.leaky = 1 if ly["activation"] == "leaky" else 0
            q.weight_ofs, q.bias_ofs = nw, nb
            ws.append(w.ravel())
            bs.append(b.ravel())
            nw += w.size
            nb += b.size
        elif ly["kind"] == dk.MAXPOOL:
            q.size, q.stride = ly["size"], ly["stride"]
        elif ly["kind"] == dk.UPSAMPLE:
            q.stride = ly["stride"]
        elif ly["kind"] == dk.ROUTE:
            for k, s in enumerate(ly["layers"][:2]):
                q.src[k] = s
        elif ly["kind"] == dk.SHORTCUT:
            q.src[0] = ly["from"]
        elif ly["kind"] == dk.YOLO:
            q.n_mask, q.anchor_ofs = len(ly["mask"]), len(anchors)
            anchors.extend(ly["anchors"][m] for m in ly["mask"])
            classes = ly["classes"] if classes in (0, ly["classes"]) else -1
    wv = np.concatenate(ws).astype(np.float32) if ws else np.zeros(0, np.float32)
    bv = np.concatenate(bs).astype(np.float32) if bs else np.zeros(0, np.float32)
    av = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(-1, 2))
    if channels is None:
        channels = layers[0]["in_c"] if layers else 3
    d = FMYoloDesc(len(layers), arr, _ptr(wv), wv.size, _ptr(bv), bv.size, _ptr(av), len(av), int(channels),
                   int(net_w), int(net_h), int(classes), int(max_frames), float(zero_thresh))
    return d, [arr, wv, bv, av]


class YoloDetector:
    """cvlib.detect_common_objects on the GPU from the user's Darknet files (find_motion.py:733-741).

    `YoloDetector.from_dir(dir, tiny)` reads yolov3[-tiny].cfg, yolov3[-tiny].weights and
    yolov3_classes.txt (find_motion_amd.darknet); `detect_frames` returns cvlib's (bboxes, labels, confs)
    per frame.  The network input is 416 x 416 whatever the cfg's [net] says, as cvlib passes it.
    precision "f16" keeps weights and activations in half precision (fm_yolo_create_precision); the default
    "f32" is the arithmetic the parity tests pin."""

    def __init__(self, layers, params, classes, net_w: int = 416, net_h: int = 416, max_frames: int = 1,
                 zero_thresh: float = 0.2, device: int = 0, channels=None, roi_upscale: bool = False,
                 precision: str = "f32"):
        # roi_upscale: frames narrower than roi_w are enlarged, as imutils.resize does (else FM_ENOTSUP)
        if precision not in YOLO_PRECISIONS:
            raise ValueError(f"precision {precision!r}: one of {sorted(YOLO_PRECISIONS)}")
        self._precision = precision
        L = load()
        self.layers, self.classes = layers, list(classes)
        self.net_w, self.net_h, self.max_frames = int(net_w), int(net_h), int(max_frames)
        d, self._keep = yolo_desc(layers, params, net_w, net_h, max_frames, zero_thresh, channels)
        h = C.c_void_p()
        rc = L.fm_yolo_create_precision(int(device), C.byref(d), YOLO_PRECISIONS[precision], C.byref(h))
        self._h = h
        if rc != FM_OK:
            msg = L.fm_yolo_last_error(h).decode() if h else ""
            L.fm_yolo_destroy(h)
            self._h = None
            raise FMError(rc, f"fm_yolo_create: {msg}")
        if roi_upscale:
            self.set_roi_upscale(True)
        rows = C.c_int()
        L.fm_yolo_layer_shape(self._h, -1, None, None, None, C.byref(rows))
        self.rows = rows.value  # candidate rows of all heads, per frame

    @property
    def precision(self) -> str:
        """"f32" or "f16": what the detector was created with."""
        return self._precision

    def set_roi_upscale(self, on: bool) -> None:
        load().fm_yolo_set_roi_upscale(self._h, int(bool(on)))

    @classmethod
    def from_dir(cls, directory, tiny: bool = False, device: int = 0, **kw):
        from . import darknet as dk
        stem = os.path.join(directory, "yolov3-tiny" if tiny else "yolov3")
        with open(stem + ".cfg", "r") as f:
            _net, layers = dk.parse_cfg(f.read())
        params = dk.load_weights(stem + ".weights", layers)
        classes = dk.load_classes(os.path.join(directory, "yolov3_classes.txt"))
        nc = {ly["classes"] for ly in layers if ly["kind"] == dk.YOLO}
        if not nc or any(n > len(classes) for n in nc):
            raise ValueError(f"{stem}.cfg: heads of {sorted(nc)} classes, {len(classes)} names in yolov3_classes.txt")
        return cls(layers, params, classes, device=device, **kw)

    def _fail(self, rc: int, what: str):
        raise FMError(rc, f"{what}: {load().fm_yolo_last_error(self._h).decode()}")

    def _run(self, call, n: int, what: str):
        """call(cand, cap, counts) until the rows fit: a list of [k, 9] float32 arrays, one per frame."""
        cap = 64
        while True:
            cand = np.zeros((n, cap, YOLO_CAND), np.float32)
            counts = np.zeros(n, np.int32)
            rc = call(_ptr(cand), cap, _ptr(counts))
            if rc != FM_OK:
                self._fail(rc, what)
            if counts.max(initial=0) <= cap:
                return [cand[i, :counts[i]].copy() for i in range(n)]
            cap = int(counts.max())

    def candidates(self, frames, width: int = 300, confidence: float = 0.25):
        """The decoded rows above the confidence of each frame, sorted by (head, row), and the ROI height.
        `frames` as CascadeClassifier.detect_frames takes them: a host array [n, H, W, 3] BGR, a contiguous
        uint8 torch tensor on the detector's GPU, or a tuple (device address, n, H, W)."""
        L = load()
        rh = C.c_int32()
        if isinstance(frames, tuple):
            ptr, n, H, W = frames
            fr, ptr, on_dev = None, C.c_void_p(ptr), 1
        elif getattr(frames, "is_cuda", False):
            import torch
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
                raise ValueError("device frames must be a contiguous uint8 tensor [n, H, W, 3]")
            torch.cuda.current_stream(frames.device).synchronize()
            fr, ptr, on_dev = frames, C.c_void_p(frames.data_ptr()), 1
            n, H, W = frames.shape[:3]
        else:
            fr = np.ascontiguousarray(frames, np.uint8)
            if fr.ndim != 4 or fr.shape[3] != 3:
                raise ValueError("frames must be [n, H, W, 3]")
            ptr, on_dev = _ptr(fr), 0
            n, H, W = fr.shape[:3]
        n, H, W = int(n), int(H), int(W)
        rows = self._run(lambda c, cap, k: L.fm_yolo_detect_frames(self._h, ptr, n, H, W, on_dev, int(width),
                                                                   float(confidence), c, cap, k, C.byref(rh)),
                         n, "fm_yolo_detect_frames")
        return rows, rh.value

    def candidates_frame_list(self, ptrs, H: int, W: int, width: int = 300, confidence: float = 0.25):
        """`candidates` over frames in device memory at separate addresses (fm_yolo_detect_frame_list)."""
        L = load()
        n = len(ptrs)
        arr = (C.c_void_p * n)(*[int(p) for p in ptrs])
        rh = C.c_int32()
        rows = self._run(lambda c, cap, k: L.fm_yolo_detect_frame_list(self._h, C.cast(arr, C.c_void_p), n, int(H),
                                                                       int(W), int(width), float(confidence), c, cap,
                                                                       k, C.byref(rh)),
                         n, "fm_yolo_detect_frame_list")
        return rows, rh.value

    def detect_frames(self, frames, width: int = 300, confidence: float = 0.25, nms: float = 0.3):
        """cvlib.detect_common_objects(imutils.resize(frame, width=width), confidence, nms) per frame:
        a list of (bboxes [x1, y1, x2, y2], labels, confs)."""
        from . import darknet as dk
        rows, rh = self.candidates(frames, width, confidence)
        return [dk.detections(r, int(width), rh, self.classes, confidence, nms) for r in rows]

    def detect_frame_list(self, ptrs, H: int, W: int, width: int = 300, confidence: float = 0.25, nms: float = 0.3):
        from . import darknet as dk
        rows, rh = self.candidates_frame_list(ptrs, H, W, width, confidence)
        return [dk.detections(r, int(width), rh, self.classes, confidence, nms) for r in rows]

    # -- parity tests ------------------------------------------------------------
    def forward(self, blob) -> None:
        """The network alone on a host blob [n, channels, net_h, net_w] float32 (fm_yolo_forward)."""
        b = np.ascontiguousarray(blob, np.float32)
        rc = load().fm_yolo_forward(self._h, _ptr(b), int(b.shape[0]))
        if rc != FM_OK:
            self._fail(rc, "fm_yolo_forward")

    def decode(self, n: int, confidence: float = 0.25):
        """The decode alone on the last call's head tensors (fm_yolo_decode)."""
        L = load()
        return self._run(lambda c, cap, k: L.fm_yolo_decode(self._h, int(n), float(confidence), c, cap, k), int(n),
                         "fm_yolo_decode")

    def layer_shape(self, layer: int):
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        if load().fm_yolo_layer_shape(self._h, int(layer), C.byref(c), C.byref(h), C.byref(w), None) != FM_OK:
            raise IndexError(f"layer {layer}")
        return c.value, h.value, w.value

    def layer_output(self, layer: int, n: int) -> np.ndarray:
        """Layer `layer`'s activations [n, c, h, w] of the last call over n frames (-1: the network input)."""
        out = np.zeros((int(n),) + self.layer_shape(layer), np.float32)
        rc = load().fm_yolo_layer_output(self._h, int(layer), _ptr(out), out.size)
        if rc < 0:
            self._fail(rc, "fm_yolo_layer_output")
        if rc != out.size:
            raise FMError(FM_ESTATE, f"fm_yolo_layer_output: the last call ran {rc // max(out[0].size, 1)} frames, not {n}")
        return out

    def route_in_place(self, layer: int) -> bool:
        rc = load().fm_yolo_route_in_place(self._h, int(layer))
        if rc < 0:
            raise IndexError(f"layer {layer} is not a route")
        return bool(rc)

    def last_ms(self) -> dict:
        st = (C.c_double * 3)()
        total = float(load().fm_yolo_last_ms(self._h, C.cast(st, C.c_void_p)))
        return {"blob": st[0], "network": st[1], "decode": st[2], "total": total}

    def close(self):
        if self._h:
            load().fm_yolo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _jpeg_arrays(jpegs):
    """(pointer array, size array, keep-alive list) for a sequence of JPEG byte strings."""
    keep = [np.frombuffer(j, np.uint8) if not isinstance(j, np.ndarray) else np.ascontiguousarray(j, np.uint8)
            for j in jpegs]
    ptrs = np.array([k.ctypes.data for k in keep], np.uint64)
    sizes = np.array([k.size for k in keep], np.uint64)
    return ptrs, sizes, keep


class MJpegDecoder:
    """The decode side on the GPU: baseline JPEG frames of an MJPEG stream ->
    BGR u8 frames as cv2.VideoCapture.read returns them (fm.py:497-506), libjpeg-turbo's default
    decode reproduced bit for bit (jpeg_idct_islow, fancy upsampling, integer YCbCr tables)."""

    def __init__(self, width: int, height: int, max_frames: int = 64, device: int = 0,
                 chunk_bits: int | None = None, spec_bits: int | None = None):
        L = load()
        h = C.c_void_p()
        rc = L.fm_mjpeg_create(int(device), int(width), int(height), int(max_frames), C.byref(h))
        self._h = h
        if rc != FM_OK:
            msg = L.fm_mjpeg_last_error(h).decode() if h else ""
            L.fm_mjpeg_destroy(h)
            self._h = None
            raise FMError(rc, f"fm_mjpeg_create: {msg}")
        self.width, self.height, self.max_frames = int(width), int(height), int(max_frames)
        if chunk_bits is not None or spec_bits is not None:  # fm_mjpeg_tune: speed only, same results
            rc = L.fm_mjpeg_tune(h, int(chunk_bits or 512), int(512 if spec_bits is None else spec_bits))
            if rc != FM_OK:
                msg = L.fm_mjpeg_last_error(h).decode()
                self.close()
                raise FMError(rc, f"fm_mjpeg_tune: {msg}")

    def decode(self, jpegs) -> np.ndarray:
        """JPEG byte strings -> BGR u8 [n, H, W, 3] (host)."""
        L = load()
        ptrs, sizes, keep = _jpeg_arrays(jpegs)
        out = np.empty((len(keep), self.height, self.width, 3), np.uint8)
        rc = L.fm_mjpeg_decode(self._h, _ptr(ptrs), _ptr(sizes), len(keep), _ptr(out), 0)
        if rc != FM_OK:
            raise FMError(rc, f"fm_mjpeg_decode: {L.fm_mjpeg_last_error(self._h).decode()}")
        return out

    def decode_device(self, jpegs, ptr: int) -> None:
        """JPEG byte strings -> BGR frames at device address ptr (synchronous)."""
        L = load()
        ptrs, sizes, keep = _jpeg_arrays(jpegs)
        rc = L.fm_mjpeg_decode(self._h, _ptr(ptrs), _ptr(sizes), len(keep), C.c_void_p(ptr), 1)
        if rc != FM_OK:
            raise FMError(rc, f"fm_mjpeg_decode: {L.fm_mjpeg_last_error(self._h).decode()}")

    def last_ms(self) -> float:
        return float(load().fm_mjpeg_last_ms(self._h))

    def close(self):
        if self._h:
            load().fm_mjpeg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def jpeg_header(width: int, height: int, quality: int = 95, subsampling: int = 2, restart_interval: int = 0) -> bytes:
    """The bytes from SOI through the SOS segment of the JPEGs MJpegEncoder writes (fm_jpeg_header; host only)."""
    L = load()
    n = C.c_size_t()
    args = (int(width), int(height), int(quality), int(subsampling), int(restart_interval))
    L.fm_jpeg_header(*args, None, 0, C.byref(n))
    buf = np.empty(max(n.value, 1), np.uint8)
    rc = L.fm_jpeg_header(*args, _ptr(buf), buf.size, C.byref(n))
    if rc != FM_OK:
        raise FMError(rc, f"fm_jpeg_header: bad settings {args}")
    return buf[:n.value].tobytes()


class MJpegEncoder:
    """The write side on the GPU: BGR u8 frames -> baseline JPEGs, byte for byte what Pillow's libjpeg-turbo
    writes for Image.save(..., "JPEG", quality=quality, subsampling=subsampling[, restart_marker_blocks=
    restart_interval]) -- the bytes videoio.MjpegAviWriter writes on the host (fm.py:447-546 with codec 'MJPG').
    subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0; restart_interval in MCUs, 0 = none."""

    def __init__(self, width: int, height: int, max_frames: int = 64, device: int = 0, quality: int = 95,
                 subsampling: int = 2, restart_interval: int = 0):
        L = load()
        h = C.c_void_p()
        rc = L.fm_mjpeg_enc_create(int(device), int(width), int(height), int(max_frames), int(quality),
                                   int(subsampling), int(restart_interval), C.byref(h))
        self._h = h
        if rc != FM_OK:
            msg = L.fm_mjpeg_enc_last_error(h).decode() if h else ""
            L.fm_mjpeg_enc_destroy(h)
            self._h = None
            raise FMError(rc, f"fm_mjpeg_enc_create: {msg}")
        self.width, self.height, self.max_frames, self.device = int(width), int(height), int(max_frames), int(device)
        self.quality, self.subsampling, self.restart_interval = int(quality), int(subsampling), int(restart_interval)
        hs, vs = (1, 1) if subsampling == 0 else (2, 1) if subsampling == 1 else (2, 2)
        self.blocks = -(-self.width // (8 * hs)) * -(-self.height // (8 * vs)) * (hs * vs + 2)

    def _fail(self, rc: int, what: str):
        raise FMError(rc, f"{what}: {load().fm_mjpeg_enc_last_error(self._h).decode()}")

    def _collect(self, n: int) -> list:
        L = load()
        out = []
        ln = C.c_size_t()
        for i in range(n):
            L.fm_mjpeg_enc_get(self._h, i, None, 0, C.byref(ln))  # the size
            buf = np.empty(max(ln.value, 1), np.uint8)
            rc = L.fm_mjpeg_enc_get(self._h, i, _ptr(buf), buf.size, C.byref(ln))
            if rc != FM_OK:
                self._fail(rc, "fm_mjpeg_enc_get")
            out.append(buf[:ln.value].tobytes())
        return out

    def encode(self, frames) -> list:
        """Host frames [n, H, W, 3] (or one [H, W, 3]) BGR u8 -> list of JPEG byte strings."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.ndim == 3:
            f = f[None]
        if f.ndim != 4 or f.shape[1:] != (self.height, self.width, 3):
            raise FMError(FM_EINVAL, f"frames of shape {f.shape}, the encoder takes [n, {self.height}, {self.width}, 3]")
        rc = load().fm_mjpeg_encode(self._h, _ptr(f), f.shape[0], 0)
        if rc != FM_OK:
            self._fail(rc, "fm_mjpeg_encode")
        return self._collect(f.shape[0])

    def encode_device(self, ptrs_or_ptr, n: int | None = None) -> list:
        """Frames already in device memory: one address of n contiguous frames [n, H, W, 3] (an int, or a
        contiguous uint8 torch tensor on the encoder's GPU), or a sequence of addresses of single frames
        (e.g. MotionEngine.frame_device_ptr).  The frames must be complete on the device."""
        L = load()
        src = ptrs_or_ptr
        if getattr(src, "is_cuda", False):
            import torch
            if src.dtype != torch.uint8 or not src.is_contiguous() or tuple(src.shape[-3:]) != (self.height, self.width, 3):
                raise FMError(FM_EINVAL, f"device frames must be a contiguous uint8 tensor [n, {self.height}, {self.width}, 3]")
            torch.cuda.current_stream(src.device).synchronize()
            n = 1 if src.dim() == 3 else int(src.shape[0])
            rc = L.fm_mjpeg_encode(self._h, C.c_void_p(src.data_ptr()), n, 1)
        elif isinstance(src, (int, np.integer)):
            if n is None:
                raise ValueError("n is required with a single device address")
            rc = L.fm_mjpeg_encode(self._h, C.c_void_p(int(src)), int(n), 1)
        else:
            ptrs = [int(p) for p in src]
            n = len(ptrs) if n is None else int(n)
            if n > len(ptrs):
                raise ValueError(f"{len(ptrs)} addresses for n = {n}")
            arr = (C.c_void_p * max(n, 1))(*ptrs[:n])
            rc = L.fm_mjpeg_encode_frame_list(self._h, C.cast(arr, C.c_void_p), n)
        if rc != FM_OK:
            self._fail(rc, "fm_mjpeg_encode")
        return self._collect(int(n))

    def coefficients(self, i: int) -> np.ndarray:
        """Quantized coefficients of frame i of the last call: int16 [blocks, 64], scan order, zigzag."""
        out = np.empty((self.blocks, 64), np.int16)
        rc = load().fm_mjpeg_enc_coefficients(self._h, int(i), _ptr(out), out.size)
        if rc < 0:
            self._fail(rc, "fm_mjpeg_enc_coefficients")
        return out

    def last_ms(self) -> float:
        return float(load().fm_mjpeg_enc_last_ms(self._h))

    def close(self):
        if self._h:
            load().fm_mjpeg_enc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
