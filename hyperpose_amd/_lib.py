"""ctypes binding of libhp_hip.so (include/hp_hip.h).  Fails loudly: there is NO CPU fallback.

The shared library is built in-tree by ``python -m hyperpose_amd.build`` (hipcc, gfx950).  Importing this
module never needs a GPU; calling into it does (hp_init reports HP_ERR_NO_DEVICE otherwise).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libhp_hip.so")

HP_OK = 0
HP_ERR_INVALID, HP_ERR_HIP, HP_ERR_CAPACITY, HP_ERR_STATE, HP_ERR_NO_DEVICE = -1, -2, -3, -4, -5
HP_YUV_NV12, HP_YUV_I420 = 0, 1
YUV_FORMATS = {"nv12": HP_YUV_NV12, "i420": HP_YUV_I420}  # what hp_resize_yuv420 / hp_pipeline_submit_yuv take
HP_YUV_P010, HP_YUV_I010, HP_YUV_NV16, HP_YUV_I422, HP_YUV_YUY2, HP_YUV_UYVY, HP_YUV_I444 = 2, 3, 4, 5, 6, 7, 8
HP_YUV_BT601, HP_YUV_BT709, HP_YUV_BT2020 = 0, 1, 2
HP_YUV_LIMITED, HP_YUV_FULL = 0, 1
# every layout hp_yuv_image names: (code, planes, bytes per sample, chroma shift x, chroma shift y).  The names, the codes and the sample
# width (which numpy dtype a plane has) are what Python needs of its own; the geometry of the planes comes from hp_yuv_plane_layout
# (frontend.yuv_plane_shapes), and tests/test_yuv_formats_convert.py ties this table to it
YUV_LAYOUTS = {"nv12": (0, 2, 1, 1, 1), "i420": (1, 3, 1, 1, 1), "p010": (2, 2, 2, 1, 1), "i010": (3, 3, 2, 1, 1), "nv16": (4, 2, 1, 1, 0),
               "i422": (5, 3, 1, 1, 0), "yuy2": (6, 1, 1, 1, 0), "uyvy": (7, 1, 1, 1, 0), "i444": (8, 3, 1, 0, 0)}
# every layout hp_rgb_image names (a type of its own, not hp_yuv_image formats): (code, bytes per pixel, byte offsets of B, G, R inside a pixel);
# hyperpose_amd/csrc/rgb_formats.hpp holds the same table, tests/test_rgb_host.py ties the two together
HP_RGB_BGR24, HP_RGB_RGB24, HP_RGB_BGRA32, HP_RGB_RGBA32, HP_RGB_ARGB32, HP_RGB_ABGR32, HP_RGB_GRAY8 = 0, 1, 2, 3, 4, 5, 6
RGB_LAYOUTS = {"bgr24": (0, 3, 0, 1, 2), "rgb24": (1, 3, 2, 1, 0), "bgra": (2, 4, 0, 1, 2), "rgba": (3, 4, 2, 1, 0), "argb": (4, 4, 3, 2, 1),
               "abgr": (5, 4, 1, 2, 3), "gray": (6, 1, 0, 0, 0)}
YUV_MATRICES = {"bt601": HP_YUV_BT601, "bt709": HP_YUV_BT709, "bt2020": HP_YUV_BT2020}
YUV_RANGES = {"limited": HP_YUV_LIMITED, "full": HP_YUV_FULL}


class HpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libhp_hip error {code}: {msg}")
        self.code = code


class BodyPart(C.Structure):
    _fields_ = [("has_value", C.c_int32), ("x", C.c_float), ("y", C.c_float), ("score", C.c_float)]


class Human(C.Structure):
    _fields_ = [("parts", BodyPart * 18), ("score", C.c_float)]


class Peak(C.Structure):
    _fields_ = [("part_id", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("score", C.c_float), ("id", C.c_int32)]


class Conn(C.Structure):
    _fields_ = [("pair_id", C.c_int32), ("cid1", C.c_int32), ("cid2", C.c_int32), ("score", C.c_float)]


class YuvImage(C.Structure):
    """hp_yuv_image"""
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("plane", C.c_void_p * 3), ("stride", C.c_int32 * 3)]


class RgbImage(C.Structure):
    """hp_rgb_image"""
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("data", C.c_void_p), ("stride", C.c_int32)]


class OverlayPrim(C.Structure):
    """hp_overlay_prim"""
    _fields_ = [(k, C.c_int32) for k in ("kind", "x0", "y0", "x1", "y1", "t", "colour", "human")]


class RedactRegion(C.Structure):
    """hp_redact_region"""
    _fields_ = [(k, C.c_int32) for k in ("kind", "x0", "y0", "x1", "y1", "human")]


HP_REDACT_RECT, HP_REDACT_DISC = 0, 1
HP_REDACT_HEAD, HP_REDACT_BODY = 0, 1
HP_REDACT_PIXELATE, HP_REDACT_BLACK = 0, 1
REDACT_WHAT = {"head": HP_REDACT_HEAD, "body": HP_REDACT_BODY}
REDACT_EFFECTS = {"pixelate": HP_REDACT_PIXELATE, "black": HP_REDACT_BLACK}


class Roi(C.Structure):
    """hp_roi: a region of a frame in source pixels"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class MapViewDesc(C.Structure):
    """hp_mapview_desc"""
    _fields_ = [("maps", C.c_void_p), ("C", C.c_int32), ("mh", C.c_int32), ("mw", C.c_int32), ("frame", C.c_int32), ("c0", C.c_int32), ("cn", C.c_int32),
                ("c_step", C.c_int32), ("mode", C.c_int32), ("gain", C.c_float), ("cover_x", C.c_double), ("cover_y", C.c_double),
                ("orientation", C.c_int32), ("roi", Roi), ("has_roi", C.c_int32)]


HP_MAPVIEW_MAX, HP_MAPVIEW_FIELD = 0, 1
MAPVIEW_MODES = {"max": HP_MAPVIEW_MAX, "field": HP_MAPVIEW_FIELD}
MAPVIEW_PALETTES = {"jet": 0, "heat": 1, "grey": 2}
MAPVIEW_ALPHAS = {"constant": 0, "scaled": 1}


class FlipOutput(C.Structure):
    """hp_flip_output"""
    _fields_ = [("output", C.c_int32), ("perm", C.POINTER(C.c_int32)), ("sign", C.POINTER(C.c_int8))]


class HdrDesc(C.Structure):
    """hp_hdr_desc"""
    _fields_ = [("transfer", C.c_int32), ("to_bt709", C.c_int32), ("peak_nits", C.c_float), ("white_nits", C.c_float)]


HP_TRC_PQ, HP_TRC_HLG = 1, 2
HDR_TRANSFERS = {"pq": HP_TRC_PQ, "hlg": HP_TRC_HLG}
# the mirrors' tone-map defaults (HP_HDR_DEFAULT_* in include/hp_hip.h)
HDR_DEFAULT_PEAK, HDR_DEFAULT_WHITE = 1000.0, 203.0


class Tiling(C.Structure):
    """hp_tiling"""
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("overlap_x", C.c_int32), ("overlap_y", C.c_int32), ("with_full", C.c_int32),
                ("min_common", C.c_int32), ("tol", C.c_double)]


# the mirrors' merge defaults (HP_TILING_DEFAULT_* in include/hp_hip.h)
TILING_DEFAULT_MIN_COMMON, TILING_DEFAULT_TOL = 3, 0.08

PART_DTYPE = np.dtype([("has_value", "<i4"), ("x", "<f4"), ("y", "<f4"), ("score", "<f4")])
HUMAN_DTYPE = np.dtype({"names": ["parts", "score"], "formats": [(PART_DTYPE, 18), "<f4"]})
PEAK_DTYPE = np.dtype([("part_id", "<i4"), ("x", "<i4"), ("y", "<i4"), ("score", "<f4"), ("id", "<i4")])
OVERLAY_PRIM_DTYPE = np.dtype([(k, "<i4") for k in ("kind", "x0", "y0", "x1", "y1", "t", "colour", "human")])
REDACT_REGION_DTYPE = np.dtype([(k, "<i4") for k in ("kind", "x0", "y0", "x1", "y1", "human")])
CONN_DTYPE = np.dtype([("pair_id", "<i4"), ("cid1", "<i4"), ("cid2", "<i4"), ("score", "<f4")])
assert HUMAN_DTYPE.itemsize == C.sizeof(Human) == 292

_lib = None

# every symbol include/hp_hip.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "hp_init", "hp_device_count", "hp_last_error", "hp_version", "hp_malloc", "hp_free", "hp_malloc_host",
    "hp_free_host", "hp_memcpy_h2d", "hp_memcpy_d2h", "hp_device_synchronize", "hp_stream_wait_stream", "hp_dist_unique_id", "hp_dist_init", "hp_dist_destroy", "hp_dist_broadcast_weights", "hp_dist_shard", "hp_preproc_u8hwc_to_f32nchw", "hp_resize_u8c3", "hp_letterbox_u8c3", "hp_letterbox_inner", "hp_resume_ratio",
    "hp_resize_yuv420", "hp_letterbox_yuv420", "hp_pipeline_submit_yuv",
    "hp_resize_yuv", "hp_letterbox_yuv", "hp_yuv_coefficients", "hp_yuv_packed_bytes", "hp_yuv_plane_layout", "hp_pipeline_submit_yuv_images",
    "hp_overlay_create", "hp_overlay_destroy", "hp_overlay_primitives", "hp_yuv_colours", "hp_overlay_draw_u8c3", "hp_overlay_draw_yuv",
    "hp_overlay_draw_u8c3_host", "hp_overlay_draw_yuv_host",
    "hp_redact_create", "hp_redact_destroy", "hp_redact_regions", "hp_redact_u8c3", "hp_redact_yuv", "hp_redact_u8c3_host", "hp_redact_yuv_host",
    "hp_mapview_create", "hp_mapview_destroy", "hp_mapview_cover", "hp_mapview_taps", "hp_mapview_palette", "hp_mapview_palette_yuv",
    "hp_mapview_draw_u8c3", "hp_mapview_draw_yuv", "hp_mapview_draw_u8c3_host", "hp_mapview_draw_yuv_host", "hp_mapview_index_host", "hp_mapview_debug_plane",
    "hp_paf_create", "hp_paf_stream", "hp_paf_destroy", "hp_paf_set_conf_thresh", "hp_paf_set_paf_thresh", "hp_paf_process_batch",
    "hp_paf_enqueue", "hp_paf_collect", "hp_paf_debug_peaks", "hp_paf_debug_conns", "hp_paf_debug_maps", "hp_paf_debug_sort",
    "hp_pifpaf_create", "hp_pifpaf_destroy", "hp_pifpaf_process_batch", "hp_pifpaf_stream", "hp_pifpaf_enqueue", "hp_pifpaf_collect", "hp_pifpaf_decode_flags",
    "hp_ppn_create", "hp_ppn_destroy", "hp_ppn_set_thresholds", "hp_ppn_process_batch", "hp_ppn_stream", "hp_ppn_enqueue", "hp_ppn_collect", "hp_ppn_decode_flags",
    "hp_engine_create", "hp_engine_destroy", "hp_engine_max_batch", "hp_engine_describe", "hp_engine_input_size", "hp_engine_infer_u8",
    "hp_engine_infer_f32", "hp_engine_synchronize", "hp_engine_stream", "hp_engine_set_graph", "hp_engine_set_concurrency", "hp_engine_arena_info", "hp_debug_first_conv_verify", "hp_engine_concurrency", "hp_engine_cached_graphs", "hp_engine_num_outputs",
    "hp_engine_output", "hp_engine_output_to_host", "hp_engine_debug_tensor", "hp_engine_debug_raw_tensor", "hp_engine_profile", "hp_engine_profile_sequence", "hp_engine_profile_pair", "hp_model_build", "hp_model_from_onnx", "hp_model_from_onnx_file", "hp_model_weights",
    "hp_model_input_size",
    "hp_model_destroy", "hp_model_archs", "hp_model_layers", "hp_model_outputs", "hp_model_num_weights",
    "hp_model_preproc", "hp_model_flops_per_frame", "hp_model_init_weights", "hp_engine_create_from_model", "hp_engine_create_from_model_dtype", "hp_engine_dtype", "hp_engine_calibrate_u8", "hp_engine_int8_scales", "hp_engine_set_int8_scales", "hp_engine_split_fallbacks", "hp_engine_device_bytes", "hp_engine_save", "hp_engine_load", "hp_pipeline_create", "hp_pipeline_create_ex", "hp_pipeline_destroy", "hp_pipeline_submit", "hp_pipeline_collect", "hp_pipeline_in_flight",
    "hp_tonemap_tables", "hp_tonemap_create", "hp_tonemap_destroy", "hp_resize_yuv_hdr", "hp_letterbox_yuv_hdr", "hp_resize_rois_yuv_hdr",
    "hp_tonemap_convert_host", "hp_yuv_colours_hdr", "hp_overlay_set_transfer", "hp_overlay_draw_yuv_host_hdr", "hp_pipeline_set_tonemap",
    "hp_resize_rois_u8c3", "hp_resize_rois_yuv", "hp_yuv_roi_alignment", "hp_tile_plan", "hp_humans_to_frame", "hp_humans_merge", "hp_pipeline_set_tiling",
    "hp_resize_oriented_u8c3", "hp_resize_oriented_yuv", "hp_resize_rois_oriented_u8c3", "hp_resize_rois_oriented_yuv", "hp_oriented_size",
    "hp_orientation_from_exif", "hp_orient_roi", "hp_orient_u8c3_host", "hp_humans_orient", "hp_pipeline_set_orientation",
    "hp_hflip_u8c3", "hp_hflip_u8c3_host", "hp_flip_merge", "hp_flip_merge_host", "hp_flip_tables_coco", "hp_engine_set_flip_ensemble",
    "hp_engine_set_flip_ensemble_coco", "hp_engine_flip_ensemble", "hp_pipeline_set_flip_ensemble",
    "hp_scale_stage_u8c3", "hp_scale_stage_u8c3_host", "hp_scale_tables", "hp_scale_merge", "hp_scale_merge_host", "hp_engine_set_scale_ensemble",
    "hp_engine_set_scale_ensemble_coco", "hp_engine_scale_ensemble", "hp_pipeline_set_scale_ensemble",
    "hp_resize_rgb", "hp_resize_rois_rgb", "hp_rgb_pixel_bytes", "hp_rgb_packed_bytes", "hp_rgb_to_bgr_host", "hp_pipeline_submit_rgb_images",
    "hp_rgb_to_yuv", "hp_rgb_to_yuv_host", "hp_yuv_forward_coefficients", "hp_yuv_padded_size",
]


def lib() -> C.CDLL:
    """Load libhp_hip.so or raise: the product path has no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -m hyperpose_amd.build` (hipcc, gfx950). "
                              "hyperpose_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.hp_last_error.restype = C.c_char_p
        L.hp_version.restype = C.c_char_p
        L.hp_yuv_packed_bytes.restype = C.c_size_t
        L.hp_rgb_packed_bytes.restype = C.c_size_t
        L.hp_humans_to_frame.restype = None
        L.hp_engine_debug_raw_tensor.restype = C.c_int
        L.hp_engine_debug_raw_tensor.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise HpError(rc, lib().hp_last_error().decode("utf-8", "replace"))
    return rc


_initialised = set()


def init(device: int = 0) -> None:
    check(lib().hp_init(int(device)))
    _initialised.add(device)


class DevBuf:
    """A device allocation owned through the C ABI (no torch needed)."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(lib().hp_malloc(C.byref(self.ptr), C.c_size_t(self.nbytes)))

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        check(lib().hp_memcpy_h2d(b.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))
        return b

    def to_numpy(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(lib().hp_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes)))
        return out

    def free(self):
        if self.ptr:
            lib().hp_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def as_ptr(x):
    """Device pointer of a DevBuf, a torch CUDA tensor or a raw int."""
    if isinstance(x, DevBuf):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))
