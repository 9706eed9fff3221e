"""``hyperpose::make_stream(engine, parser)`` on the GPU (reference include/hyperpose/stream/stream.hpp:119-145):
host frames of any size in, humans out, in submission order; see ``hp_pipeline_*`` in include/hp_hip.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (HDR_DEFAULT_PEAK, HDR_DEFAULT_WHITE, HUMAN_DTYPE, TILING_DEFAULT_MIN_COMMON, TILING_DEFAULT_TOL, YUV_FORMATS, YUV_LAYOUTS, Human, RgbImage,
                   YuvImage, check, lib)
from .engine import _DTYPES, EngineDesc, Layer, OutputDesc


class ParserDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("thresh", C.c_float * 3), ("res_w", C.c_int32), ("res_h", C.c_int32)]


PARSER_PAF, PARSER_PPN, PARSER_PIFPAF = 0, 1, 2


class Pipeline:
    """``parser`` selects the hyperpose::parser the stream ends in: "paf" (conf_thresh, paf_thresh), "ppn" (thresholds =
    (point, limb, nms), default 0.10 / 0.05 / 0.3) or "pifpaf" (thresholds = (thresh,), default 0.1)."""

    def __init__(self, model, weights: np.ndarray, max_batch: int = 8, n_pipes: int = 4, keep_ratio: bool = False,
                 conf_thresh: float = 0.05, paf_thresh: float = 0.05, max_frame_wh=(1920, 1080), factor: float = 1.0 / 255,
                 flip_rgb: bool = True, cap_per_frame: int = 128, parser: str = "paf", thresholds=None, dtype="f16",
                 int8_scales=None):
        """``dtype="i8"`` needs ``int8_scales``: the calibrated scale vector of an engine of the same model (``Engine.int8_scales``)."""
        self._h = C.c_void_p()
        weights = np.ascontiguousarray(weights, np.float32)
        larr = (Layer * len(model.layers))(*model.layers)
        oarr = (OutputDesc * len(model.outputs))(*model.outputs)
        d = EngineDesc(model.in_w, model.in_h, max_batch, factor, int(flip_rgb), (C.c_float * 3)(*model.mean),
                       (C.c_float * 3)(*model.inv_std), larr, len(model.layers), oarr, len(model.outputs),
                       weights.ctypes.data_as(C.POINTER(C.c_float)), weights.size, _DTYPES[dtype])
        if int8_scales is not None:
            scales = np.ascontiguousarray(int8_scales, np.float32).ravel()
            assert scales.size == len(model.layers)
            d.int8_scales = scales.ctypes.data_as(C.POINTER(C.c_float))
        kind = {"paf": PARSER_PAF, "ppn": PARSER_PPN, "pifpaf": PARSER_PIFPAF}[parser]
        th = thresholds if thresholds is not None else {PARSER_PAF: (conf_thresh, paf_thresh, 0.0), PARSER_PPN: (0.10, 0.05, 0.3),
                                                        PARSER_PIFPAF: (0.1, 0.0, 0.0)}[kind]
        th = tuple(th) + (0.0,) * (3 - len(th))
        pd = ParserDesc(kind, (C.c_float * 3)(*th), -1, -1)
        check(lib().hp_pipeline_create_ex(C.byref(self._h), C.byref(d), C.byref(pd), n_pipes, int(keep_ratio),
                                          C.c_size_t(max_frame_wh[0] * max_frame_wh[1] * 3)))
        self.max_batch, self.n_pipes, self.cap = max_batch, n_pipes, cap_per_frame
        self._out = (Human * (max_batch * cap_per_frame))()
        self._n = (C.c_int * max_batch)()

    def close(self):
        if self._h:
            lib().hp_pipeline_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def in_flight(self) -> int:
        return lib().hp_pipeline_in_flight(self._h)

    def set_tiling(self, cols=None, rows=None, overlap=(0, 0), with_full: bool = False, min_common: int = TILING_DEFAULT_MIN_COMMON,
                   tol: float = TILING_DEFAULT_TOL) -> None:
        """``hp_pipeline_set_tiling``: from now on a submitted frame is cut into ``cols`` x ``rows`` tiles that share at least ``overlap`` =
        (ox, oy) pixels (plus the whole frame when ``with_full``), every region takes one slot of the batch - a submit carries at most
        ``max_batch // regions`` frames - and ``collect`` returns the merged humans of each frame in the frame's coordinates.
        ``set_tiling(None)`` turns it off.  Not while batches are in flight."""
        from . import frontend
        if cols is None:
            check(lib().hp_pipeline_set_tiling(self._h, None))
            return
        t = frontend.tiling(cols, rows, overlap, with_full, min_common, tol)
        check(lib().hp_pipeline_set_tiling(self._h, C.byref(t)))

    def set_tonemap(self, transfer=None, to_bt709: bool = True, peak_nits: float = HDR_DEFAULT_PEAK, white_nits: float = HDR_DEFAULT_WHITE) -> None:
        """``hp_pipeline_set_tonemap``: from now on the P010 / I010 frames of ``submit_yuv_images`` are ``transfer`` = "pq" or "hlg" frames and are
        tone-mapped to SDR sRGB while they are resized (include/hp_hip.h, "HDR video in"); 8-bit frames are converted as before.
        ``set_tonemap(None)`` turns it off.  Not while batches are in flight."""
        from . import frontend
        if transfer is None:
            check(lib().hp_pipeline_set_tonemap(self._h, None))
            return
        d = frontend.hdr_desc(transfer, to_bt709, peak_nits, white_nits)
        check(lib().hp_pipeline_set_tonemap(self._h, C.byref(d)))

    def set_orientation(self, orientation: int = 0) -> None:
        """``hp_pipeline_set_orientation``: from now on the frames of ``submit`` and ``submit_yuv_images`` are STORED frames, turned and / or
        mirrored as the HP_ORIENT_* code ``orientation`` (0 .. 7, ``frontend.orientation_from_exif``) says; they are read upright inside the resize
        and ``collect`` returns humans normalised to the upright frame (``frontend.humans_orient`` takes them to the stored frame).  0 turns it
        off.  Not while batches are in flight; ``submit_yuv`` is refused while an orientation is set."""
        check(lib().hp_pipeline_set_orientation(self._h, int(orientation)))

    def set_flip_ensemble(self, on: bool = True) -> None:
        """``hp_pipeline_set_flip_ensemble``: from now on every network-sized slot runs with its left-right flip and the parser reads the
        merged maps (COCO tables; "paf" pipelines only).  A submit then carries at most ``max_batch // 2`` frames (tiled:
        ``max_batch // (2 * regions)``).  Not while batches are in flight."""
        check(lib().hp_pipeline_set_flip_ensemble(self._h, int(bool(on))))

    def set_scale_ensemble(self, scales=(0.5,)) -> None:
        """``hp_pipeline_set_scale_ensemble``: from now on every network-sized slot also runs shrunk by each of ``scales`` (1 .. 3 values in
        (0, 1]) and the parser reads the maps averaged over the K = len(scales) + 1 passes ("paf" pipelines only).  A submit then carries at most
        ``max_batch // (K * (2 if flip else 1))`` frames (tiled: that over the regions).  Empty ``scales`` (or None) turns it off.  Not while
        batches are in flight."""
        s = np.ascontiguousarray(list(scales or []), np.float32)
        check(lib().hp_pipeline_set_scale_ensemble(self._h, s.ctypes.data_as(C.POINTER(C.c_float)) if s.size else None, int(s.size)))

    def submit(self, frames) -> None:
        """frames: list of [h, w, 3] uint8 BGR arrays (any sizes), at most max_batch."""
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        n = len(frames)
        ptrs = (C.POINTER(C.c_uint8) * n)(*[f.ctypes.data_as(C.POINTER(C.c_uint8)) for f in frames])
        ws = (C.c_int * n)(*[f.shape[1] for f in frames])
        hs = (C.c_int * n)(*[f.shape[0] for f in frames])
        check(lib().hp_pipeline_submit(self._h, ptrs, ws, hs, n))
        self._keep = frames  # the async copies read the arrays until the batch is collected

    def submit_ptrs(self, ptrs, ws, hs, n: int) -> None:
        """Pre-marshalled form for hot loops (pinned frames allocated with hp_malloc_host)."""
        check(lib().hp_pipeline_submit(self._h, ptrs, ws, hs, n))

    def submit_yuv(self, frames, fmt: str = "nv12") -> None:
        """frames: list of [h*3/2, w] uint8 YUV 4:2:0 arrays (the layout cv2 and ffmpeg use: Y rows, then the chroma rows; even w and h),
        ``fmt`` "nv12" or "i420".  They go up in their 1.5-byte form and are converted to BGR inside the resize kernel."""
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        n = len(frames)
        for f in frames:
            if f.ndim != 2 or f.shape[0] % 3:
                raise ValueError(f"submit_yuv: a frame must be a [h*3/2, w] array, got shape {f.shape}")
        ptrs = (C.POINTER(C.c_uint8) * n)(*[f.ctypes.data_as(C.POINTER(C.c_uint8)) for f in frames])
        ws = (C.c_int * n)(*[f.shape[1] for f in frames])
        hs = (C.c_int * n)(*[f.shape[0] * 2 // 3 for f in frames])
        check(lib().hp_pipeline_submit_yuv(self._h, YUV_FORMATS[fmt], ptrs, ws, hs, n))
        self._keep = frames

    def submit_yuv_ptrs(self, fmt: str, ptrs, ws, hs, n: int) -> None:
        """Pre-marshalled form of ``submit_yuv`` for hot loops (pinned frames allocated with hp_malloc_host)."""
        check(lib().hp_pipeline_submit_yuv(self._h, YUV_FORMATS[fmt], ptrs, ws, hs, n))

    def submit_yuv_images(self, frames, fmt="nv12", matrix="bt601", range="limited", on_device: bool = False) -> None:
        """Video frames of any layout ``hp_yuv_image`` names (``hp_pipeline_submit_yuv_images``).  A frame is the list of its 2-D plane
        arrays (``frontend.yuv_planes``; uint16 words for the 10-bit layouts; row-padded views keep their stride) or, ready-made, a
        ``YuvImage`` (``frontend.yuv_image``), which is the only form of a device-resident frame.  ``fmt``, ``matrix`` and ``range`` are one
        name for the batch or one per frame.  ``on_device=True``: the planes are device pointers and nothing is copied; the surfaces must
        be complete now and stay untouched until the batch has been collected."""
        from . import frontend
        n = len(frames)
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
        arr = (YuvImage * n)()
        keep = []
        for i, (f, fm, mx, rg) in enumerate(zip(frames, per(fmt), per(matrix), per(range))):
            if isinstance(f, YuvImage):
                arr[i] = f
                continue
            if on_device:
                raise ValueError("submit_yuv_images: a device-resident frame is given as a YuvImage (frontend.yuv_image)")
            want = np.uint16 if YUV_LAYOUTS[fm][2] == 2 else np.uint8
            planes = [p if p.dtype == want and p.ndim == 2 and p.strides[1] == p.itemsize else np.ascontiguousarray(p, want) for p in map(np.asarray, f)]
            if len(planes) != YUV_LAYOUTS[fm][1] or any(p.ndim != 2 for p in planes):
                raise ValueError(f"submit_yuv_images: a {fm} frame has {YUV_LAYOUTS[fm][1]} 2-D planes, got {[p.shape for p in planes]}")
            w, h = frontend.yuv_size_of_planes(fm, planes)
            arr[i] = frontend.yuv_image(fm, [p.ctypes.data for p in planes], [p.strides[0] for p in planes], w, h, mx, rg)
            keep.append(planes)
        check(lib().hp_pipeline_submit_yuv_images(self._h, arr, n, int(bool(on_device))))
        self._keep = (keep, frames)

    def submit_yuv_images_raw(self, images, n: int, on_device: bool = False) -> None:
        """Pre-marshalled form for hot loops: ``images`` is a ctypes array of ``YuvImage``."""
        check(lib().hp_pipeline_submit_yuv_images(self._h, images, n, int(bool(on_device))))

    def submit_rgb_images(self, frames, format="bgr24", on_device: bool = False) -> None:
        """Packed RGB, BGRA-family and grey frames (``hp_pipeline_submit_rgb_images``).  A frame is a uint8 array ``[h, w, 3]`` (``format`` "bgr24" or
        "rgb24"), ``[h, w, 4]`` ("bgra", "rgba", "argb", "abgr") or ``[h, w]`` ("gray"); a row-padded view keeps its stride and is not copied - or,
        ready-made, an ``RgbImage`` (``frontend.rgb_image``), which is the only form of a device-resident frame.  ``format`` is one name for the batch
        or one per frame.  The frames go up in their own form and are read by the fused resize: nothing is repacked to BGR.
        ``on_device=True``: ``data`` is a device pointer and nothing is copied; the surfaces must be complete now and stay untouched until the
        batch has been collected."""
        from . import frontend
        n = len(frames)
        fmts = list(format) if isinstance(format, (list, tuple)) else [format] * n
        arr = (RgbImage * n)()
        keep = []
        for i, (f, fm) in enumerate(zip(frames, fmts)):
            if isinstance(f, RgbImage):
                arr[i] = f
                continue
            if on_device:
                raise ValueError("submit_rgb_images: a device-resident frame is given as an RgbImage (frontend.rgb_image)")
            arr[i], a = frontend.rgb_host_image(f, fm)
            keep.append(a)
        check(lib().hp_pipeline_submit_rgb_images(self._h, arr, n, int(bool(on_device))))
        self._keep = (keep, frames)

    def submit_rgb_images_raw(self, images, n: int, on_device: bool = False) -> None:
        """Pre-marshalled form for hot loops: ``images`` is a ctypes array of ``RgbImage``."""
        check(lib().hp_pipeline_submit_rgb_images(self._h, images, n, int(bool(on_device))))

    def collect(self):
        """Humans of the oldest batch in flight: list (per frame) of Human structure arrays."""
        nf = C.c_int(0)
        check(lib().hp_pipeline_collect(self._h, self._out, self.cap, self._n, C.byref(nf)))
        arr = np.frombuffer(self._out, dtype=HUMAN_DTYPE)
        return [arr[i * self.cap: i * self.cap + min(self._n[i], self.cap)].copy() for i in range(nf.value)]
