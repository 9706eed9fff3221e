"""Stream front-end geometry over the C ABI: ``cv::resize`` / ``non_scaling_resize`` on device images and
``resume_ratio`` (reference src/stream.cpp:89-103, src/data.cpp:53-69, include/hyperpose/utility/human.hpp:44-58)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import YUV_FORMATS, DevBuf, as_ptr, check, lib


def resize(src_dev, sw: int, sh: int, dst_dev, dw: int, dh: int, stream=None, src_stride=None, dst_stride=None) -> None:
    check(lib().hp_resize_u8c3(as_ptr(src_dev), sw, sh, src_stride or sw * 3, as_ptr(dst_dev), dw, dh, dst_stride or dw * 3,
                               C.c_void_p(stream) if stream else None))


def letterbox(src_dev, sw: int, sh: int, dst_dev, dw: int, dh: int, bgcolor=(0, 0, 0), stream=None) -> None:
    check(lib().hp_letterbox_u8c3(as_ptr(src_dev), sw, sh, sw * 3, as_ptr(dst_dev), dw, dh, dw * 3, int(bgcolor[0]), int(bgcolor[1]),
                                  int(bgcolor[2]), C.c_void_p(stream) if stream else None))


def _yuv_planes(fmt: str, dev, sw: int, sh: int, y_stride, uv_stride):
    """(format, y, y_stride, u, v, uv_stride) of one contiguous 4:2:0 frame at device address ``dev``: Y plane, then the interleaved UV
    plane (nv12) or the U and the V plane (i420), rows ``y_stride`` / ``uv_stride`` bytes apart."""
    base = as_ptr(dev).value
    ys = y_stride or sw
    uvs = uv_stride or (sw if fmt == "nv12" else sw // 2)
    u = base + ys * sh
    v = u + uvs * (sh // 2) if fmt == "i420" else None
    return YUV_FORMATS[fmt], C.c_void_p(base), ys, C.c_void_p(u), C.c_void_p(v), uvs


def resize_yuv420(src_dev, sw: int, sh: int, dst_dev, dw: int, dh: int, fmt: str = "nv12", stream=None, y_stride=None, uv_stride=None,
                  dst_stride=None) -> None:
    """``hp_resize_yuv420``: a YUV 4:2:0 frame (one contiguous device buffer, see ``_yuv_planes``) -> BGR at (dw, dh), bit-equal to
    cv::cvtColor(COLOR_YUV2BGR_NV12 / _I420) followed by ``resize``."""
    f, y, ys, u, v, uvs = _yuv_planes(fmt, src_dev, sw, sh, y_stride, uv_stride)
    check(lib().hp_resize_yuv420(f, y, ys, u, v, uvs, sw, sh, as_ptr(dst_dev), dw, dh, dst_stride or dw * 3,
                                 C.c_void_p(stream) if stream else None))


def letterbox_yuv420(src_dev, sw: int, sh: int, dst_dev, dw: int, dh: int, fmt: str = "nv12", bgcolor=(0, 0, 0), stream=None,
                     y_stride=None, uv_stride=None) -> None:
    f, y, ys, u, v, uvs = _yuv_planes(fmt, src_dev, sw, sh, y_stride, uv_stride)
    check(lib().hp_letterbox_yuv420(f, y, ys, u, v, uvs, sw, sh, as_ptr(dst_dev), dw, dh, dw * 3, int(bgcolor[0]), int(bgcolor[1]),
                                    int(bgcolor[2]), C.c_void_p(stream) if stream else None))


def letterbox_inner(sw: int, sh: int, dw: int, dh: int):
    iw, ih = C.c_int(), C.c_int()
    lib().hp_letterbox_inner(sw, sh, dw, dh, C.byref(iw), C.byref(ih))
    return iw.value, ih.value


def resize_host(img: np.ndarray, dw: int, dh: int, keep_ratio: bool = False, bgcolor=(0, 0, 0)) -> np.ndarray:
    """Convenience for tests: host image [h, w, 3] u8 -> device -> resized -> host."""
    img = np.ascontiguousarray(img, np.uint8)
    sh, sw, _ = img.shape
    src = DevBuf.from_numpy(img)
    dst = DevBuf(dw * dh * 3)
    (letterbox(src, sw, sh, dst, dw, dh, bgcolor) if keep_ratio else resize(src, sw, sh, dst, dw, dh))
    check(lib().hp_device_synchronize())
    out = np.empty((dh, dw, 3), np.uint8)
    check(lib().hp_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dst.ptr, C.c_size_t(out.nbytes)))
    return out


def resize_yuv420_host(frame: np.ndarray, dw: int, dh: int, fmt: str = "nv12", keep_ratio: bool = False, bgcolor=(0, 0, 0),
                       pitch: int = 0) -> np.ndarray:
    """Convenience for tests: host 4:2:0 frame [h*3/2, w] u8 -> device -> converted + resized -> host.  ``pitch`` > 0 lays the planes out
    with padded rows on the device (luma rows ``w + pitch`` bytes apart, chroma rows likewise), as decoder surfaces do."""
    frame = np.ascontiguousarray(frame, np.uint8)
    sh, sw = frame.shape[0] * 2 // 3, frame.shape[1]
    ys = uvs = None
    if pitch:
        ys = sw + pitch
        uvs = (sw if fmt == "nv12" else sw // 2) + pitch
        luma = np.full((sh, ys), 0xA5, np.uint8)
        luma[:, :sw] = frame[:sh]
        cw = uvs - pitch
        chroma = np.full(((sh // 2) * (1 if fmt == "nv12" else 2), uvs), 0x5A, np.uint8)
        chroma[:, :cw] = frame[sh:].reshape(-1, cw)
        frame = np.concatenate([luma.ravel(), chroma.ravel()])
    src = DevBuf.from_numpy(frame)
    dst = DevBuf(dw * dh * 3)
    if keep_ratio:
        letterbox_yuv420(src, sw, sh, dst, dw, dh, fmt, bgcolor, y_stride=ys, uv_stride=uvs)
    else:
        resize_yuv420(src, sw, sh, dst, dw, dh, fmt, y_stride=ys, uv_stride=uvs)
    check(lib().hp_device_synchronize())
    return dst.to_numpy(np.uint8, (dh, dw, 3))
