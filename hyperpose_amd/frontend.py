"""Stream front-end geometry over the C ABI: ``cv::resize`` / ``non_scaling_resize`` on device images and
``resume_ratio`` (reference src/stream.cpp:89-103, src/data.cpp:53-69, include/hyperpose/utility/human.hpp:44-58)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (HDR_DEFAULT_PEAK, HDR_DEFAULT_WHITE, HDR_TRANSFERS, HUMAN_DTYPE, MAPVIEW_ALPHAS, MAPVIEW_MODES, MAPVIEW_PALETTES, MapViewDesc, OVERLAY_PRIM_DTYPE, REDACT_EFFECTS, REDACT_REGION_DTYPE, REDACT_WHAT,
                   TILING_DEFAULT_MIN_COMMON, TILING_DEFAULT_TOL, YUV_FORMATS, YUV_LAYOUTS, YUV_MATRICES, YUV_RANGES, DevBuf, HdrDesc, Human, OverlayPrim,
                   RedactRegion, RGB_LAYOUTS, RgbImage, Roi, Tiling, YuvImage, as_ptr, check, lib)


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


# ---- frames described by hp_yuv_image: every layout, matrix and range (hp_resize_yuv / hp_letterbox_yuv) ----------------------------

def yuv_packed_bytes(fmt: str, w: int, h: int) -> int:
    """``hp_yuv_packed_bytes``: the size of one tightly packed frame, 0 for a size the layout cannot hold."""
    return int(lib().hp_yuv_packed_bytes(YUV_LAYOUTS[fmt][0], int(w), int(h)))


def yuv_coefficients(matrix: str = "bt601", range: str = "limited", depth: int = 8):
    """``hp_yuv_coefficients``: [y_off, c_off, CY, CUB, CUG, CVG, CVR], the table the kernel is given."""
    out = (C.c_int32 * 7)()
    check(lib().hp_yuv_coefficients(YUV_MATRICES[matrix], YUV_RANGES[range], int(depth), out))
    return list(out)


def yuv_plane_shapes(fmt: str, w: int, h: int):
    """[(rows, samples per row)] of the planes of a ``w`` x ``h`` frame; a packed layout's one plane holds 2 * w bytes per row."""
    code, _, sample_bytes, _, _ = YUV_LAYOUTS[fmt]
    out = []
    for k in range(lib().hp_yuv_plane_layout(code, 0, int(w), int(h), None, None)):
        row, rows = C.c_size_t(), C.c_int()
        lib().hp_yuv_plane_layout(code, k, int(w), int(h), C.byref(row), C.byref(rows))
        out.append((rows.value, row.value // sample_bytes))
    return out


def yuv_planes(buffer, fmt: str, w: int, h: int):
    """The planes of one tightly packed frame (a flat buffer of ``yuv_packed_bytes`` bytes) as 2-D views: uint8, or uint16 words for the
    10-bit layouts.  This list of arrays is the host form of a frame in ``resize_yuv_host`` and ``Pipeline.submit_yuv_images``."""
    nbytes = yuv_packed_bytes(fmt, w, h)
    if nbytes == 0:
        raise ValueError(f"yuv_planes: a {fmt} frame cannot be {w} x {h}")
    flat = np.ascontiguousarray(buffer).reshape(-1).view(np.uint8)
    if flat.size != nbytes:
        raise ValueError(f"yuv_planes: a {w} x {h} {fmt} frame has {nbytes} bytes, got {flat.size}")
    dt = np.uint16 if YUV_LAYOUTS[fmt][2] == 2 else np.uint8
    out, at = [], 0
    for rows, cols in yuv_plane_shapes(fmt, w, h):
        n = rows * cols * np.dtype(dt).itemsize
        out.append(flat[at:at + n].view(dt).reshape(rows, cols))
        at += n
    return out


def yuv_image(fmt: str, planes, strides, w: int, h: int, matrix: str = "bt601", range: str = "limited") -> YuvImage:
    """An ``hp_yuv_image`` from plane addresses (ints / c_void_p, host or device) and row strides in bytes."""
    im = YuvImage(YUV_LAYOUTS[fmt][0], YUV_MATRICES[matrix], YUV_RANGES[range], int(w), int(h))
    for k, (p, s) in enumerate(zip(planes, strides)):
        im.plane[k] = p.value if isinstance(p, C.c_void_p) else int(p)
        im.stride[k] = int(s)
    return im


def yuv_size_of_planes(fmt: str, planes):
    """(w, h) of a frame given as its list of 2-D plane arrays."""
    rows, cols = planes[0].shape
    return (cols // 2 if YUV_LAYOUTS[fmt][1] == 1 else cols), rows


def _host_image(frame_planes, fmt: str, matrix: str, range: str, written: bool = False) -> YuvImage:
    """The ``hp_yuv_image`` of a frame in HOST memory given as its list of 2-D plane arrays: rows may be padded (views of wider arrays),
    samples must be contiguous within a row; ``written``: the call paints into the planes."""
    for p in frame_planes:
        assert p.ndim == 2 and p.strides[1] == p.itemsize and (p.flags.writeable or not written)
    w, h = yuv_size_of_planes(fmt, frame_planes)
    return yuv_image(fmt, [p.ctypes.data for p in frame_planes], [p.strides[0] for p in frame_planes], w, h, matrix, range)


def _host_bgr(frame):
    """(address, w, h, stride in bytes) of a writeable uint8 [h, w, 3] frame in HOST memory whose rows may be padded"""
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and frame.strides[1:] == (3, 1) and frame.flags.writeable
    return C.c_void_p(frame.ctypes.data), frame.shape[1], frame.shape[0], frame.strides[0]


class _Handle:
    """One handle of the C ABI: ``self.h`` is made by ``hp_<NAME>_create(&h, *args)`` and given back to ``hp_<NAME>_destroy`` by ``close``
    or when the object is collected."""
    NAME = ""

    def __init__(self, *args):
        self.h = C.c_void_p()
        check(getattr(lib(), f"hp_{self.NAME}_create")(C.byref(self.h), *args))

    def close(self):
        if self.h:
            getattr(lib(), f"hp_{self.NAME}_destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_handles = {}


def _default_handle(cls, floor: int, n: int):
    """This module's own handle of class ``cls`` (an ``Overlay``, a ``Redactor``), made anew when a call brings more than it holds"""
    held = _default_handles.get(cls)
    if held is None or held[1] < n:
        cap = max(floor, n)
        held = _default_handles[cls] = (cls(cap), cap)
    return held[0]


def yuv_upload(planes, fmt: str, pitch=0, fill: int = 0xA5):
    """Device copy of a frame's planes, each in a ``DevBuf`` of its own with rows ``pitch`` bytes longer than the picture's (the padding
    holds ``fill``), as a decoder surface has them; ``pitch`` is one number or one per plane (the U and the V plane of a planar frame may
    differ).  Returns (bufs, strides in bytes)."""
    bufs, strides = [], []
    pitches = list(pitch) if isinstance(pitch, (list, tuple)) else [pitch] * len(planes)
    for p, extra in zip(planes, pitches):
        p = np.ascontiguousarray(p)
        row = p.shape[1] * p.itemsize
        padded = np.full((p.shape[0], row + extra), fill, np.uint8)
        padded[:, :row] = p.view(np.uint8).reshape(p.shape[0], row)
        bufs.append(DevBuf.from_numpy(padded))
        strides.append(row + extra)
    return bufs, strides


def resize_yuv(im: YuvImage, dst_dev, dw: int, dh: int, keep_ratio: bool = False, bgcolor=(0, 0, 0), stream=None, dst_stride=None, tonemap=None) -> None:
    """``hp_resize_yuv`` / ``hp_letterbox_yuv`` on an image whose planes are in device memory; with ``tonemap`` (a ``Tonemap``) their HDR twins
    ``hp_resize_yuv_hdr`` / ``hp_letterbox_yuv_hdr``: the frame is PQ / HLG P010 or I010."""
    s = C.c_void_p(stream) if stream else None
    L, tm = lib(), ([tonemap.h] if tonemap is not None else [])
    if keep_ratio:
        call = L.hp_letterbox_yuv_hdr if tm else L.hp_letterbox_yuv
        check(call(C.byref(im), *tm, as_ptr(dst_dev), dw, dh, dst_stride or dw * 3, int(bgcolor[0]), int(bgcolor[1]), int(bgcolor[2]), s))
    else:
        check((L.hp_resize_yuv_hdr if tm else L.hp_resize_yuv)(C.byref(im), *tm, as_ptr(dst_dev), dw, dh, dst_stride or dw * 3, s))


def resize_yuv_host(frame_planes, dw: int, dh: int, fmt: str = "nv12", matrix: str = "bt601", range: str = "limited", keep_ratio: bool = False,
                    bgcolor=(0, 0, 0), pitch=0, tonemap=None) -> np.ndarray:
    """Convenience for tests: a host frame (its list of 2-D plane arrays, see ``yuv_planes``) -> device -> converted + resized -> host.
    ``pitch`` > 0 pads every plane row by that many bytes on the device."""
    w, h = yuv_size_of_planes(fmt, frame_planes)
    bufs, strides = yuv_upload(frame_planes, fmt, pitch)
    dst = DevBuf(dw * dh * 3)
    resize_yuv(yuv_image(fmt, [b.ptr for b in bufs], strides, w, h, matrix, range), dst, dw, dh, keep_ratio, bgcolor, tonemap=tonemap)
    check(lib().hp_device_synchronize())
    return dst.to_numpy(np.uint8, (dh, dw, 3))


# ---- HDR video in: PQ / HLG 10-bit frames tone-mapped inside the fused resize (include/hp_hip.h; the rule: csrc/tonemap.hpp) -----

def hdr_desc(transfer: str = "pq", to_bt709: bool = True, peak_nits: float = HDR_DEFAULT_PEAK, white_nits: float = HDR_DEFAULT_WHITE) -> HdrDesc:
    """An ``hp_hdr_desc``; ``transfer`` is "pq" or "hlg" (or the raw code, for tests of the refusals)."""
    return HdrDesc(HDR_TRANSFERS.get(transfer, transfer), int(bool(to_bt709)), float(peak_nits), float(white_nits))


def tonemap_tables(transfer: str = "pq", to_bt709: bool = True, peak_nits: float = HDR_DEFAULT_PEAK, white_nits: float = HDR_DEFAULT_WHITE):
    """``hp_tonemap_tables``: (A uint16 [1024], M int32 [3, 3], O uint8 [4096]), the tables every pixel of an HDR frame goes through."""
    d = hdr_desc(transfer, to_bt709, peak_nits, white_nits)
    lin, m, out = np.zeros(1024, np.uint16), np.zeros((3, 3), np.int32), np.zeros(4096, np.uint8)
    check(lib().hp_tonemap_tables(C.byref(d), lin.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return lin, m, out


class Tonemap(_Handle):
    """``hp_tonemap``: the tables of one description in device memory, what ``resize_yuv(..., tonemap=)`` and ``resize_rois(..., tonemap=)`` take."""
    NAME = "tonemap"

    def __init__(self, transfer: str = "pq", to_bt709: bool = True, peak_nits: float = HDR_DEFAULT_PEAK, white_nits: float = HDR_DEFAULT_WHITE):
        self.desc = hdr_desc(transfer, to_bt709, peak_nits, white_nits)
        super().__init__(C.byref(self.desc))


def tonemap_host(frame_planes, fmt: str, matrix: str = "bt2020", range: str = "limited", transfer: str = "pq", to_bt709: bool = True,
                 peak_nits: float = HDR_DEFAULT_PEAK, white_nits: float = HDR_DEFAULT_WHITE) -> np.ndarray:
    """``hp_tonemap_convert_host``: a P010 / I010 frame in host memory (its list of 2-D plane arrays; rows may be padded) -> [h, w, 3] uint8 BGR,
    no device needed."""
    im = _host_image(frame_planes, fmt, matrix, range)
    d = hdr_desc(transfer, to_bt709, peak_nits, white_nits)
    out = np.empty((im.height, im.width, 3), np.uint8)
    check(lib().hp_tonemap_convert_host(C.byref(im), C.byref(d), out.ctypes.data_as(C.c_void_p), im.width * 3))
    return out


def yuv_colours_hdr(matrix: str = "bt2020", range: str = "limited", transfer: str = "pq", to_bt709: bool = True,
                    peak_nits: float = HDR_DEFAULT_PEAK, white_nits: float = HDR_DEFAULT_WHITE) -> np.ndarray:
    """``hp_yuv_colours_hdr``: the 19 skeleton colours as 10-bit (Y, U, V) of a PQ / HLG frame, graphics white at ``white_nits``; int32 [19, 3]."""
    d = hdr_desc(transfer, to_bt709, peak_nits, white_nits)
    out = np.zeros((19, 3), np.int32)
    check(lib().hp_yuv_colours_hdr(YUV_MATRICES[matrix], YUV_RANGES[range], C.byref(d), out.ctypes.data_as(C.c_void_p)))
    return out


# ---- upright input: stored frames that are turned and / or mirrored (HP_ORIENT_* in include/hp_hip.h; DESIGN.md 1.1 "Orientation") -------------

def oriented_size(orientation: int, sw: int, sh: int):
    """``hp_oriented_size``: (uw, uh) of the upright frame of a stored ``sw`` x ``sh`` frame."""
    uw, uh = C.c_int(), C.c_int()
    check(lib().hp_oriented_size(int(orientation), int(sw), int(sh), C.byref(uw), C.byref(uh)))
    return uw.value, uh.value


def orientation_from_exif(exif: int) -> int:
    """``hp_orientation_from_exif``: the HP_ORIENT_* code of EXIF orientation 1 .. 8."""
    return check(lib().hp_orientation_from_exif(int(exif)))


def orient_roi(roi, orientation: int, sw: int, sh: int):
    """``hp_orient_roi``: the stored rectangle (x, y, w, h) an upright region covers."""
    u, st = Roi(*[int(v) for v in roi]), Roi()
    check(lib().hp_orient_roi(C.byref(u), int(orientation), int(sw), int(sh), C.byref(st)))
    return st.x, st.y, st.w, st.h


def orient_host(img: np.ndarray, orientation: int, dst_pitch: int = 0) -> np.ndarray:
    """``hp_orient_u8c3_host``: the materialised upright frame of a stored [h, w, 3] uint8 BGR image (rows may be padded: a view of a wider
    array), no device needed.  ``dst_pitch`` > 0 pads the result's rows by that many bytes (returned as a view of the padded array)."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.strides[1:] == (3, 1)
    sh, sw = img.shape[:2]
    uw, uh = oriented_size(orientation, sw, sh)
    out = np.full((uh, uw * 3 + int(dst_pitch)), 0xA5, np.uint8)
    check(lib().hp_orient_u8c3_host(C.c_void_p(img.ctypes.data), sw, sh, img.strides[0], int(orientation), C.c_void_p(out.ctypes.data), out.strides[0]))
    return out[:, :uw * 3].reshape(uh, uw, 3)


def humans_orient(humans, orientation: int, to_stored: bool) -> np.ndarray:
    """``hp_humans_orient`` on a copy: humans normalised to the upright frame -> to the stored frame (``to_stored``), or back."""
    hs = _humans(humans).copy()
    check(lib().hp_humans_orient(hs.ctypes.data_as(C.POINTER(Human)), len(hs), int(orientation), int(bool(to_stored))))
    return hs


def resize_oriented(src, dst_dev, dw: int, dh: int, orientation: int, keep_ratio: bool = False, bgcolor=(0, 0, 0), sw=None, sh=None, src_stride=None,
                    dst_stride=None, stream=None, tonemap=None) -> None:
    """``hp_resize_oriented_u8c3`` / ``hp_resize_oriented_yuv``: a STORED device frame - 8-bit BGR (``src`` a device buffer, with ``sw``, ``sh`` as
    stored and optionally ``src_stride``) or a ``YuvImage`` with device planes (with ``tonemap`` a PQ / HLG frame) - read upright and resized
    (letterboxed with ``bgcolor`` when ``keep_ratio``) to ``dw`` x ``dh``."""
    s = C.c_void_p(stream) if stream else None
    bg = [int(c) for c in bgcolor]
    if isinstance(src, YuvImage):
        check(lib().hp_resize_oriented_yuv(C.byref(src), tonemap.h if tonemap is not None else None, int(orientation), int(bool(keep_ratio)), bg[0], bg[1],
                                           bg[2], as_ptr(dst_dev), int(dw), int(dh), int(dst_stride or dw * 3), s))
    else:
        check(lib().hp_resize_oriented_u8c3(as_ptr(src), int(sw), int(sh), int(src_stride or sw * 3), int(orientation), int(bool(keep_ratio)), bg[0], bg[1],
                                            bg[2], as_ptr(dst_dev), int(dw), int(dh), int(dst_stride or dw * 3), s))


# ---- packed RGB and grey frames: hp_rgb_image, its host twin and the fused resize (include/hp_hip.h, "packed RGB and grey frames") -------------

def rgb_image(fmt: str, data, w: int, h: int, stride=None) -> RgbImage:
    """An ``hp_rgb_image``: ``data`` an address (host or device; a ``DevBuf`` or tensor works), ``stride`` the row pitch in bytes (default: tight)."""
    return RgbImage(RGB_LAYOUTS[fmt][0], int(w), int(h), as_ptr(data), int(stride if stride is not None else w * RGB_LAYOUTS[fmt][1]))


def rgb_host_image(frame, fmt: str):
    """(``RgbImage``, the array it points into) of a host frame ``[h, w, 3]``, ``[h, w, 4]`` or ``[h, w]`` uint8; a view whose pixels are contiguous
    keeps its row stride and is not copied."""
    pb = RGB_LAYOUTS[fmt][1]
    a = np.asarray(frame)
    shape_ok = a.ndim == 2 if pb == 1 else a.ndim == 3 and a.shape[2] == pb
    if not shape_ok:
        raise ValueError(f"a {fmt} frame is a {'[h, w]' if pb == 1 else f'[h, w, {pb}]'} uint8 array, got shape {a.shape}")
    if a.dtype != np.uint8 or a.strides[1] != pb or (pb > 1 and a.strides[2] != 1) or a.strides[0] < a.shape[1] * pb:
        a = np.ascontiguousarray(a, np.uint8)
    return RgbImage(RGB_LAYOUTS[fmt][0], a.shape[1], a.shape[0], a.ctypes.data, a.strides[0]), a


def rgb_pixel_bytes(fmt: str) -> int:
    return int(lib().hp_rgb_pixel_bytes(RGB_LAYOUTS[fmt][0]))


def rgb_packed_bytes(fmt: str, w: int, h: int) -> int:
    """``hp_rgb_packed_bytes``: bytes of one tightly packed frame; 0 for an invalid size."""
    return int(lib().hp_rgb_packed_bytes(RGB_LAYOUTS[fmt][0], int(w), int(h)))


def rgb_to_bgr_host(frame, fmt: str = "bgra", pitch: int = 0, fill: int = 0) -> np.ndarray:
    """``hp_rgb_to_bgr_host``: a host frame (array or ``RgbImage``) as 8-bit BGR ``[h, w, 3]`` - the definition of what every RGB feed computes.
    With ``pitch`` the result is a view into rows of ``pitch`` bytes pre-filled with ``fill`` (``.base`` shows that the padding was not written)."""
    im, keep = (frame, None) if isinstance(frame, RgbImage) else rgb_host_image(frame, fmt)  # (keep: the array the description points into)
    w, h = im.width, im.height
    stride = int(pitch or w * 3)
    buf = np.full((max(h, 0), max(stride, 0)), fill, np.uint8)
    check(lib().hp_rgb_to_bgr_host(C.byref(im), buf.ctypes.data_as(C.c_void_p), stride))
    return np.ndarray((h, w, 3), np.uint8, buffer=buf, strides=(stride, 3, 1))


def resize_rgb(im: RgbImage, dst_dev, dw: int, dh: int, orientation: int = 0, keep_ratio: bool = False, bgcolor=(0, 0, 0), dst_stride=None,
               stream=None) -> None:
    """``hp_resize_rgb``: a STORED device frame of any ``hp_rgb_image`` layout read upright and resized (letterboxed with ``bgcolor`` when
    ``keep_ratio``) to 8-bit BGR ``dw`` x ``dh``: the bytes of ``resize_oriented`` on ``rgb_to_bgr_host`` of the frame."""
    bg = [int(c) for c in bgcolor]
    check(lib().hp_resize_rgb(C.byref(im), int(orientation), int(bool(keep_ratio)), bg[0], bg[1], bg[2], as_ptr(dst_dev), int(dw), int(dh),
                              int(dst_stride or dw * 3), C.c_void_p(stream) if stream else None))


def resize_rois_rgb(im: RgbImage, rois, dst_dev, dw: int, dh: int, orientation: int = 0, keep_ratio: bool = False, bgcolor=(0, 0, 0), dst_stride=None,
                    slot_stride=None, stream=None) -> None:
    """``hp_resize_rois_rgb``: the UPRIGHT regions ``rois`` [(x, y, w, h)] of one stored device frame to ``len(rois)`` slots of ``dst_dev``."""
    arr, n = _rois(rois)
    ds = int(dst_stride or dw * 3)
    ss = C.c_size_t(int(slot_stride if slot_stride is not None else ds * dh))
    bg = [int(c) for c in bgcolor]
    check(lib().hp_resize_rois_rgb(C.byref(im), int(orientation), arr, n, int(bool(keep_ratio)), bg[0], bg[1], bg[2], as_ptr(dst_dev), int(dw), int(dh),
                                   ds, ss, C.c_void_p(stream) if stream else None))


def resize_rgb_host(frame, dw: int, dh: int, fmt: str = "bgra", orientation: int = 0, keep_ratio: bool = False, bgcolor=(0, 0, 0)) -> np.ndarray:
    """Convenience for tests, like ``resize_host``: host frame -> device (tightly packed) -> ``resize_rgb`` -> host ``[dh, dw, 3]``."""
    a = np.ascontiguousarray(frame, np.uint8)
    src = DevBuf.from_numpy(a)
    dst = DevBuf(dw * dh * 3)
    resize_rgb(rgb_image(fmt, src, a.shape[1], a.shape[0]), dst, dw, dh, orientation, keep_ratio, bgcolor)
    check(lib().hp_device_synchronize())
    return dst.to_numpy(np.uint8, (dh, dw, 3))


# ---- encoder hand-off: RGB / grey frames to every YUV layout (hp_rgb_to_yuv; the rule: csrc/to_yuv.hpp, DESIGN.md 1.1 "Encoder hand-off") -----------

def yuv_forward_coefficients(matrix: str = "bt601", range: str = "limited", depth: int = 8):
    """``hp_yuv_forward_coefficients``: [y_off, c_off, YR, YG, YB, UR, UG, UB, VR, VG, VB], multiples of 2^-18."""
    out = (C.c_int32 * 11)()
    check(lib().hp_yuv_forward_coefficients(YUV_MATRICES[matrix], YUV_RANGES[range], int(depth), out))
    return list(out)


def yuv_padded_size(fmt: str, w: int, h: int, align: int = 1):
    """``hp_yuv_padded_size``: the smallest (w, h) at least as large whose sides are multiples of ``align`` and of what the layout needs."""
    pw, ph = C.c_int(), C.c_int()
    check(lib().hp_yuv_padded_size(YUV_LAYOUTS[fmt][0], int(w), int(h), int(align), C.byref(pw), C.byref(ph)))
    return pw.value, ph.value


def rgb_to_yuv(im: RgbImage, dst: YuvImage, stream=None) -> None:
    """``hp_rgb_to_yuv``: a device frame of any ``hp_rgb_image`` layout written into the device planes of ``dst`` in its layout, matrix, range and
    bit depth; ``dst`` may be larger than ``im`` (edge replication).  Only enqueues; the annotators take ``dst`` as they take a decoder's surface."""
    check(lib().hp_rgb_to_yuv(C.byref(im), C.byref(dst), C.c_void_p(stream) if stream else None))


def rgb_to_yuv_host(frame, fmt_rgb: str = "bgra", yuv_fmt: str = "nv12", matrix: str = "bt709", range: str = "limited", pad_to=None, pitch=0,
                    fill: int = 0xA5):
    """``hp_rgb_to_yuv_host``: a host frame (array or ``RgbImage``) as the list of 2-D plane arrays of a ``yuv_fmt`` frame - the definition of what
    ``rgb_to_yuv`` computes.  ``pad_to``: None (the smallest size the layout holds), an alignment (``yuv_padded_size``) or the output's (w, h).
    With ``pitch`` (one number or one per plane) every plane is a view into rows that many bytes longer, pre-filled with ``fill`` (``.base`` shows
    that the padding was not written)."""
    im, keep = (frame, None) if isinstance(frame, RgbImage) else rgb_host_image(frame, fmt_rgb)  # (keep: the array the description points into)
    w, h = pad_to if isinstance(pad_to, (tuple, list)) else yuv_padded_size(yuv_fmt, im.width, im.height, pad_to or 1)
    shapes = yuv_plane_shapes(yuv_fmt, w, h)
    if not shapes or shapes[0][0] == 0:
        raise ValueError(f"rgb_to_yuv_host: a {yuv_fmt} frame cannot be {w} x {h}")
    dt = np.dtype(np.uint16 if YUV_LAYOUTS[yuv_fmt][2] == 2 else np.uint8)
    pitches = list(pitch) if isinstance(pitch, (list, tuple)) else [pitch] * len(shapes)
    planes = []
    for (rows, cols), extra in zip(shapes, pitches):
        stride = cols * dt.itemsize + int(extra)
        buf = np.full((rows, stride), fill, np.uint8)
        planes.append(np.ndarray((rows, cols), dt, buffer=buf, strides=(stride, dt.itemsize)))
    dst = _host_image(planes, yuv_fmt, matrix, range, written=True)
    dst.width, dst.height = int(w), int(h)
    check(lib().hp_rgb_to_yuv_host(C.byref(im), C.byref(dst)))
    return planes


# ---- flip ensemble: the frame flip, the map merge and the COCO tables (include/hp_hip.h; the definition: csrc/flip_ensemble.hpp) ---------------

def flip_tables_coco(conf_channels: int = 19):
    """``hp_flip_tables_coco``: (conf_perm int32 [conf_channels], paf_perm int32 [38], paf_sign int8 [38]) of a COCO PAF network."""
    conf = np.zeros(max(1, int(conf_channels)), np.int32)
    perm, sign = np.zeros(38, np.int32), np.zeros(38, np.int8)
    check(lib().hp_flip_tables_coco(int(conf_channels), conf.ctypes.data_as(C.POINTER(C.c_int32)), perm.ctypes.data_as(C.POINTER(C.c_int32)),
                                    sign.ctypes.data_as(C.POINTER(C.c_int8))))
    return conf[:conf_channels], perm, sign


def hflip_u8c3(src_dev, dst_dev, w: int, h: int, n: int = 1, stream=None) -> None:
    """``hp_hflip_u8c3``: ``n`` packed u8 HWC device frames flipped left-right into ``dst_dev`` (no overlap); only enqueues."""
    check(lib().hp_hflip_u8c3(as_ptr(src_dev), as_ptr(dst_dev), int(w), int(h), int(n), C.c_void_p(stream) if stream else None))


def hflip_u8c3_host(frames: np.ndarray) -> np.ndarray:
    """``hp_hflip_u8c3_host``: [n, h, w, 3] (or [h, w, 3]) uint8 -> the flipped frames, no device needed."""
    src = np.ascontiguousarray(frames, np.uint8)
    assert src.ndim in (3, 4) and src.shape[-1] == 3
    h, w = src.shape[-3], src.shape[-2]
    out = np.empty_like(src)
    check(lib().hp_hflip_u8c3_host(C.c_void_p(src.ctypes.data), C.c_void_p(out.ctypes.data), w, h, src.shape[0] if src.ndim == 4 else 1))
    return out


def _flip_tables(perm, sign):
    p, s = np.ascontiguousarray(perm, np.int32).ravel(), np.ascontiguousarray(sign, np.int8).ravel()
    return p, s, p.ctypes.data_as(C.POINTER(C.c_int32)), s.ctypes.data_as(C.POINTER(C.c_int8))


def flip_merge(maps_dev, n: int, C_: int, H: int, W: int, perm, sign, stream=None) -> None:
    """``hp_flip_merge``: device maps [>= 2n, C, H, W] fp32; maps [0, n) become 0.5 * (a +- b), in place; only enqueues.  ``perm`` and
    ``sign`` are passed as they are (C entries expected), so that the refusals can be tested."""
    p, s, pp, sp = _flip_tables(perm, sign)
    check(lib().hp_flip_merge(as_ptr(maps_dev), int(n), int(C_), int(H), int(W), pp, sp, C.c_void_p(stream) if stream else None))


def flip_merge_host(maps: np.ndarray, n: int, perm, sign, shape=None) -> np.ndarray:
    """``hp_flip_merge_host`` on a copy of ``maps`` [>= 2n, C, H, W] float32: the whole array back, maps [0, n) merged.  ``shape`` = (C, H, W)
    overrides the array's (tests of the refusals)."""
    out = np.array(maps, np.float32, order="C", copy=True)
    Cc, H, W = shape if shape is not None else out.shape[1:]
    p, s, pp, sp = _flip_tables(perm, sign)
    check(lib().hp_flip_merge_host(out.ctypes.data_as(C.POINTER(C.c_float)), int(n), int(Cc), int(H), int(W), pp, sp))
    return out


# ---- scale ensemble: the shrunken slots, the bicubic tables and the map merge (include/hp_hip.h; the definition: csrc/scale_ensemble.hpp) ------

def _scales(scales):
    s = np.ascontiguousarray(scales, np.float32).ravel()
    return s, len(s), s.ctypes.data_as(C.POINTER(C.c_float))


def scale_tables(W: int, mw: int):
    """``hp_scale_tables``: (idx int32 [W, 4], wgt float32 [W, 4]), the bicubic taps from ``mw`` valid columns to ``W``."""
    idx, wgt = np.zeros((max(1, int(W)), 4), np.int32), np.zeros((max(1, int(W)), 4), np.float32)
    check(lib().hp_scale_tables(int(W), int(mw), idx.ctypes.data_as(C.c_void_p), wgt.ctypes.data_as(C.c_void_p)))
    return idx[:W], wgt[:W]


def scale_stage(src_dev, dst_dev, w: int, h: int, n: int, map_w: int, map_h: int, scales, bgcolor=(0, 0, 0), stream=None) -> None:
    """``hp_scale_stage_u8c3``: ``n`` packed network-sized u8 HWC device slots -> the ``len(scales) * n`` shrunken slots of ``dst_dev``, scale-major;
    only enqueues."""
    s, k, sp = _scales(scales)
    check(lib().hp_scale_stage_u8c3(as_ptr(src_dev), as_ptr(dst_dev), int(w), int(h), int(n), int(map_w), int(map_h), sp, k, int(bgcolor[0]),
                                    int(bgcolor[1]), int(bgcolor[2]), C.c_void_p(stream) if stream else None))


def scale_stage_host(slots: np.ndarray, map_w: int, map_h: int, scales, bgcolor=(0, 0, 0)) -> np.ndarray:
    """``hp_scale_stage_u8c3_host``: [n, h, w, 3] uint8 network-sized slots -> [len(scales) * n, h, w, 3], no device needed."""
    src = np.ascontiguousarray(slots, np.uint8)
    assert src.ndim == 4 and src.shape[-1] == 3
    n, h, w = src.shape[:3]
    s, k, sp = _scales(scales)
    out = np.zeros((max(1, k) * n, h, w, 3), np.uint8)
    check(lib().hp_scale_stage_u8c3_host(C.c_void_p(src.ctypes.data), C.c_void_p(out.ctypes.data), w, h, n, int(map_w), int(map_h), sp, k,
                                         int(bgcolor[0]), int(bgcolor[1]), int(bgcolor[2])))
    return out


def scale_merge(maps_dev, n: int, K: int, C_: int, H: int, W: int, scales, stream=None) -> None:
    """``hp_scale_merge``: device maps [>= K * n, C, H, W] fp32, scale-major; maps [0, n) become the ensemble, in place; only enqueues (after the
    first call of a geometry, which uploads its tables).  ``scales`` is passed as it is (K - 1 entries expected), so that the refusals can be tested."""
    s, _, sp = _scales(scales)
    check(lib().hp_scale_merge(as_ptr(maps_dev), int(n), int(K), int(C_), int(H), int(W), sp, C.c_void_p(stream) if stream else None))


def scale_merge_host(maps: np.ndarray, n: int, scales, K=None, shape=None) -> np.ndarray:
    """``hp_scale_merge_host`` on a copy of ``maps`` [>= K * n, C, H, W] float32: the whole array back, maps [0, n) merged.  ``K`` defaults to
    ``len(scales) + 1``; ``shape`` = (C, H, W) overrides the array's (tests of the refusals)."""
    out = np.array(maps, np.float32, order="C", copy=True)
    Cc, H, W = shape if shape is not None else out.shape[1:]
    s, k, sp = _scales(scales)
    check(lib().hp_scale_merge_host(out.ctypes.data_as(C.POINTER(C.c_float)), int(n), int(k + 1 if K is None else K), int(Cc), int(H), int(W), sp))
    return out


# ---- regions and tiles: many regions of one frame per launch, the tile planner, the way back and the merge (include/hp_hip.h) -----------

def _rois(rois):
    rois = [tuple(int(v) for v in r) for r in rois]
    return (Roi * max(1, len(rois)))(*[Roi(*r) for r in rois]), len(rois)


def yuv_roi_alignment(fmt: str):
    """``hp_yuv_roi_alignment``: (ax, ay) a region's x / w and y / h must be multiples of in this layout."""
    ax, ay = C.c_int(), C.c_int()
    check(lib().hp_yuv_roi_alignment(YUV_LAYOUTS[fmt][0], C.byref(ax), C.byref(ay)))
    return ax.value, ay.value


def resize_rois(src, rois, dst_dev, dw: int, dh: int, keep_ratio: bool = False, bgcolor=(0, 0, 0), sw=None, sh=None, src_stride=None,
                dst_stride=None, slot_stride=None, stream=None, tonemap=None, orientation=None) -> None:
    """``hp_resize_rois_u8c3`` / ``hp_resize_rois_yuv``: the regions ``rois`` [(x, y, w, h)] of ONE device frame - 8-bit BGR (``src`` a device
    buffer, with ``sw``, ``sh`` and optionally ``src_stride``) or a ``YuvImage`` with device planes - to ``len(rois)`` slots of ``dst_dev``,
    slot i at byte ``i * slot_stride`` (default: slots back to back), each what ``resize`` / ``letterbox`` give on the cut-out region."""
    arr, n = _rois(rois)
    ds = int(dst_stride or dw * 3)
    ss = C.c_size_t(int(slot_stride if slot_stride is not None else ds * dh))
    s = C.c_void_p(stream) if stream else None
    bg = [int(c) for c in bgcolor]
    if orientation is not None:  # ``hp_resize_rois_oriented_*``: a stored frame (``sw`` x ``sh`` as stored), ``rois`` in UPRIGHT coordinates
        if isinstance(src, YuvImage):
            check(lib().hp_resize_rois_oriented_yuv(C.byref(src), tonemap.h if tonemap is not None else None, int(orientation), arr, n,
                                                    int(bool(keep_ratio)), bg[0], bg[1], bg[2], as_ptr(dst_dev), int(dw), int(dh), ds, ss, s))
        else:
            check(lib().hp_resize_rois_oriented_u8c3(as_ptr(src), int(sw), int(sh), int(src_stride or sw * 3), int(orientation), arr, n,
                                                     int(bool(keep_ratio)), bg[0], bg[1], bg[2], as_ptr(dst_dev), int(dw), int(dh), ds, ss, s))
        return
    if isinstance(src, YuvImage) and tonemap is not None:  # a PQ / HLG P010 or I010 frame
        check(lib().hp_resize_rois_yuv_hdr(C.byref(src), tonemap.h, arr, n, int(bool(keep_ratio)), bg[0], bg[1], bg[2], as_ptr(dst_dev), int(dw), int(dh),
                                           ds, ss, s))
    elif isinstance(src, YuvImage):
        check(lib().hp_resize_rois_yuv(C.byref(src), arr, n, int(bool(keep_ratio)), bg[0], bg[1], bg[2], as_ptr(dst_dev), int(dw), int(dh), ds, ss, s))
    else:
        check(lib().hp_resize_rois_u8c3(as_ptr(src), int(sw), int(sh), int(src_stride or sw * 3), arr, n, int(bool(keep_ratio)), bg[0], bg[1], bg[2],
                                        as_ptr(dst_dev), int(dw), int(dh), ds, ss, s))


def tiling(cols: int, rows: int, overlap=(0, 0), with_full: bool = False, min_common: int = TILING_DEFAULT_MIN_COMMON,
           tol: float = TILING_DEFAULT_TOL) -> Tiling:
    """An ``hp_tiling``; ``overlap`` is one number or (ox, oy)."""
    ox, oy = overlap if isinstance(overlap, (list, tuple)) else (overlap, overlap)
    return Tiling(int(cols), int(rows), int(ox), int(oy), int(bool(with_full)), int(min_common), float(tol))


def plan_tiles(frame_w: int, frame_h: int, cols: int, rows: int, overlap=(0, 0), with_full: bool = False, fmt=None, align=None, cap: int = 64):
    """``hp_tile_plan``: the regions [(x, y, w, h)] of a frame, the whole frame first when ``with_full``, then the tiles row-major.  ``fmt`` names a
    YUV layout whose alignment the tiles keep (``align`` = (ax, ay) gives it directly; default (1, 1): BGR)."""
    ax, ay = align if align is not None else (yuv_roi_alignment(fmt) if fmt else (1, 1))
    t = tiling(cols, rows, overlap, with_full)
    out = (Roi * max(1, int(cap)))()
    n = check(lib().hp_tile_plan(C.byref(t), int(frame_w), int(frame_h), int(ax), int(ay), out, int(cap)))
    return [(out[i].x, out[i].y, out[i].w, out[i].h) for i in range(n)]


def humans_to_frame(humans, roi, frame_w: int, frame_h: int) -> np.ndarray:
    """``hp_humans_to_frame`` on a copy: humans normalised to the region ``roi`` (x, y, w, h) -> normalised to the frame."""
    hs = _humans(humans).copy()
    r = Roi(*[int(v) for v in roi])
    lib().hp_humans_to_frame(hs.ctypes.data_as(C.POINTER(Human)), len(hs), C.byref(r), int(frame_w), int(frame_h))
    return hs


def merge_humans(humans, region_of, frame_w: int, frame_h: int, min_common: int = TILING_DEFAULT_MIN_COMMON, tol: float = TILING_DEFAULT_TOL,
                 cap=None) -> np.ndarray:
    """``hp_humans_merge``: ``humans`` (frame coordinates) with the region index each came from -> the merged humans, in kept order."""
    hs = _humans(humans)
    reg = np.ascontiguousarray(region_of, np.int32).reshape(-1)
    assert len(reg) == len(hs)
    cap = len(hs) if cap is None else int(cap)
    out = np.zeros(max(1, cap), HUMAN_DTYPE)
    n = check(lib().hp_humans_merge(hs.ctypes.data_as(C.POINTER(Human)), reg.ctypes.data_as(C.POINTER(C.c_int32)), len(hs), int(frame_w), int(frame_h),
                                    int(min_common), C.c_double(tol), out.ctypes.data_as(C.POINTER(Human)), cap))
    return out[:n]


# ---- writing back: skeletons painted into frames (hp_overlay_*; the rules are stated in csrc/overlay.hpp and DESIGN.md 1.1) -------------

def _humans(humans) -> np.ndarray:
    return np.ascontiguousarray(humans, HUMAN_DTYPE).reshape(-1)


def overlay_primitives(humans, w: int, h: int, thickness: int = 0) -> np.ndarray:
    """``hp_overlay_primitives``: the primitive list of a frame's humans (OVERLAY_PRIM_DTYPE records, in painting order)."""
    hs = _humans(humans)
    out = np.zeros(max(1, 37 * len(hs)), OVERLAY_PRIM_DTYPE)
    n = check(lib().hp_overlay_primitives(hs.ctypes.data_as(C.POINTER(Human)), len(hs), int(w), int(h), int(thickness),
                                          out.ctypes.data_as(C.POINTER(OverlayPrim)), len(out)))
    return out[:n]


def yuv_colours(matrix: str = "bt601", range: str = "limited", depth: int = 8) -> np.ndarray:
    """``hp_yuv_colours``: the 19 skeleton colours as ``depth``-bit (Y, U, V), int32 [19, 3]."""
    out = np.zeros((19, 3), np.int32)
    check(lib().hp_yuv_colours(YUV_MATRICES[matrix], YUV_RANGES[range], int(depth), out.ctypes.data_as(C.c_void_p)))
    return out


class Overlay(_Handle):
    """``hp_overlay``: the handle the device entry points draw through (pinned staging slots and device lists for ``max_humans`` per call)."""
    NAME = "overlay"

    def __init__(self, max_humans: int = 64):
        self.max_humans = int(max_humans)
        super().__init__(self.max_humans)

    def set_transfer(self, transfer=None, to_bt709: bool = True, peak_nits: float = HDR_DEFAULT_PEAK, white_nits: float = HDR_DEFAULT_WHITE) -> None:
        """``hp_overlay_set_transfer``: 10-bit frames drawn through this handle are "pq" / "hlg" frames and get ``yuv_colours_hdr``'s colours;
        ``None`` means SDR again."""
        d = None if transfer is None else hdr_desc(transfer, to_bt709, peak_nits, white_nits)
        check(lib().hp_overlay_set_transfer(self.h, C.byref(d) if d is not None else None))


def draw_humans(target, humans, opacity: float = 1.0, thickness: int = 0, w=None, h=None, stride=None, stream=None, overlay=None) -> None:
    """Paint the skeletons of ``humans`` (HUMAN_DTYPE, in the frame's normalised coordinates) into a frame in DEVICE memory, in place and
    stream-ordered: ``target`` is a ``YuvImage`` whose planes are device pointers (``hp_overlay_draw_yuv``) or a device buffer of 8-bit BGR
    with ``w``, ``h`` and optionally ``stride`` in bytes (``hp_overlay_draw_u8c3``)."""
    hs = _humans(humans)
    ov = overlay or _default_handle(Overlay, 64, len(hs))
    hp, s = hs.ctypes.data_as(C.POINTER(Human)), C.c_void_p(stream) if stream else None
    if isinstance(target, YuvImage):
        check(lib().hp_overlay_draw_yuv(ov.h, C.byref(target), hp, len(hs), C.c_float(opacity), int(thickness), s))
    else:
        check(lib().hp_overlay_draw_u8c3(ov.h, as_ptr(target), int(w), int(h), int(stride or w * 3), hp, len(hs), C.c_float(opacity), int(thickness), s))


def draw_humans_host(frame, humans, fmt=None, matrix: str = "bt601", range: str = "limited", opacity: float = 1.0, thickness: int = 0,
                     hdr=None) -> None:
    """The same picture on a frame in HOST memory, in place, no device needed: ``frame`` is a uint8 array [h, w, 3] (BGR, ``fmt`` None) or the
    list of 2-D plane arrays ``yuv_planes`` returns (``fmt`` names the layout).  Rows may be padded (views of wider arrays); samples must be
    contiguous within a row."""
    hs = _humans(humans)
    hp = hs.ctypes.data_as(C.POINTER(Human))
    if fmt is None:
        check(lib().hp_overlay_draw_u8c3_host(*_host_bgr(frame), hp, len(hs), C.c_float(opacity), int(thickness)))
        return
    im = _host_image(frame, fmt, matrix, range, written=True)
    if hdr is not None:  # an ``hdr_desc``: the frame is PQ / HLG (``hp_overlay_draw_yuv_host_hdr``)
        check(lib().hp_overlay_draw_yuv_host_hdr(C.byref(im), C.byref(hdr), hp, len(hs), C.c_float(opacity), int(thickness)))
        return
    check(lib().hp_overlay_draw_yuv_host(C.byref(im), hp, len(hs), C.c_float(opacity), int(thickness)))


# ---- writing back: heads or whole persons made unrecognisable (hp_redact_*; the rules are stated in csrc/redact.hpp and DESIGN.md 1.1) ----

def _regions(regions) -> np.ndarray:
    return np.ascontiguousarray(regions, REDACT_REGION_DTYPE).reshape(-1)


def redact_regions(humans, w: int, h: int, what: str = "head", margin: float = 1.0) -> np.ndarray:
    """``hp_redact_regions``: the regions (REDACT_REGION_DTYPE records, in order) that cover the heads (``what`` "head": one disc per human
    with a face part) or the whole persons ("body": a rectangle, then the head disc) of a ``w`` x ``h`` frame's humans."""
    hs = _humans(humans)
    out = np.zeros(max(1, 2 * len(hs)), REDACT_REGION_DTYPE)
    n = check(lib().hp_redact_regions(hs.ctypes.data_as(C.POINTER(Human)), len(hs), int(w), int(h), REDACT_WHAT[what], C.c_float(margin),
                                      out.ctypes.data_as(C.POINTER(RedactRegion)), len(out)))
    return out[:n]


class Redactor(_Handle):
    """``hp_redact``: the handle the device entry points work through (pinned staging slots and device lists for ``max_regions`` per call)."""
    NAME = "redact"

    def __init__(self, max_regions: int = 128):
        self.max_regions = int(max_regions)
        super().__init__(self.max_regions)


def redact(target, regions, effect: str = "pixelate", cell: int = 16, w=None, h=None, stride=None, stream=None, redactor=None) -> None:
    """Pixelate or black out every ``cell`` x ``cell`` cell that ``regions`` (REDACT_REGION_DTYPE, in the frame's pixels: ``redact_regions`` or the
    caller's own) reach, in a frame in DEVICE memory, in place and stream-ordered: ``target`` is a ``YuvImage`` whose planes are device pointers
    (``hp_redact_yuv``) or a device buffer of 8-bit BGR with ``w``, ``h`` and optionally ``stride`` in bytes (``hp_redact_u8c3``)."""
    rs = _regions(regions)
    rd = redactor or _default_handle(Redactor, 128, len(rs))
    rp, s = rs.ctypes.data_as(C.POINTER(RedactRegion)), C.c_void_p(stream) if stream else None
    if isinstance(target, YuvImage):
        check(lib().hp_redact_yuv(rd.h, C.byref(target), rp, len(rs), REDACT_EFFECTS[effect], int(cell), s))
    else:
        check(lib().hp_redact_u8c3(rd.h, as_ptr(target), int(w), int(h), int(stride or w * 3), rp, len(rs), REDACT_EFFECTS[effect], int(cell), s))


def redact_host(frame, regions, fmt=None, matrix: str = "bt601", range: str = "limited", effect: str = "pixelate", cell: int = 16) -> None:
    """The same picture on a frame in HOST memory, in place, no device needed: ``frame`` is a uint8 array [h, w, 3] (BGR, ``fmt`` None) or the
    list of 2-D plane arrays ``yuv_planes`` returns (``fmt`` names the layout).  Rows may be padded (views of wider arrays); samples must be
    contiguous within a row."""
    rs = _regions(regions)
    rp = rs.ctypes.data_as(C.POINTER(RedactRegion))
    if fmt is None:
        check(lib().hp_redact_u8c3_host(*_host_bgr(frame), rp, len(rs), REDACT_EFFECTS[effect], int(cell)))
        return
    im = _host_image(frame, fmt, matrix, range, written=True)
    check(lib().hp_redact_yuv_host(C.byref(im), rp, len(rs), REDACT_EFFECTS[effect], int(cell)))


# ---- writing back: the network's own maps shown on the frame (hp_mapview_*; the rules are stated in csrc/mapview.hpp and DESIGN.md 1.1) ----

def map_cover(frame_w: int, frame_h: int, in_w: int, in_h: int, keep_ratio: bool = True):
    """``hp_mapview_cover``: (cover_x, cover_y), the fractions of the network's ``in_w`` x ``in_h`` input - and so of the maps' cells - that an
    upright ``frame_w`` x ``frame_h`` frame fills: the letterbox's inner size over the input size, or (1, 1) for a plain resize."""
    out = (C.c_double * 2)()
    check(lib().hp_mapview_cover(int(frame_w), int(frame_h), int(in_w), int(in_h), int(bool(keep_ratio)), out))
    return out[0], out[1]


def map_taps(U: int, m: int, cover: float = 1.0) -> np.ndarray:
    """``hp_mapview_taps``: int32 [U, 3], per upright pixel of an axis the two map cells it samples and the weight (of 2048) of the second."""
    out = np.zeros((max(1, int(U)), 3), np.int32)
    check(lib().hp_mapview_taps(int(U), int(m), C.c_double(cover), out.ctypes.data_as(C.c_void_p)))
    return out[:U]


def map_palette(kind="jet", alpha: str = "constant", matrix=None, range: str = "limited", depth: int = 8) -> np.ndarray:
    """``hp_mapview_palette``: int32 [256, 4], the built-in palette ``kind`` ("jet", "heat", "grey") as (R, G, B, A), A = 255 ("constant") or the
    index ("scaled").  With ``matrix``: the ``depth``-bit (Y, U, V, A) a frame of that matrix and range is painted with
    (``hp_mapview_palette_yuv``); ``kind`` may then also be a caller's own [256, 4] (R, G, B, A) table."""
    if isinstance(kind, str):
        rgba = np.zeros((256, 4), np.int32)
        check(lib().hp_mapview_palette(MAPVIEW_PALETTES[kind], MAPVIEW_ALPHAS[alpha], rgba.ctypes.data_as(C.c_void_p)))
    else:
        rgba = _palette(kind)
    if matrix is None:
        return rgba
    out = np.zeros((256, 4), np.int32)
    check(lib().hp_mapview_palette_yuv(rgba.ctypes.data_as(C.c_void_p), YUV_MATRICES[matrix], YUV_RANGES[range], int(depth), out.ctypes.data_as(C.c_void_p)))
    return out


def _palette(palette) -> np.ndarray:
    p = map_palette(palette) if isinstance(palette, str) else np.ascontiguousarray(palette, np.int32)
    assert p.shape == (256, 4)
    return p


def _map_desc(maps_ptr, shape, frame, mode, channels, gain, cover, orientation, roi) -> MapViewDesc:
    """``hp_mapview_desc``; ``channels`` is (c0, cn, c_step) or None = every channel (every pair, for "field")"""
    C_, mh, mw = (int(v) for v in shape)
    field = MAPVIEW_MODES[mode] == MAPVIEW_MODES["field"]
    c0, cn, step = channels if channels is not None else (0, C_ // 2 if field else C_, 2 if field else 1)
    d = MapViewDesc(maps_ptr, C_, mh, mw, int(frame), int(c0), int(cn), int(step), MAPVIEW_MODES[mode], float(gain), float(cover[0]), float(cover[1]),
                    int(orientation))
    if roi is not None:
        d.roi, d.has_roi = Roi(*(int(v) for v in roi)), 1
    return d


def map_index_host(maps, frame: int = 0, mode: str = "max", channels=None, gain: float = 1.0) -> np.ndarray:
    """``hp_mapview_index_host``: uint8 [mh, mw], the index plane of frame ``frame`` of ``maps`` (float32 [frames, C, mh, mw] in host memory)."""
    maps = np.ascontiguousarray(maps, np.float32)
    assert maps.ndim == 4
    d = _map_desc(maps.ctypes.data, maps.shape[1:], frame, mode, channels, gain, (1.0, 1.0), 0, None)
    out = np.zeros(maps.shape[2:], np.uint8)
    check(lib().hp_mapview_index_host(C.byref(d), out.ctypes.data_as(C.c_void_p)))
    return out


class MapView(_Handle):
    """``hp_mapview``: the handle the device entry points draw through (staging slots for maps of up to ``max_map_cells`` cells)."""
    NAME = "mapview"

    def __init__(self, max_map_cells: int = 1 << 16):
        self.max_map_cells = int(max_map_cells)
        super().__init__(self.max_map_cells)

    def debug_plane(self) -> np.ndarray:
        """``hp_mapview_debug_plane``: the index plane of the last draw call, flat (synchronises the device)"""
        out = np.zeros(self.max_map_cells, np.uint8)
        n = check(lib().hp_mapview_debug_plane(self.h, out.ctypes.data_as(C.c_void_p), len(out)))
        return out[:n]


def draw_maps(target, maps_dev, shape, frame: int = 0, mode: str = "max", palette="jet", opacity: float = 0.5, gain: float = 1.0, channels=None,
              cover=(1.0, 1.0), orientation: int = 0, roi=None, w=None, h=None, stride=None, stream=None, view=None) -> None:
    """Blend the colour-mapped, up-sampled maps of one frame into that frame in DEVICE memory, in place and stream-ordered.  ``maps_dev``: device
    address of fp32 [frames, C, mh, mw] (``Engine.output_device``), ``shape`` = (C, mh, mw); ``mode`` "max" (confidence maps) or "field" (channel
    pairs are vectors: part-affinity fields); ``palette`` a built-in name or an int [256, 4] (R, G, B, A) table; ``channels`` (c0, cn, c_step) or
    None for all; ``cover`` from ``map_cover``; ``roi`` (x, y, w, h) in stored pixels.  ``target`` is a ``YuvImage`` whose planes are device
    pointers (``hp_mapview_draw_yuv``) or a device buffer of 8-bit BGR with ``w``, ``h`` and optionally ``stride`` (``hp_mapview_draw_u8c3``)."""
    d = _map_desc(as_ptr(maps_dev).value, shape, frame, mode, channels, gain, cover, orientation, roi)
    mv = view or _default_handle(MapView, 1 << 16, d.mh * d.mw)
    pal, s = _palette(palette), C.c_void_p(stream) if stream else None
    pp = pal.ctypes.data_as(C.c_void_p)
    if isinstance(target, YuvImage):
        check(lib().hp_mapview_draw_yuv(mv.h, C.byref(target), C.byref(d), pp, C.c_float(opacity), s))
    else:
        check(lib().hp_mapview_draw_u8c3(mv.h, as_ptr(target), int(w), int(h), int(stride or w * 3), C.byref(d), pp, C.c_float(opacity), s))


def draw_maps_host(frame, maps, fmt=None, matrix: str = "bt601", range: str = "limited", index: int = 0, mode: str = "max", palette="jet",
                   opacity: float = 0.5, gain: float = 1.0, channels=None, cover=(1.0, 1.0), orientation: int = 0, roi=None) -> None:
    """The same picture with frame and maps in HOST memory, in place, no device needed: ``frame`` is a uint8 array [h, w, 3] (BGR, ``fmt`` None) or
    the list of 2-D plane arrays ``yuv_planes`` returns; ``maps`` float32 [frames, C, mh, mw], of which frame ``index`` is shown."""
    maps = np.ascontiguousarray(maps, np.float32)
    assert maps.ndim == 4
    d = _map_desc(maps.ctypes.data, maps.shape[1:], index, mode, channels, gain, cover, orientation, roi)
    pp = _palette(palette).ctypes.data_as(C.c_void_p)
    if fmt is None:
        check(lib().hp_mapview_draw_u8c3_host(*_host_bgr(frame), C.byref(d), pp, C.c_float(opacity)))
        return
    im = _host_image(frame, fmt, matrix, range, written=True)
    check(lib().hp_mapview_draw_yuv_host(C.byref(im), C.byref(d), pp, C.c_float(opacity)))
