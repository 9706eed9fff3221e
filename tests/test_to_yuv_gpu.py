"""GPU: hp_rgb_to_yuv (hyperpose_amd/csrc/to_yuv.hip) against hp_rgb_to_yuv_host, byte for byte over WHOLE destination buffers: device and host
planes are pre-filled with 0xA5, carry padded pitches and trailing guard bytes and are compared in full, so a write outside the samples fails the
comparison; sources carry a pitch and guard bytes of another value, so a read outside a row's pixels changes the result.

The kernel built: a thread owns a run of r = 8 luma pixels, a block spans b = 64 runs = 512 pixels and 4 rows of chroma blocks (8 pixel rows of a
4:2:0 layout, 4 of the others)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import to_yuv_ref as ref  # noqa: E402
from overlay_ref import seeded_humans  # noqa: E402
from test_to_yuv_host import SIZES, dst_size, sizes_of  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402
from hyperpose_amd._lib import HP_ERR_INVALID  # noqa: E402

pytestmark = pytest.mark.gpu
R, B = 8, 512  # run length and a block's span, in luma pixels
FILL, SRC_FILL, GUARD = 0xA5, 0x5A, 32


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.init(0)


class Source:
    """a frame on the device with rows `pad` bytes longer than the picture's and GUARD trailing bytes, all SRC_FILL"""

    def __init__(self, frame, fmt_rgb, pad=8):
        self.frame, self.fmt = frame, fmt_rgb
        h, w = frame.shape[:2]
        pb = ref.RGB[fmt_rgb][0]
        stride = w * pb + pad
        flat = np.full(h * stride + GUARD, SRC_FILL, np.uint8)
        flat[:h * stride].reshape(h, stride)[:, :w * pb] = frame.reshape(h, w * pb)
        self.buf = _lib.DevBuf.from_numpy(flat)
        self.image = frontend.rgb_image(fmt_rgb, self.buf, w, h, stride)
        self.host, self.keep = frontend.rgb_host_image(frame, fmt_rgb)


class Surface:
    """the planes of a w x h frame twice, in host and in device memory: flat byte buffers of `offset` + rows * stride + GUARD bytes, all FILL, the
    plane starting `offset` bytes in; stride = the row's bytes + pitch"""

    def __init__(self, fmt, w, h, matrix="bt709", rng="limited", pitch=6, offset=0):
        self.fmt = fmt
        sb = 2 if ref.LAYOUT[fmt][2] == 10 else 1
        self.hosts, self.bufs, strides = [], [], []
        for rows, cols in frontend.yuv_plane_shapes(fmt, w, h):
            stride = cols * sb + pitch
            self.hosts.append(np.full(offset + rows * stride + GUARD, FILL, np.uint8))
            self.bufs.append(_lib.DevBuf.from_numpy(self.hosts[-1]))
            strides.append(stride)
        self.host_image = frontend.yuv_image(fmt, [a.ctypes.data + offset for a in self.hosts], strides, w, h, matrix, rng)
        self.image = frontend.yuv_image(fmt, [b.ptr.value + offset for b in self.bufs], strides, w, h, matrix, rng)

    def download(self):
        _lib.check(_lib.lib().hp_device_synchronize())
        return [b.to_numpy(np.uint8, a.shape) for a, b in zip(self.hosts, self.bufs)]

    def check(self, what=""):
        for k, (g, a) in enumerate(zip(self.download(), self.hosts)):
            bad = np.argwhere(g != a)
            assert bad.size == 0, f"{what} {self.fmt} plane {k}: {len(bad)} bytes differ, first at byte {bad[0].tolist()}"

    def untouched(self):
        return all(np.all(g == FILL) for g in self.download()) and all(np.all(a == FILL) for a in self.hosts)


def convert_both(src, dst, stream=None):
    _lib.check(_lib.lib().hp_rgb_to_yuv_host(C.byref(src.host), C.byref(dst.host_image)))
    frontend.rgb_to_yuv(src.image, dst.image, stream=stream)


def run_case(frame, fmt_rgb, fmt, size, matrix="bt709", rng="limited", what="", **surface):
    src = Source(frame, fmt_rgb)
    dst = Surface(fmt, *size, matrix, rng, **surface)
    convert_both(src, dst)
    dst.check(f"{what} {fmt_rgb} {frame.shape[1]} x {frame.shape[0]} -> {size}")
    assert any(np.any(a != FILL) for a in dst.hosts)


# ---- the host test's crosses and sizes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ref.YUV_FORMATS)
def test_every_layout_pair_bt709_limited(fmt):
    for n, fmt_rgb in enumerate(ref.RGB_FORMATS):
        for src, dst in sizes_of(fmt):
            run_case(ref.random_frame(100 + n, fmt_rgb, *src), fmt_rgb, fmt, dst_size(fmt, src, dst))
        run_case(ref.extremes_frame(fmt_rgb, 3, 5), fmt_rgb, fmt, ref.padded_size(fmt, 3, 5), what="extremes")


@pytest.mark.parametrize("fmt", ["nv12", "p010", "i444"])
def test_every_matrix_and_range_from_bgra(fmt):
    for matrix in ref.MATRICES:
        for rng in ref.RANGES:
            for src, dst in SIZES[2:]:
                run_case(ref.random_frame(7, "bgra", *src), "bgra", fmt, dst_size(fmt, src, dst), matrix, rng)
            run_case(ref.extremes_frame("bgra", 31, 3), "bgra", fmt, (32, 4), matrix, rng, what="extremes")


# ---- the kernel's own edges: widths around a run and a block, heights around a block's rows ---------------------------------------------------------------

@pytest.mark.parametrize("fmt", ref.YUV_FORMATS)
def test_widths_and_heights_around_a_run_and_a_block(fmt):
    rows = 4 << ref.LAYOUT[fmt][1]  # pixel rows of one block
    for fmt_rgb in ("bgra", "rgb24", "gray"):
        for w in (R - 1, R, R + 1, B + 1):
            for h in (rows - 1, rows, rows + 1):
                run_case(ref.random_frame(w + h, fmt_rgb, w, h), fmt_rgb, fmt, ref.padded_size(fmt, w, h))


@pytest.mark.parametrize("fmt", ref.YUV_FORMATS)
def test_322x182_to_336x192(fmt):
    assert frontend.yuv_padded_size(fmt, 322, 182, 16) == (336, 192)
    for fmt_rgb in ("abgr", "bgr24"):
        run_case(ref.random_frame(9, fmt_rgb, 322, 182), fmt_rgb, fmt, (336, 192))


# ---- alignment: planes off a dword go out sample by sample; a 4-byte source's last run must not be loaded as a vector ----------------------------------

@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_destination_planes_off_a_dword_with_an_odd_stride(fmt, offset):
    for w, h in ((40, 6), (26, 10)):
        for pitch in (3, 7):  # a Y row has an even number of bytes: its stride is odd
            run_case(ref.random_frame(offset, "bgra", w - 1, h - 1), "bgra", fmt, (w, h), pitch=pitch, offset=offset)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_a_4_byte_source_of_width_5(fmt):
    """the run's 32-byte load would cross the row (and, in the last row, the buffer): it goes pixel by pixel and the guard bytes stay unread"""
    frame = ref.random_frame(5, "rgba", 5, 3)
    src = Source(frame, "rgba", pad=0)
    dst = Surface(fmt, 8, 4)
    convert_both(src, dst)
    dst.check("width 5")


# ---- on a stream, and what the annotators make of the result ---------------------------------------------------------------------------------------------

def test_two_calls_on_one_stream_then_draw_humans():
    L = _lib.lib()
    owner = C.c_void_p()  # a stream that is not the default one: a parser's own
    _lib.check(L.hp_paf_create(C.byref(owner), C.c_float(0.05), C.c_float(0.05), -1, -1, 1))
    L.hp_paf_stream.restype = C.c_void_p
    stream = L.hp_paf_stream(owner)
    assert stream
    a, b = Source(ref.random_frame(1, "bgra", 97, 61), "bgra"), Source(ref.random_frame(2, "gray", 97, 61), "gray")
    sa, sb = Surface("nv12", 112, 64, "bt709", "limited"), Surface("p010", 98, 62, "bt2020", "full", pitch=10)
    convert_both(a, sa, stream)
    convert_both(b, sb, stream)
    humans = seeded_humans(3, 2, lo=0.2, hi=0.8)
    ov = frontend.Overlay(4)
    frontend.draw_humans(sa.image, humans, opacity=0.7, stream=stream, overlay=ov)
    before = [h.copy() for h in sa.hosts]
    _lib.check(L.hp_overlay_draw_yuv_host(C.byref(sa.host_image), humans.ctypes.data_as(C.POINTER(_lib.Human)), len(humans), C.c_float(0.7), 0))
    assert any(not np.array_equal(x, y) for x, y in zip(before, sa.hosts))  # something was drawn
    sa.check("nv12 + skeletons")
    sb.check("p010")
    ov.close()
    L.hp_paf_destroy(owner)


# ---- refusals launch nothing ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_destination_untouched():
    L = _lib.lib()
    frame = ref.random_frame(1, "bgra", 6, 4)

    def refused(src_image, dst, *words):
        assert L.hp_rgb_to_yuv(C.byref(src_image), C.byref(dst.image), None) == HP_ERR_INVALID
        msg = L.hp_last_error().decode()
        assert msg.startswith("hp_rgb_to_yuv: ") and all(w in msg for w in words), msg
        assert dst.untouched()

    src = Source(frame, "bgra")
    for spoil, words in ((lambda d: setattr(d.image, "format", 9), ["unknown format 9"]),
                         (lambda d: setattr(d.image, "matrix", 3), ["HP_YUV_NV12", "matrix 3"]),
                         (lambda d: setattr(d.image, "range", 2), ["HP_YUV_NV12", "range 2"]),
                         (lambda d: setattr(d.image, "height", 5), ["HP_YUV_NV12", "even"]),
                         (lambda d: d.image.plane.__setitem__(1, None), ["HP_YUV_NV12", "plane 1 is null"]),
                         (lambda d: d.image.stride.__setitem__(0, 7), ["HP_YUV_NV12", "stride 7"]),
                         (lambda d: setattr(d.image, "width", 4), ["HP_YUV_NV12", "width 4", "HP_RGB_BGRA32"]),
                         (lambda d: setattr(d.image, "height", 2), ["HP_YUV_NV12", "height 2", "HP_RGB_BGRA32"])):
        dst = Surface("nv12", 8, 4)
        spoil(dst)
        refused(src.image, dst, *words)
    for spoil, words in ((lambda s: setattr(s, "format", 7), ["unknown format 7"]),
                         (lambda s: setattr(s, "data", None), ["HP_RGB_BGRA32", "data is null"]),
                         (lambda s: setattr(s, "stride", 23), ["HP_RGB_BGRA32", "stride 23"]),
                         (lambda s: setattr(s, "stride", 34), ["HP_RGB_BGRA32", "multiples of 4"]),
                         (lambda s: setattr(s, "data", s.data + 2), ["HP_RGB_BGRA32", "multiples of 4"])):
        other = Source(frame, "bgra")
        spoil(other.image)
        refused(other.image, Surface("nv12", 8, 4), *words)
    odd = Surface("p010", 8, 4, pitch=5)  # 16-bit words on the device need even strides
    refused(src.image, odd, "HP_YUV_P010", "even")
    small = Source(ref.random_frame(1, "gray", 1, 1), "gray")
    refused(small.image, Surface("nv12", 8194, 2), "HP_YUV_NV12", "8194 x 2", "8192")
