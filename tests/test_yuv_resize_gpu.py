"""GPU: hp_resize_yuv420 / hp_letterbox_yuv420 (resize_yuv.hip) against "convert the whole frame on the CPU (tests/yuv_ref.py), then the
restated cv::resize / non_scaling_resize (oracle/resize_oracle.cpp)": byte-equal, zero mismatches allowed - the bar hp_resize_u8c3 meets.

Oracle status: the conversion is a restatement of OpenCV's constants, parity unpinned (no OpenCV in the build image).  With cv2,
``cv2.cvtColor(yuv_ref.corner_frame("nv12"), cv2.COLOR_YUV2BGR_NV12)`` must equal ``yuv_ref.to_bgr(yuv_ref.corner_frame("nv12"), "nv12")``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from oracle import loader  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = ["nv12", "i420"]
# tests/test_resize_gpu.py's geometries with even sources (1280x720 and 1920x1080 -> 432x368 among them), the exact 2x down-scale
# (area mode), the identity size (conversion alone), up-scales, and the smallest frame a 4:2:0 layout can hold
RESIZE_GEOMETRIES = [(640, 480, 432, 368), (1280, 720, 432, 368), (1920, 1080, 432, 368), (100, 80, 432, 368), (864, 736, 432, 368),
                     (432, 368, 432, 368), (34, 58, 64, 64), (8, 6, 20, 3), (1920, 1080, 385, 385), (4, 2, 1, 1), (2, 2, 7, 5),
                     (216, 184, 432, 368)]
LETTERBOX_SOURCES = [(640, 480), (480, 640), (1280, 720), (1920, 1080), (432, 368), (500, 500), (34, 900), (864, 736), (100, 80)]


def _random_frame(sw, sh, seed):
    return np.random.default_rng(seed).integers(0, 256, (sh * 3 // 2, sw), dtype=np.uint8)


def _assert_same(got, want):
    bad = int((got != want).any(axis=-1).sum())
    assert bad == 0, f"{bad} of {got.shape[0] * got.shape[1]} pixels differ, first at {np.argwhere((got != want).any(axis=-1))[0].tolist()}"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sw,sh,dw,dh", RESIZE_GEOMETRIES)
def test_resize_yuv_bit_exact(hp, fmt, sw, sh, dw, dh):
    src = _random_frame(sw, sh, sw * 31 + dh)
    _assert_same(frontend.resize_yuv420_host(src, dw, dh, fmt), loader.resize_linear_u8(yuv_ref.to_bgr(src, fmt), dw, dh))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sw,sh", LETTERBOX_SOURCES)
def test_letterbox_yuv_bit_exact(hp, fmt, sw, sh):
    src = _random_frame(sw, sh, sw + sh)
    got = frontend.resize_yuv420_host(src, 432, 368, fmt, keep_ratio=True, bgcolor=(3, 250, 77))
    _assert_same(got, loader.letterbox_u8(yuv_ref.to_bgr(src, fmt), 432, 368, bgcolor=(3, 250, 77)))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dw,dh", [(64, 48), (32, 24), (432, 368), (50, 31), (200, 150)])
def test_corner_frame_every_saturation_branch(hp, fmt, dw, dh):
    """All (Y, U, V) in {0, 16, 128, 235, 255}^3: identity (conversion alone), the 2x area mode, up- and down-scales."""
    src = yuv_ref.corner_frame(fmt)
    bgr = yuv_ref.to_bgr(src, fmt)
    assert bgr.min() == 0 and bgr.max() == 255
    _assert_same(frontend.resize_yuv420_host(src, dw, dh, fmt), loader.resize_linear_u8(bgr, dw, dh))
    _assert_same(frontend.resize_yuv420_host(src, dw, dh, fmt, keep_ratio=True, bgcolor=(9, 8, 7)), loader.letterbox_u8(bgr, dw, dh, bgcolor=(9, 8, 7)))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sw,sh,dw,dh,pitch", [(1280, 720, 432, 368, 64), (100, 80, 432, 368, 28), (864, 736, 432, 368, 32), (64, 48, 64, 48, 2)])
def test_padded_pitch(hp, fmt, sw, sh, dw, dh, pitch):
    """Decoder surfaces: plane rows `pitch` bytes longer than the picture, the padding filled with other values."""
    src = _random_frame(sw, sh, sw + pitch)
    bgr = yuv_ref.to_bgr(src, fmt)
    _assert_same(frontend.resize_yuv420_host(src, dw, dh, fmt, pitch=pitch), loader.resize_linear_u8(bgr, dw, dh))
    _assert_same(frontend.resize_yuv420_host(src, dw, dh, fmt, keep_ratio=True, pitch=pitch), loader.letterbox_u8(bgr, dw, dh))


def test_fused_equals_two_steps_on_the_device(hp):
    """The statement of the feature itself: the fused kernel == hp_resize_u8c3 of the converted frame, both on the GPU."""
    src = _random_frame(1280, 720, 5)
    for fmt in FORMATS:
        _assert_same(frontend.resize_yuv420_host(src, 432, 368, fmt), frontend.resize_host(yuv_ref.to_bgr(src, fmt), 432, 368))


@pytest.mark.parametrize("letterbox", [False, True])
def test_invalid_arguments_are_refused(hp, letterbox):
    L = hp.lib()
    src, dst = hp.DevBuf(64 * 48 * 3 // 2), hp.DevBuf(32 * 32 * 3)
    sentinel = np.full(32 * 32 * 3, 0xCD, np.uint8)
    hp.check(L.hp_memcpy_h2d(dst.ptr, sentinel.ctypes.data_as(C.c_void_p), C.c_size_t(sentinel.nbytes)))
    y = src.ptr.value
    u, v = y + 64 * 48, y + 64 * 48 + 32 * 24

    def call(fmt, py, ys, pu, pv, uvs, sw, sh, pd=dst.ptr.value):
        args = [fmt, C.c_void_p(py), ys, C.c_void_p(pu), C.c_void_p(pv), uvs, sw, sh, C.c_void_p(pd), 32, 32, 96]
        if letterbox:
            return L.hp_letterbox_yuv420(*args, 0, 0, 0, None)
        return L.hp_resize_yuv420(*args, None)

    bad = [
        call(hp.HP_YUV_NV12, y, 63, u, None, 64, 63, 48),    # odd width
        call(hp.HP_YUV_I420, y, 64, u, v, 32, 64, 47),       # odd height
        call(hp.HP_YUV_NV12, None, 64, u, None, 64, 64, 48),  # null Y plane
        call(hp.HP_YUV_NV12, y, 64, None, None, 64, 64, 48),  # null UV plane
        call(hp.HP_YUV_I420, y, 64, u, None, 32, 64, 48),     # I420 without a V plane
        call(hp.HP_YUV_I420, y, 64, None, v, 32, 64, 48),     # I420 without a U plane
        call(hp.HP_YUV_NV12, y, 64, u, None, 64, 64, 48, pd=None),  # null destination
        call(hp.HP_YUV_NV12, y, 62, u, None, 64, 64, 48),     # luma stride smaller than a row
        call(hp.HP_YUV_NV12, y, 64, u, None, 32, 64, 48),     # NV12 chroma stride smaller than a row of pairs
        call(7, y, 64, u, v, 64, 64, 48),                     # unknown format
        call(hp.HP_YUV_NV12, y, 64, u, None, 64, 0, 0),       # empty
    ]
    assert bad == [hp.HP_ERR_INVALID] * len(bad), bad
    assert len(L.hp_last_error()) > 0
    hp.check(L.hp_device_synchronize())
    assert np.array_equal(dst.to_numpy(np.uint8, (32 * 32 * 3,)), sentinel), "a refused call wrote to the destination"
    assert call(hp.HP_YUV_NV12, y, 64, u, None, 64, 64, 48) == hp.HP_OK  # NV12 ignores dev_v
    hp.check(L.hp_device_synchronize())
