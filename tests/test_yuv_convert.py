"""CPU: the YUV 4:2:0 input path's constants, input generator and ABI (no GPU needed).

The integer conversion (tests/yuv_ref.py, the same statement as hyperpose_amd/csrc/resize_yuv.hip) is compared with an independent
float64 BT.601 limited-range evaluation over the full 256^3 (Y, U, V) cube; this guards the constants, not the kernel
(tests/test_yuv_resize_gpu.py does that).  Oracle status: parity with OpenCV unpinned, see tests/yuv_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref  # noqa: E402

from hyperpose_amd import _lib, synth  # noqa: E402


def test_integer_formula_within_one_of_float_bt601_over_the_cube():
    u = np.arange(256).reshape(256, 1)
    v = np.arange(256).reshape(1, 256)
    worst = np.zeros(3, np.int64)
    for y in range(256):
        got = yuv_ref.yuv_to_bgr(np.full((256, 256), y), u, v).astype(np.int64)
        yy = 1.164 * max(0, y - 16)
        uu, vv = u.astype(np.float64) - 128, v.astype(np.float64) - 128
        b = yy + 2.018 * uu + 0 * vv
        g = yy - 0.813 * vv - 0.391 * uu
        r = yy + 1.596 * vv + 0 * uu
        ref = np.clip(np.rint(np.stack([b, g, r], axis=-1)), 0, 255).astype(np.int64)
        worst = np.maximum(worst, np.abs(got - ref).reshape(-1, 3).max(0))
    print("max |integer - float64| over the cube (B, G, R):", worst.tolist())
    assert (worst <= 1).all(), worst.tolist()


def test_integer_formula_stays_inside_int32():
    # the extreme sums, evaluated in Python integers
    ymax = (255 - 16) * yuv_ref.CY + (1 << 19)
    sums = [ymax + yuv_ref.CUB * 127, yuv_ref.CUB * -128 + (1 << 19), ymax + yuv_ref.CVR * 127, yuv_ref.CVR * -128 + (1 << 19),
            ymax + (yuv_ref.CVG + yuv_ref.CUG) * -128, (yuv_ref.CVG + yuv_ref.CUG) * 127 + (1 << 19)]
    assert max(abs(s) for s in sums) < 2 ** 31 - 1
    assert max(abs(s) for s in sums) < 6e8


def test_known_pixels():
    # black, white, mid grey of limited range, and the clamps on both ends
    assert yuv_ref.yuv_to_bgr(16, 128, 128).tolist() == [0, 0, 0]
    assert yuv_ref.yuv_to_bgr(235, 128, 128).tolist() == [255, 255, 255]
    assert yuv_ref.yuv_to_bgr(0, 128, 128).tolist() == [0, 0, 0]
    assert yuv_ref.yuv_to_bgr(255, 128, 128).tolist() == [255, 255, 255]
    assert yuv_ref.yuv_to_bgr(126, 128, 128).tolist() == [128, 128, 128]
    # by hand: 1.164 * 112 = 130.4; B = 130.4 + 2.018 * 127 -> clamps high, G = 130.4 + 0.813 * 128 - 0.391 * 127 = 184.8, R = 130.4 - 1.596 * 128 -> clamps low
    assert yuv_ref.yuv_to_bgr(128, 255, 0).tolist() == [255, 185, 0]


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_corner_frame_holds_every_triple(fmt):
    y, u, v = yuv_ref.planes(yuv_ref.corner_frame(fmt), fmt)
    up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    seen = set(zip(y.ravel().tolist(), up(u).ravel().tolist(), up(v).ravel().tolist()))
    assert len(seen) == 125


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_bgr_to_yuv420_shapes_and_layout(fmt):
    frames = synth.images_u8(synth.rng_for(1, salt=9), 3, 36, 48)
    out = synth.bgr_to_yuv420(frames, fmt)
    assert out.shape == (3, 54, 48) and out.dtype == np.uint8 and out.flags.c_contiguous
    one = synth.bgr_to_yuv420(frames[1], fmt)
    assert one.shape == (54, 48) and np.array_equal(one, out[1])
    # a flat grey frame: Y = 16 + 219 * g / 255, chroma neutral; and the round trip through the library's conversion is close
    grey = np.full((4, 6, 3), 200, np.uint8)
    g = synth.bgr_to_yuv420(grey, fmt)
    assert (g[:4] == round(16 + 219 * 200 / 255)).all() and (g[4:] == 128).all()
    # distinct U and V land where the layout says: a blue frame has U > 128 > V
    blue = np.zeros((4, 6, 3), np.uint8)
    blue[..., 0] = 255
    _, u, v = yuv_ref.planes(synth.bgr_to_yuv420(blue, fmt), fmt)
    assert (u > 200).all() and (v < 128).all()
    smooth = np.broadcast_to(np.linspace(20, 230, 48).astype(np.uint8)[None, :, None], (36, 48, 3))
    back = yuv_ref.to_bgr(synth.bgr_to_yuv420(smooth, fmt), fmt)
    assert np.abs(back.astype(int) - smooth).max() <= 3


def test_bgr_to_yuv420_refuses_odd_sizes_and_unknown_formats():
    with pytest.raises(ValueError):
        synth.bgr_to_yuv420(np.zeros((5, 6, 3), np.uint8), "nv12")
    with pytest.raises(ValueError):
        synth.bgr_to_yuv420(np.zeros((4, 6, 3), np.uint8), "p010")


def test_abi_exports_the_yuv_symbols():
    L = _lib.lib()
    for name in ("hp_resize_yuv420", "hp_letterbox_yuv420", "hp_pipeline_submit_yuv"):
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS
    assert (_lib.HP_YUV_NV12, _lib.HP_YUV_I420) == (0, 1)
