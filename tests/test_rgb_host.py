"""CPU: the host side of hp_rgb_image (include/hp_hip.h, "packed RGB and grey frames"): hp_rgb_to_bgr_host - the definition every parity statement of
the RGB feeds refers to - against the numpy twin of the rule (tests/rgb_ref.py), the two size functions against _lib.RGB_LAYOUTS, and every refusal
of a description, whose message names the layout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgb_ref  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402
from hyperpose_amd._lib import RGB_LAYOUTS, HpError, RgbImage  # noqa: E402

NAMES = {"bgr24": "HP_RGB_BGR24", "rgb24": "HP_RGB_RGB24", "bgra": "HP_RGB_BGRA32", "rgba": "HP_RGB_RGBA32", "argb": "HP_RGB_ARGB32",
         "abgr": "HP_RGB_ABGR32", "gray": "HP_RGB_GRAY8"}


def test_the_two_tables_name_the_same_layouts():
    assert sorted(RGB_LAYOUTS) == sorted(rgb_ref.FORMATS) == sorted(NAMES)
    assert sorted(v[0] for v in RGB_LAYOUTS.values()) == list(range(7))
    for fmt, (code, pb, b, g, r) in RGB_LAYOUTS.items():
        o = rgb_ref.ORDER[fmt]
        assert pb == len(o) == frontend.rgb_pixel_bytes(fmt)
        assert (b, g, r) == ((0, 0, 0) if o == "Y" else tuple(o.index(c) for c in "BGR")), fmt


@pytest.mark.parametrize("fmt", rgb_ref.FORMATS)
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (97, 65)])
def test_to_bgr_host_equals_the_numpy_rule(fmt, size):
    w, h = size
    rng = np.random.default_rng(w * 7 + h)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    frame, whole = rgb_ref.padded(rgb_ref.from_bgr(bgr, fmt, rng), 5, 0xEE)  # a padded stride, the padding poisoned
    want = rgb_ref.to_bgr(frame, fmt)
    if fmt != "gray":
        assert want.tobytes() == bgr.tobytes()
    got = frontend.rgb_to_bgr_host(frame, fmt, pitch=w * 3 + 7, fill=0x3C)
    assert got.tobytes() == want.tobytes()
    assert (got.base[:, w * 3:] == 0x3C).all(), "the padding of the output rows was written"
    assert (whole[:, w * rgb_ref.pixel_bytes(fmt):] == 0xEE).all()
    assert frontend.rgb_to_bgr_host(np.ascontiguousarray(frame), fmt).tobytes() == want.tobytes()  # tight in, tight out


def test_alpha_is_ignored():
    rng = np.random.default_rng(5)
    bgr = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    for fmt in ("bgra", "rgba", "argb", "abgr"):
        a, b = rgb_ref.from_bgr(bgr, fmt, np.random.default_rng(1)), rgb_ref.from_bgr(bgr, fmt, np.random.default_rng(2))
        assert a.tobytes() != b.tobytes()
        assert frontend.rgb_to_bgr_host(a, fmt).tobytes() == frontend.rgb_to_bgr_host(b, fmt).tobytes() == bgr.tobytes()


def test_sizes():
    L = _lib.lib()
    for fmt, (code, pb, *_rest) in RGB_LAYOUTS.items():
        assert L.hp_rgb_pixel_bytes(code) == pb
        for w, h in [(1, 1), (5, 3), (97, 65), (1920, 1080)]:
            assert frontend.rgb_packed_bytes(fmt, w, h) == w * h * pb
        for w, h in [(0, 4), (4, 0), (-1, 4), (4, -3)]:
            assert frontend.rgb_packed_bytes(fmt, w, h) == 0
    for bad in (-1, 7, 9):
        assert L.hp_rgb_pixel_bytes(bad) == 0 and L.hp_rgb_packed_bytes(bad, 4, 4) == 0


def _refused(im, out, stride, *needles):
    rc = _lib.lib().hp_rgb_to_bgr_host(C.byref(im) if im is not None else None, out.ctypes.data_as(C.c_void_p) if out is not None else None, stride)
    assert rc == _lib.HP_ERR_INVALID
    msg = _lib.lib().hp_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)
    return msg


@pytest.mark.parametrize("fmt", rgb_ref.FORMATS)
def test_refusals_name_the_layout(fmt):
    code, pb = RGB_LAYOUTS[fmt][:2]
    w, h = 6, 4
    src = np.zeros((h, w * pb + 4), np.uint8)
    out = np.full((h, w * 3), 0x77, np.uint8)
    ok = RgbImage(code, w, h, src.ctypes.data, w * pb + 4)
    assert _lib.lib().hp_rgb_to_bgr_host(C.byref(ok), out.ctypes.data_as(C.c_void_p), w * 3) == 0
    out[:] = 0x77
    name = NAMES[fmt]
    _refused(RgbImage(code, 0, h, src.ctypes.data, 32), out, w * 3, name, "0 x 4")
    _refused(RgbImage(code, w, -2, src.ctypes.data, 32), out, w * 3, name, "6 x -2")
    _refused(RgbImage(code, w, h, None, 32), out, w * 3, name, "null")
    _refused(RgbImage(code, w, h, src.ctypes.data, w * pb - 1), out, w * 3, name, f"stride {w * pb - 1}", f"{w * pb} bytes")
    _refused(ok, None, w * 3, name, "null")
    _refused(ok, out, w * 3 - 1, name, f"stride {w * 3 - 1}")
    assert (out == 0x77).all(), "a refused call wrote"


def test_refusals_without_a_layout():
    out = np.zeros((4, 18), np.uint8)
    src = np.zeros((4, 32), np.uint8)
    _refused(None, out, 18, "null image")
    for bad in (-1, 7, 9):
        _refused(RgbImage(bad, 6, 4, src.ctypes.data, 32), out, 18, f"unknown format {bad}", "HP_RGB_BGR24", "HP_RGB_GRAY8")


def test_host_frames_have_no_alignment_rule():
    # an odd address and an odd stride: fine for a host frame (repacked bytewise); the device calls refuse it (tests/test_rgb_resize_gpu.py)
    rng = np.random.default_rng(3)
    buf = rng.integers(0, 256, 1 + 5 * 31, dtype=np.uint8)
    im = RgbImage(RGB_LAYOUTS["bgra"][0], 7, 5, buf.ctypes.data + 1, 31)
    want = rgb_ref.to_bgr(np.lib.stride_tricks.as_strided(buf[1:], (5, 7, 4), (31, 4, 1)), "bgra")
    assert frontend.rgb_to_bgr_host(im).tobytes() == want.tobytes()


def test_python_rejects_a_frame_of_the_wrong_shape():
    with pytest.raises(ValueError):
        frontend.rgb_host_image(np.zeros((4, 4, 3), np.uint8), "bgra")
    with pytest.raises(ValueError):
        frontend.rgb_host_image(np.zeros((4, 4, 3), np.uint8), "gray")
    with pytest.raises(HpError):
        frontend.rgb_to_bgr_host(RgbImage(3, 4, 4, None, 16))
