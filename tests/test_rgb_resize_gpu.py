"""GPU: hp_resize_rgb (resize_rgb.hip) for all seven hp_rgb_image layouts.  The contract, byte for byte: what hp_resize_oriented_u8c3 - the existing
path - gives on hp_rgb_to_bgr_host(src), for every size, orientation code, keep_ratio and background.  The source is strided with poisoned padding
(and random alpha that holds 0 and 255); the destination is strided with poisoned padding and poisoned rows beyond dh, which must come back intact.
Refused calls launch nothing."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgb_ref  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402
from hyperpose_amd._lib import RGB_LAYOUTS, DevBuf, RgbImage  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = (3, 250, 77)
PREFILL = 0xA5
TAIL_ROWS = 2

# (sw, sh, dw, dh, keep_ratio, what)
GEOMETRIES = [(97, 65, 64, 48, False, "linear, odd sizes"), (128, 96, 64, 48, False, "2 x 2 area"), (64, 48, 64, 48, False, "copy"),
              (31, 17, 64, 48, False, "up-scaling, one-tap last column"), (1, 1, 8, 8, False, "one pixel"), (97, 65, 64, 48, True, "letterbox")]


def _dst(dw, dh):
    stride = dw * 3 + 7
    return DevBuf.from_numpy(np.full((dh + TAIL_ROWS) * stride + 11, PREFILL, np.uint8)), stride


def _split(dst, stride, dw, dh):
    """([dh, dw, 3] picture, every other byte of the destination)"""
    flat = dst.to_numpy(np.uint8, ((dh + TAIL_ROWS) * stride + 11,))
    rows = flat[:dh * stride].reshape(dh, stride)
    return rows[:, :dw * 3].reshape(dh, dw, 3).copy(), np.concatenate([rows[:, dw * 3:].ravel(), flat[dh * stride:]])


def _sync():
    _lib.check(_lib.lib().hp_device_synchronize())


class Frame:
    """One host frame of a layout on the device with a padded, poisoned pitch, and its BGR form (the definition's) on the device as well."""

    def __init__(self, fmt, w, h, seed):
        rng = np.random.default_rng(seed)
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        pb = rgb_ref.pixel_bytes(fmt)
        self.fmt, self.w, self.h = fmt, w, h
        view, whole = rgb_ref.padded(rgb_ref.from_bgr(bgr, fmt, rng), 8 if pb == 4 else 5, 0x5A)
        self.bgr = frontend.rgb_to_bgr_host(view, fmt)
        assert self.bgr.tobytes() == rgb_ref.to_bgr(view, fmt).tobytes()
        self.pitch = whole.shape[1]
        self.dev = DevBuf.from_numpy(whole)
        self.image = frontend.rgb_image(fmt, self.dev, w, h, self.pitch)
        bview, bwhole = rgb_ref.padded(self.bgr, 5, 0x5A)
        self.bgr_pitch = bwhole.shape[1]
        self.bgr_dev = DevBuf.from_numpy(bwhole)

    def got(self, dw, dh, code, keep_ratio):
        dst, stride = _dst(dw, dh)
        frontend.resize_rgb(self.image, dst, dw, dh, code, keep_ratio, FILL, dst_stride=stride)
        _sync()
        return _split(dst, stride, dw, dh)

    def want(self, dw, dh, code, keep_ratio):
        dst, stride = _dst(dw, dh)
        frontend.resize_oriented(self.bgr_dev, dst, dw, dh, code, keep_ratio, FILL, sw=self.w, sh=self.h, src_stride=self.bgr_pitch, dst_stride=stride)
        _sync()
        pic, rest = _split(dst, stride, dw, dh)
        assert (rest == PREFILL).all()
        return pic


@pytest.fixture(scope="module")
def frames(hp):
    cache = {}

    def get(fmt, w, h):
        if (fmt, w, h) not in cache:
            cache[fmt, w, h] = Frame(fmt, w, h, 100 + w + h)  # one seed per size: every colour layout holds the same BGR picture
        return cache[fmt, w, h]
    return get


def _same(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


@pytest.mark.parametrize("fmt", rgb_ref.FORMATS)
def test_every_geometry_equals_the_bgr_path(hp, frames, fmt):
    for sw, sh, dw, dh, keep_ratio, what in GEOMETRIES:
        f = frames(fmt, sw, sh)
        got, rest = f.got(dw, dh, 0, keep_ratio)
        what = f"{fmt} {sw} x {sh} -> {dw} x {dh} ({what})"
        assert (rest == PREFILL).all(), what + ": bytes outside dw * 3 x dh were written"
        _same(got, f.want(dw, dh, 0, keep_ratio), what)


@pytest.mark.parametrize("fmt", rgb_ref.FORMATS)
def test_every_orientation_equals_the_bgr_path(hp, frames, fmt):
    f = frames(fmt, 97, 65)
    for code in range(8):
        for dw, dh, keep_ratio in [(64, 48, False), (48, 64, True)]:
            got, rest = f.got(dw, dh, code, keep_ratio)
            what = f"{fmt} code {code} 97 x 65 -> {dw} x {dh} keep_ratio {keep_ratio}"
            assert (rest == PREFILL).all(), what + ": bytes outside dw * 3 x dh were written"
            _same(got, f.want(dw, dh, code, keep_ratio), what)


def test_colour_layouts_of_one_picture_agree_and_grey_is_replicated(hp, frames):
    ref = frames("bgr24", 97, 65)
    for fmt in rgb_ref.COLOUR:
        assert frames(fmt, 97, 65).bgr.tobytes() == ref.bgr.tobytes()
        _same(frames(fmt, 97, 65).got(64, 48, 3, True)[0], ref.want(64, 48, 3, True), fmt)
    g = frames("gray", 97, 65)
    assert (g.bgr[..., 0] == g.bgr[..., 1]).all() and (g.bgr[..., 0] == g.bgr[..., 2]).all()
    got = g.got(64, 48, 0, False)[0]
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()


def test_bgr24_equals_the_u8c3_calls_on_the_same_buffer(hp, frames):
    f = frames("bgr24", 97, 65)
    for code in range(8):
        for keep_ratio in (False, True):
            dst, stride = _dst(64, 48)
            frontend.resize_oriented(f.dev, dst, 64, 48, code, keep_ratio, FILL, sw=97, sh=65, src_stride=f.pitch, dst_stride=stride)
            _sync()
            want = dst.to_numpy(np.uint8, ((48 + TAIL_ROWS) * stride + 11,))
            dst2, _ = _dst(64, 48)
            frontend.resize_rgb(f.image, dst2, 64, 48, code, keep_ratio, FILL, dst_stride=stride)
            _sync()
            assert dst2.to_numpy(np.uint8, want.shape).tobytes() == want.tobytes(), (code, keep_ratio)


CHILD = """
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
sys.path.insert(0, sys.argv[1])
import rgb_ref
from hyperpose_amd import _lib, frontend
_lib.init(0)
rng = np.random.default_rng(7)
bgr = rng.integers(0, 256, (65, 97, 3), dtype=np.uint8)
bdev = _lib.DevBuf.from_numpy(bgr)
for fmt in ["bgra", "rgba", "argb", "abgr", "rgb24", "gray"]:
    frame = rgb_ref.from_bgr(bgr, fmt, rng)
    ref = _lib.DevBuf.from_numpy(rgb_ref.to_bgr(frame, fmt))
    dev = _lib.DevBuf.from_numpy(frame)
    for code in range(8):
        for dw, dh, keep in [(40, 33, False), (150, 131, False), (48, 48, True)]:
            a = _lib.DevBuf.from_numpy(np.full(dw * dh * 3 + 5, 0xA5, np.uint8))
            b = _lib.DevBuf.from_numpy(np.full(dw * dh * 3 + 5, 0xA5, np.uint8))
            frontend.resize_rgb(frontend.rgb_image(fmt, dev, 97, 65), a, dw, dh, code, keep, (9, 8, 7))
            frontend.resize_oriented(ref, b, dw, dh, code, keep, (9, 8, 7), sw=97, sh=65)
            _lib.check(_lib.lib().hp_device_synchronize())
            assert a.to_numpy(np.uint8, (dw * dh * 3 + 5,)).tobytes() == b.to_numpy(np.uint8, (dw * dh * 3 + 5,)).tobytes(), (fmt, code, dw, dh, keep)
print("CHILD_OK")
"""


@pytest.mark.parametrize("taps,thread_map", [("bytes", "rows"), ("words", "cols")])
def test_both_taps_and_both_thread_maps_write_the_same_bytes(hp, taps, thread_map):
    """HP_RGB_TAPS forces the Taps type of the 4-byte layouts and HP_ORIENT_MAP the thread map (both read once per process, hence the child, and both
    applied to the reference call's unit too): every code through the kernels the defaults do not pick for it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", CHILD, root], env=dict(os.environ, HP_RGB_TAPS=taps, HP_ORIENT_MAP=thread_map), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split()[-1:] == ["CHILD_OK"], out.stdout[-1500:] + out.stderr[-1500:]


def _refused(im, code, dst, dw, dh, stride, *needles):
    rc = _lib.lib().hp_resize_rgb(C.byref(im) if im is not None else None, code, 0, 0, 0, 0, dst, dw, dh, stride, None)
    assert rc == _lib.HP_ERR_INVALID, needles
    msg = _lib.lib().hp_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_launch_nothing(hp, frames):
    f = frames("bgra", 97, 65)
    dst, stride = _dst(64, 48)
    d, im = dst.ptr, f.image
    code_of = lambda fmt: RGB_LAYOUTS[fmt][0]
    _refused(im, 8, d, 64, 48, stride, "orientation 8")
    _refused(im, -1, d, 64, 48, stride, "orientation -1")
    _refused(None, 0, d, 64, 48, stride, "null image")
    _refused(RgbImage(9, 97, 65, im.data, f.pitch), 0, d, 64, 48, stride, "unknown format 9")
    _refused(RgbImage(7, 97, 65, im.data, f.pitch), 0, d, 64, 48, stride, "unknown format 7")
    for fmt, name in [("bgra", "HP_RGB_BGRA32"), ("rgb24", "HP_RGB_RGB24"), ("gray", "HP_RGB_GRAY8")]:
        pb = RGB_LAYOUTS[fmt][1]
        _refused(RgbImage(code_of(fmt), 0, 65, im.data, f.pitch), 0, d, 64, 48, stride, name, "0 x 65")
        _refused(RgbImage(code_of(fmt), 97, 65, None, f.pitch), 0, d, 64, 48, stride, name, "null")
        _refused(RgbImage(code_of(fmt), 97, 65, im.data, 97 * pb - 1), 0, d, 64, 48, stride, name, f"stride {97 * pb - 1}")
    # a misaligned 4-byte plane: the address, then the stride; the 1- and 3-byte layouts have no such rule
    for fmt, name in [("bgra", "HP_RGB_BGRA32"), ("rgba", "HP_RGB_RGBA32"), ("argb", "HP_RGB_ARGB32"), ("abgr", "HP_RGB_ABGR32")]:
        _refused(RgbImage(code_of(fmt), 96, 65, im.data + 1, f.pitch), 0, d, 64, 48, stride, name, "multiples of 4", "address % 4 = 1")
        _refused(RgbImage(code_of(fmt), 96, 65, im.data + 2, f.pitch), 0, d, 64, 48, stride, name, "address % 4 = 2")
        _refused(RgbImage(code_of(fmt), 96, 65, im.data, f.pitch - 2), 0, d, 64, 48, stride, name, "multiples of 4", f"stride {f.pitch - 2}")
    # the destination: the refusals of the BGR path
    _refused(im, 0, None, 64, 48, stride, "bad geometry")
    _refused(im, 0, d, 0, 48, stride, "bad geometry")
    _refused(im, 1, d, 64, 0, stride, "bad geometry")
    _refused(im, 0, d, 64, 48, 64 * 3 - 1, "row stride smaller than a row")
    _sync()
    assert (dst.to_numpy(np.uint8, (dst.nbytes,)) == PREFILL).all(), "a refused call wrote into the destination"
    # ... and an odd address and stride are fine for the 3-byte and the grey layout: bytes of the BGR path again
    g = frames("rgb24", 97, 65)
    odd = RgbImage(code_of("rgb24"), 96, 64, g.image.data + g.pitch + 3, g.pitch)
    frontend.resize_rgb(odd, dst, 64, 48, 0, False, dst_stride=stride)
    ref, _ = _dst(64, 48)
    frontend.resize_oriented(g.bgr_dev.ptr.value + g.bgr_pitch + 3, ref, 64, 48, 0, False, sw=96, sh=64, src_stride=g.bgr_pitch, dst_stride=stride)
    _sync()
    assert _split(dst, stride, 64, 48)[0].tobytes() == _split(ref, stride, 64, 48)[0].tobytes()
