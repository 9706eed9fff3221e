"""GPU: hp_resize_rois_rgb (resize_rgb.hip): many upright regions of one stored hp_rgb_image frame per launch, for all seven layouts.  The contract,
byte for byte: what hp_resize_rois_oriented_u8c3 - the existing path - gives on hp_rgb_to_bgr_host(src) with the same regions, orientation,
keep_ratio and background; bytes of a slot beyond dw * 3 in a row and beyond dh rows (the slot padding) keep their pre-fill; refusals are the same."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgb_ref  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402
from hyperpose_amd._lib import RGB_LAYOUTS, DevBuf, Roi  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 200, 120
DW, DH = 32, 24
FILL = (200, 3, 91)
PREFILL = 0xA5
DST_STRIDE = DW * 3 + 7
SLOT_STRIDE = (DH + 2) * DST_STRIDE + 13


def _upright(code):
    return (H, W) if code & 1 else (W, H)


def _regions(code, n):
    """n regions of the upright frame: the corner region that ends in the bottom-right pixel, one pixel, a 2 x 2 area and a copy region, then random
    ones - unsorted, overlapping, any alignment."""
    uw, uh = _upright(code)
    rng = np.random.default_rng(1000 + n + code)
    fixed = [(uw - 37, uh - 29, 37, 29), (uw - 1, uh - 1, 1, 1), (3, 5, 2 * DW, 2 * DH), (11, 1, DW, DH), (0, 0, uw, uh)]
    out = fixed[:min(n, 3)] if n <= 3 else fixed[:]
    while len(out) < n:
        w, h = int(rng.integers(1, uw + 1)), int(rng.integers(1, uh + 1))
        out.append((int(rng.integers(0, uw - w + 1)), int(rng.integers(0, uh - h + 1)), w, h))
    order = rng.permutation(n)
    return [out[i] for i in order]


def _slots(n):
    return DevBuf.from_numpy(np.full(n * SLOT_STRIDE, PREFILL, np.uint8))


def _split(dst, n):
    flat = dst.to_numpy(np.uint8, (n * SLOT_STRIDE,)).reshape(n, SLOT_STRIDE)
    rows = flat[:, :DH * DST_STRIDE].reshape(n, DH, DST_STRIDE)
    return rows[:, :, :DW * 3].copy(), np.concatenate([rows[:, :, DW * 3:].ravel(), flat[:, DH * DST_STRIDE:].ravel()])


def _sync():
    _lib.check(_lib.lib().hp_device_synchronize())


@pytest.fixture(scope="module")
def world(hp):
    rng = np.random.default_rng(42)
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frames = {}
    for fmt in rgb_ref.FORMATS:
        view, whole = rgb_ref.padded(rgb_ref.from_bgr(bgr, fmt, rng), 12 if rgb_ref.pixel_bytes(fmt) == 4 else 5, 0x5A)
        as_bgr = frontend.rgb_to_bgr_host(view, fmt)
        assert as_bgr.tobytes() == rgb_ref.to_bgr(view, fmt).tobytes()
        dev = DevBuf.from_numpy(whole)
        frames[fmt] = (frontend.rgb_image(fmt, dev, W, H, whole.shape[1]), dev, as_bgr)
    refs = {}

    def want(fmt, code, n, keep_ratio):
        key = ("gray" if fmt == "gray" else "colour", code, n, keep_ratio)  # every colour layout holds the same picture
        if key not in refs:
            _, bwhole = rgb_ref.padded(frames[fmt][2], 5, 0x5A)
            dst, src = _slots(n), DevBuf.from_numpy(bwhole)  # (src stays alive until the kernels have run)
            frontend.resize_rois(src, _regions(code, n), dst, DW, DH, keep_ratio, FILL, sw=W, sh=H, src_stride=bwhole.shape[1],
                                 dst_stride=DST_STRIDE, slot_stride=SLOT_STRIDE, orientation=code)
            _sync()
            pics, rest = _split(dst, n)
            assert (rest == PREFILL).all()
            refs[key] = pics
        return refs[key]
    return frames, want


def _check(world, fmt, code, n, keep_ratio):
    frames, want = world
    dst = _slots(n)
    frontend.resize_rois_rgb(frames[fmt][0], _regions(code, n), dst, DW, DH, code, keep_ratio, FILL, dst_stride=DST_STRIDE, slot_stride=SLOT_STRIDE)
    _sync()
    got, rest = _split(dst, n)
    what = f"{fmt} code {code} {n} regions keep_ratio {keep_ratio}"
    assert (rest == PREFILL).all(), what + ": the slot padding was written"
    ref = want(fmt, code, n, keep_ratio)
    bad = np.argwhere((got != ref).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} row-bytes groups differ, first (slot, row) {bad[0].tolist()} = region {_regions(code, n)[bad[0][0]]}"


@pytest.mark.parametrize("fmt", rgb_ref.FORMATS)
def test_three_regions_every_orientation_and_ratio(world, fmt):
    for code in (0, 1, 5):
        for keep_ratio in (False, True):
            _check(world, fmt, code, 3, keep_ratio)


@pytest.mark.parametrize("fmt", rgb_ref.FORMATS)
@pytest.mark.parametrize("n", [17, 64])
def test_many_regions(world, fmt, n):
    _check(world, fmt, 0, n, n == 17)
    _check(world, fmt, 5, n, n == 64)


def _refused(im, code, rois, n, dst, stride, slot_stride, *needles):
    arr = (Roi * max(1, len(rois)))(*[Roi(*r) for r in rois])
    rc = _lib.lib().hp_resize_rois_rgb(C.byref(im), code, arr, n, 0, 0, 0, 0, dst, DW, DH, stride, C.c_size_t(slot_stride), None)
    assert rc == _lib.HP_ERR_INVALID, needles
    msg = _lib.lib().hp_last_error().decode()
    for s in needles:
        assert s in msg, (s, msg)


def test_refusals_are_those_of_the_bgr_path(world):
    frames, _ = world
    im = frames["argb"][0]
    dst = _slots(4)
    ok = [(0, 0, 10, 10)]
    _refused(im, 0, ok, 0, dst.ptr, DST_STRIDE, SLOT_STRIDE, "HP_RGB_ARGB32", "0 regions")
    _refused(im, 0, ok * 65, 65, dst.ptr, DST_STRIDE, SLOT_STRIDE, "HP_RGB_ARGB32", "65 regions")
    _refused(im, 0, [(W - 9, 0, 10, 10)], 1, dst.ptr, DST_STRIDE, SLOT_STRIDE, "HP_RGB_ARGB32", "region 0", "200 x 120")
    _refused(im, 1, [(0, 0, 10, 10), (H - 9, 0, 10, 10)], 2, dst.ptr, DST_STRIDE, SLOT_STRIDE, "HP_RGB_ARGB32", "region 1", "120 x 200")
    _refused(im, 0, [(0, 0, 0, 10)], 1, dst.ptr, DST_STRIDE, SLOT_STRIDE, "region 0")
    _refused(im, 0, ok, 1, dst.ptr, DST_STRIDE, DH * DST_STRIDE - 1, "HP_RGB_ARGB32", "slot stride")
    _refused(im, 0, ok, 1, dst.ptr, DW * 3 - 1, SLOT_STRIDE, "bad destination")
    _refused(im, 0, ok, 1, None, DST_STRIDE, SLOT_STRIDE, "null argument")
    _refused(im, 9, ok, 1, dst.ptr, DST_STRIDE, SLOT_STRIDE, "orientation 9")
    bad = frontend.rgb_image("argb", frames["argb"][1].ptr.value + 2, W - 1, H, im.stride)
    _refused(bad, 0, ok, 1, dst.ptr, DST_STRIDE, SLOT_STRIDE, "HP_RGB_ARGB32", "address % 4 = 2")
    _sync()
    assert (dst.to_numpy(np.uint8, (dst.nbytes,)) == PREFILL).all(), "a refused call wrote into the destination"
    # any alignment of a region is fine in every layout (1 x 1), also behind a quarter turn
    assert RGB_LAYOUTS["gray"][1] == 1
    for fmt in ("gray", "rgb24", "abgr"):
        frontend.resize_rois_rgb(frames[fmt][0], [(1, 3, 5, 7), (7, 1, 1, 1)], dst, DW, DH, 1, dst_stride=DST_STRIDE, slot_stride=SLOT_STRIDE)
    _sync()
