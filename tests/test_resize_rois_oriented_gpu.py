"""GPU: hp_resize_rois_oriented_u8c3 / hp_resize_rois_oriented_yuv (resize_oriented.hip): regions in UPRIGHT coordinates of a stored frame.  Slot i ==
the per-frame oriented call on the region's stored rectangle cut out into a frame of its own, byte for byte, and == the CPU oracle on the
upright cut-out; bytes of the destination that belong to no slot's picture keep their pre-fill; misaligned stored rectangles are refused."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_ref  # noqa: E402
import orient_ref  # noqa: E402
import yuv_formats_ref as ref  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from hyperpose_amd._lib import DevBuf, Roi  # noqa: E402
from oracle import loader  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = (3, 250, 77)
PREFILL = 0xA5


def _run(src, rois, dw, dh, keep_ratio, code, **kw):
    n = len(rois)
    dst_stride, slot_stride = dw * 3 + 7, (dw * 3 + 7) * dh + 11
    dst = DevBuf.from_numpy(np.full(n * slot_stride, PREFILL, np.uint8))
    frontend.resize_rois(src, rois, dst, dw, dh, keep_ratio, FILL, dst_stride=dst_stride, slot_stride=slot_stride, orientation=code, **kw)
    frontend.check(frontend.lib().hp_device_synchronize())
    flat = dst.to_numpy(np.uint8, (n, slot_stride))
    rows = flat[:, :dh * dst_stride].reshape(n, dh, dst_stride)
    return rows[:, :, :dw * 3].reshape(n, dh, dw, 3).copy(), np.concatenate([rows[:, :, dw * 3:].ravel(), flat[:, dh * dst_stride:].ravel()])


def _frame(src, dw, dh, keep_ratio, code, **kw):
    dst = DevBuf(dw * dh * 3)
    frontend.resize_oriented(src, dst, dw, dh, code, keep_ratio, FILL, **kw)
    frontend.check(frontend.lib().hp_device_synchronize())
    return dst.to_numpy(np.uint8, (dh, dw, 3))


def _assert_slot(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}"


def _oracle(cut, dw, dh, keep_ratio):
    return loader.letterbox_u8(cut, dw, dh, bgcolor=FILL) if keep_ratio else loader.resize_linear_u8(cut, dw, dh)


# ---- BGR ------------------------------------------------------------------------------------------------------------------------------

SW, SH, PITCH = 97, 61, 97 * 3 + 5


def _bgr_rois(uw, uh):
    """17 upright regions of a uw x uh frame (one more than a launch carries); the first 9: the whole frame, the four corners, 2 x 2 pixels at the
    far corner, the slot's size (copy), twice the slot's size (area), a sliver on the far edge."""
    hw, hh = uw // 2, uh // 2
    return [(0, 0, uw, uh), (0, 0, hw, hh), (uw - hw, 0, hw, hh), (0, uh - hh, hw, hh), (uw - hw, uh - hh, hw, hh), (uw - 2, uh - 2, 2, 2),
            (5, 7, 30, 26), (1, 0, 60, 52), (uw - 7, 3, 7, uh - 5),
            (0, 0, 1, 1), (uw - 1, uh - 1, 1, 1), (0, uh - 1, uw, 1), (uw - 1, 0, 1, uh), (3, 2, 41, 29), (3, 2, 41, 29), (1, 1, uw - 1, uh - 1),
            (10, 10, 2, 2)]


@pytest.fixture(scope="module")
def bgr(hp):
    img = np.random.default_rng(21).integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    padded = np.full((SH, PITCH), 0x5A, np.uint8)
    padded[:, :SW * 3] = img.reshape(SH, SW * 3)
    return img, DevBuf.from_numpy(padded)


@pytest.mark.parametrize("code", orient_ref.CODES)
def test_bgr_slots_equal_the_per_frame_oriented_call_on_the_cut_out(hp, bgr, code):
    img, dev = bgr
    uw, uh = orient_ref.oriented_size(code, SW, SH)
    upright = orient_ref.orient(img, code)
    all_rois = _bgr_rois(uw, uh)
    assert len(all_rois) == 17
    dw, dh = 30, 26
    for rois, keep_ratio in [(all_rois[:9], False), (all_rois, True), (all_rois, False)]:
        got, rest = _run(dev, rois, dw, dh, keep_ratio, code, sw=SW, sh=SH, src_stride=PITCH)
        assert (rest == PREFILL).all(), "bytes outside the slots' pictures were written"
        for i, r in enumerate(rois):
            what = f"code {code} region {i} {r} keep_ratio={keep_ratio}"
            x, y, w, h = orient_ref.orient_roi(r, code, SW, SH)
            assert frontend.orient_roi(r, code, SW, SH) == (x, y, w, h)
            stored_cut = DevBuf.from_numpy(np.ascontiguousarray(img[y:y + h, x:x + w]))
            _assert_slot(got[i], _frame(stored_cut, dw, dh, keep_ratio, code, sw=w, sh=h), what + " vs the per-frame oriented call")
            _assert_slot(got[i], _oracle(np.ascontiguousarray(upright[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]), dw, dh, keep_ratio), what + " vs the CPU oracle")


# ---- YUV ------------------------------------------------------------------------------------------------------------------------------

YW, YH = 64, 48
PITCHES = {2: (34, 6), 3: (2, 70, 6), 1: (26,)}


def _yuv_rois(uw, uh, ax, ay):
    """Upright regions aligned to every layout (even everything): the whole frame, the four corners, 2 x 2 pixels at the far corner, copy and
    area sizes; plus odd ones where the layout's alignment (already swapped for a turned frame) allows them."""
    hw, hh = uw // 2, uh // 2
    rois = [(0, 0, uw, uh), (0, 0, hw, hh), (uw - hw, 0, hw, hh), (0, uh - hh, hw, hh), (uw - hw, uh - hh, hw, hh), (uw - 2, uh - 2, 2, 2),
            (2, 4, 24, 20), (0, 2, 48, 40), (uw - 2, 0, 2, uh), (0, uh - 2, uw, 2), (10, 6, 36, 38)]
    return rois + ([(3, 0, 21, 40)] if ax == 1 else []) + ([(4, 5, 20, 33)] if ay == 1 else [])


def _sub_planes(planes, fmt, x, y, w, h):
    n, _, sx, sy = ref.LAYOUT[fmt]
    if n == 1:
        return [planes[0][y:y + h, 2 * x:2 * (x + w)]]
    cy0, cy1, cx0, cx1 = y >> sy, (y + h) >> sy, x >> sx, (x + w) >> sx
    if n == 2:
        return [planes[0][y:y + h, x:x + w], planes[1][cy0:cy1, 2 * cx0:2 * cx1]]
    return [planes[0][y:y + h, x:x + w], planes[1][cy0:cy1, cx0:cx1], planes[2][cy0:cy1, cx0:cx1]]


@pytest.mark.parametrize("fmt,hdr", [("nv12", False), ("yuy2", False), ("i444", False), ("p010", True)])
def test_yuv_slots_equal_the_per_frame_oriented_call_on_the_sub_planes(hp, fmt, hdr):
    matrix, range_ = ("bt2020", "limited") if hdr else ("bt709", "full")
    frame = ref.random_frame(fmt, YW, YH, 61 + ref.FORMATS.index(fmt))
    planes = frontend.yuv_planes(frame, fmt, YW, YH)
    bufs, strides = frontend.yuv_upload(planes, fmt, PITCHES[len(planes)], fill=0x5A)
    im = frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, YW, YH, matrix, range_)
    tm = frontend.Tonemap("pq", True) if hdr else None
    if hdr:
        A, M, O = frontend.tonemap_tables("pq", True)
        bgr = hdr_ref.to_bgr(frame, fmt, YW, YH, matrix, range_, A, M, O, True)
    else:
        bgr = ref.to_bgr(frame, fmt, YW, YH, matrix, range_)
    ax, ay = frontend.yuv_roi_alignment(fmt)
    dw, dh = 24, 20
    try:
        for code in orient_ref.CODES:
            uw, uh = orient_ref.oriented_size(code, YW, YH)
            upright = orient_ref.orient(bgr, code)
            rois = _yuv_rois(uw, uh, *((ay, ax) if code & 1 else (ax, ay)))
            for keep_ratio in (False, True):
                got, rest = _run(im, rois, dw, dh, keep_ratio, code, tonemap=tm)
                assert (rest == PREFILL).all(), "bytes outside the slots' pictures were written"
                for i, r in enumerate(rois):
                    what = f"{fmt} code {code} region {i} {r} keep_ratio={keep_ratio}"
                    x, y, w, h = orient_ref.orient_roi(r, code, YW, YH)
                    sub = [np.ascontiguousarray(p) for p in _sub_planes(planes, fmt, x, y, w, h)]
                    sb, ss = frontend.yuv_upload(sub, fmt, 2)
                    cut = frontend.yuv_image(fmt, [b.ptr for b in sb], ss, w, h, matrix, range_)
                    _assert_slot(got[i], _frame(cut, dw, dh, keep_ratio, code, tonemap=tm), what + " vs the per-frame oriented call")
                    _assert_slot(got[i], _oracle(np.ascontiguousarray(upright[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]), dw, dh, keep_ratio),
                                 what + " vs the CPU conversion and oracle")
    finally:
        frontend.check(frontend.lib().hp_device_synchronize())
        if tm is not None:
            tm.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing(hp):
    L = hp.lib()
    dw, dh = 16, 12
    dst_stride, slot = dw * 3, dw * 3 * dh
    sentinel = np.full(slot * 64, 0xCD, np.uint8)
    dst = DevBuf.from_numpy(sentinel)
    frames = {}
    for fmt in ("nv12", "yuy2", "p010"):
        planes = frontend.yuv_planes(ref.random_frame(fmt, YW, YH, 3), fmt, YW, YH)
        bufs, strides = frontend.yuv_upload(planes, fmt, 0)
        frames[fmt] = (frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, YW, YH, "bt2020" if fmt == "p010" else "bt601"), bufs)
    bgr_dev = DevBuf.from_numpy(np.zeros((YH, YW, 3), np.uint8))
    tm = frontend.Tonemap("pq", True)

    def yuv(fmt, code, rois, n=None, slot_stride=slot, t=None):
        arr = (Roi * max(1, len(rois)))(*[Roi(*r) for r in rois])
        rc = L.hp_resize_rois_oriented_yuv(C.byref(frames[fmt][0]), t, code, arr, len(rois) if n is None else n, 0, 0, 0, 0, dst.ptr, dw, dh, dst_stride,
                                           C.c_size_t(slot_stride), None)
        return rc, L.hp_last_error().decode()

    def bgr(code, rois, n=None, slot_stride=slot):
        arr = (Roi * max(1, len(rois)))(*[Roi(*r) for r in rois])
        rc = L.hp_resize_rois_oriented_u8c3(bgr_dev.ptr, YW, YH, YW * 3, code, arr, len(rois) if n is None else n, 0, 0, 0, 0, dst.ptr, dw, dh, dst_stride,
                                            C.c_size_t(slot_stride), None)
        return rc, L.hp_last_error().decode()

    try:
        ok = (0, 0, 32, 24)
        for rc, msg in [bgr(8, [ok]), bgr(-1, [ok]), yuv("nv12", 8, [ok]), yuv("p010", 9, [ok], t=tm.h)]:
            assert rc == hp.HP_ERR_INVALID and "orientation" in msg, (rc, msg)
        # the stored rectangle's alignment: YUY2 needs an even stored x and w, any stored y and h; behind a quarter turn the upright y, h are the stored x, w
        refused = [yuv("yuy2", 0, [ok, (1, 0, 32, 24)]), yuv("yuy2", 2, [(0, 0, 31, 24)]), yuv("yuy2", 4, [(1, 0, 32, 24)]),
                   yuv("yuy2", 1, [ok, (0, 1, 32, 24)]), yuv("yuy2", 3, [(0, 0, 32, 23)]), yuv("yuy2", 7, [(0, 1, 32, 24)]),
                   yuv("nv12", 1, [(1, 0, 32, 24)]), yuv("nv12", 1, [(0, 0, 32, 23)]), yuv("p010", 5, [(0, 3, 32, 24)], t=tm.h)]
        for rc, msg in refused:
            assert rc == hp.HP_ERR_INVALID and "HP_YUV_" in msg and "region" in msg, (rc, msg)
        assert "HP_YUV_YUY2" in refused[0][1] and "region 1" in refused[0][1] and "region 1" in refused[3][1]
        # upright regions live in the upright frame: 48 x 64 behind a quarter turn
        for rc, msg in [yuv("nv12", 1, [(0, 0, 64, 48)]), yuv("nv12", 0, [(0, 0, 48, 64)]), bgr(3, [(0, 0, 64, 48)]), bgr(5, [(40, 0, 10, 10)]),
                        bgr(1, [ok], n=0), bgr(1, [ok] * 65), bgr(2, [ok, ok], slot_stride=slot - 1), yuv("nv12", 6, [ok], n=65),
                        yuv("nv12", 1, [ok], t=tm.h)]:  # the last: an 8-bit layout with a tone-map
            assert rc == hp.HP_ERR_INVALID and len(msg) > 0, (rc, msg)
        assert "HP_YUV_NV12" in yuv("nv12", 1, [ok], t=tm.h)[1]
        hp.check(L.hp_device_synchronize())
        assert np.array_equal(dst.to_numpy(np.uint8, sentinel.shape), sentinel), "a refused call wrote to the destination"
        # what the refusals were derived from is accepted
        assert yuv("yuy2", 0, [(0, 1, 32, 23)])[0] == hp.HP_OK and yuv("yuy2", 1, [(1, 0, 31, 24)])[0] == hp.HP_OK
        assert yuv("nv12", 1, [(0, 0, 48, 64)])[0] == hp.HP_OK and bgr(3, [(0, 0, 48, 64)] * 64)[0] == hp.HP_OK and yuv("p010", 5, [ok], t=tm.h)[0] == hp.HP_OK
        hp.check(L.hp_device_synchronize())
    finally:
        tm.close()
