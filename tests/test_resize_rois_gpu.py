"""GPU: hp_resize_rois_u8c3 / hp_resize_rois_yuv (resize_rois.hip).  The parity contract: slot i == the existing per-frame call on region i
cut out into a frame of its own (uploaded on its own), byte for byte, and == the CPU oracle on the cut-out; bytes of the destination
that belong to no slot's picture keep their pre-fill.  Refused calls launch nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_formats_ref as ref  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from hyperpose_amd._lib import DevBuf, Roi  # noqa: E402
from oracle import loader  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = (3, 250, 77)
PREFILL = 0xA5


def _run(src, rois, dw, dh, keep_ratio, **kw):
    """The fused call into a pre-filled destination with padded rows and padded slots: ([n, dh, dw, 3] pictures, every other byte)."""
    n = len(rois)
    dst_stride, slot_stride = dw * 3 + 7, (dw * 3 + 7) * dh + 11
    dst = DevBuf.from_numpy(np.full(n * slot_stride, PREFILL, np.uint8))
    frontend.resize_rois(src, rois, dst, dw, dh, keep_ratio, FILL, dst_stride=dst_stride, slot_stride=slot_stride, **kw)
    frontend.check(frontend.lib().hp_device_synchronize())
    flat = dst.to_numpy(np.uint8, (n, slot_stride))
    rows = flat[:, :dh * dst_stride].reshape(n, dh, dst_stride)
    return rows[:, :, :dw * 3].reshape(n, dh, dw, 3).copy(), np.concatenate([rows[:, :, dw * 3:].ravel(), flat[:, dh * dst_stride:].ravel()])


def _assert_slot(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}"


# ---- BGR ------------------------------------------------------------------------------------------------------------------------------

SW, SH, PITCH = 97, 61, 97 * 3 + 5
BASE = [(0, 0, 97, 61),                      # the whole frame
        (5, 7, 1, 1), (96, 60, 1, 1),        # one pixel, one in the last corner
        (10, 10, 2, 2),
        (20, 11, 48, 40),                    # the slot's size: copy mode
        (1, 1, 96, 60),                      # letter-boxed into 48 x 40 the inner size is 48 x 30: area mode
        (90, 8, 7, 53),                      # a sliver, on the right edge
        (0, 10, 30, 20), (40, 0, 30, 20), (67, 20, 30, 20), (30, 41, 30, 20),  # touching each edge
        (33, 17, 41, 29), (33, 17, 41, 29),  # twice the same
        (0, 0, 96, 60), (49, 21, 48, 40), (0, 60, 97, 1), (96, 0, 1, 61)]
assert len(BASE) == 17  # one more than a launch carries


@pytest.fixture(scope="module")
def bgr(hp):
    img = np.random.default_rng(21).integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    padded = np.full((SH, PITCH), 0x5A, np.uint8)
    padded[:, :SW * 3] = img.reshape(SH, SW * 3)
    return img, DevBuf.from_numpy(padded)


def _check_bgr(bgr, rois, dw, dh, keep_ratio):
    img, dev = bgr
    got, rest = _run(dev, rois, dw, dh, keep_ratio, sw=SW, sh=SH, src_stride=PITCH)
    assert (rest == PREFILL).all(), "bytes outside the slots' pictures were written"
    done = {}
    for i, (x, y, w, h) in enumerate(rois):
        if (x, y, w, h) not in done:
            cut = np.ascontiguousarray(img[y:y + h, x:x + w])
            oracle = loader.letterbox_u8(cut, dw, dh, bgcolor=FILL) if keep_ratio else loader.resize_linear_u8(cut, dw, dh)
            done[(x, y, w, h)] = (frontend.resize_host(cut, dw, dh, keep_ratio, FILL), oracle)
        device, oracle = done[(x, y, w, h)]
        _assert_slot(got[i], device, f"region {i} {(x, y, w, h)} keep_ratio={keep_ratio} vs the per-frame kernel")
        _assert_slot(got[i], oracle, f"region {i} {(x, y, w, h)} keep_ratio={keep_ratio} vs the CPU oracle")


@pytest.mark.parametrize("keep_ratio", [False, True])
def test_bgr_regions_equal_the_per_frame_call_on_the_cut_out(hp, bgr, keep_ratio):
    _check_bgr(bgr, BASE, 48, 40, keep_ratio)
    _check_bgr(bgr, BASE[:1], 48, 40, keep_ratio)
    _check_bgr(bgr, BASE[:16], 48, 40, keep_ratio)
    # half the size: (1, 1, 96, 60) -> 24 x 20 and (20, 11, 48, 40) -> 24 x 20 are the area mode without a letterbox too
    _check_bgr(bgr, [(20, 11, 48, 40), (1, 1, 96, 60), (0, 0, 24, 20), (73, 41, 24, 20)], 24, 20, keep_ratio)


@pytest.mark.parametrize("keep_ratio", [False, True])
def test_bgr_64_regions(hp, bgr, keep_ratio):
    rng = np.random.default_rng(22)
    rois = []
    for _ in range(64):
        w, h = int(rng.integers(1, SW + 1)), int(rng.integers(1, SH + 1))
        rois.append((int(rng.integers(0, SW - w + 1)), int(rng.integers(0, SH - h + 1)), w, h))
    _check_bgr(bgr, rois, 48, 40, keep_ratio)


# ---- YUV ------------------------------------------------------------------------------------------------------------------------------

YW, YH = 64, 48
# aligned to every layout (even everything), the four corners among them; 24 x 20 slots: copy, area and linear modes
YUV_ROIS = [(0, 0, 64, 48), (0, 0, 32, 24), (32, 0, 32, 24), (0, 24, 32, 24), (32, 24, 32, 24), (2, 2, 48, 40), (16, 8, 24, 20), (62, 46, 2, 2),
            (0, 0, 2, 2), (10, 6, 40, 36), (0, 46, 64, 2), (62, 0, 2, 48)]
PITCHES = {2: (34, 6), 3: (2, 70, 6), 1: (26,)}  # per plane count; the U and the V plane of a planar frame differ in pitch


def _sub_planes(planes, fmt, x, y, w, h):
    n, _, sx, sy = ref.LAYOUT[fmt]
    if n == 1:
        return [planes[0][y:y + h, 2 * x:2 * (x + w)]]
    cy0, cy1, cx0, cx1 = y >> sy, (y + h) >> sy, x >> sx, (x + w) >> sx
    if n == 2:
        return [planes[0][y:y + h, x:x + w], planes[1][cy0:cy1, 2 * cx0:2 * cx1]]
    return [planes[0][y:y + h, x:x + w], planes[1][cy0:cy1, cx0:cx1], planes[2][cy0:cy1, cx0:cx1]]


@pytest.mark.parametrize("fmt", ref.FORMATS)
@pytest.mark.parametrize("matrix,range_", [("bt601", "limited"), ("bt709", "full")])
def test_yuv_regions_equal_the_per_frame_call_on_the_sub_planes(hp, fmt, matrix, range_):
    frame = ref.random_frame(fmt, YW, YH, 31 + ref.FORMATS.index(fmt))
    planes = frontend.yuv_planes(frame, fmt, YW, YH)
    bufs, strides = frontend.yuv_upload(planes, fmt, PITCHES[len(planes)], fill=0x5A)
    im = frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, YW, YH, matrix, range_)
    ax, ay = frontend.yuv_roi_alignment(fmt)
    rois = YUV_ROIS + ([(3, 0, 21, 48)] if ax == 1 else []) + ([(4, 5, 20, 33)] if ay == 1 else [])
    for keep_ratio in (False, True):
        got, rest = _run(im, rois, 24, 20, keep_ratio)
        assert (rest == PREFILL).all(), "bytes outside the slots' pictures were written"
        for i, (x, y, w, h) in enumerate(rois):
            sub = [np.ascontiguousarray(p) for p in _sub_planes(planes, fmt, x, y, w, h)]
            what = f"{fmt} {matrix} {range_} region {i} {(x, y, w, h)} keep_ratio={keep_ratio}"
            _assert_slot(got[i], frontend.resize_yuv_host(sub, 24, 20, fmt, matrix, range_, keep_ratio, FILL, pitch=2), what + " vs the per-frame kernel")
            cut = ref.to_bgr(np.concatenate([p.view(np.uint8).ravel() for p in sub]), fmt, w, h, matrix, range_)
            oracle = loader.letterbox_u8(cut, 24, 20, bgcolor=FILL) if keep_ratio else loader.resize_linear_u8(cut, 24, 20)
            _assert_slot(got[i], oracle, what + " vs the CPU conversion and oracle")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing(hp):
    L = hp.lib()
    dw, dh, n_max = 16, 12, 64
    dst_stride, slot = dw * 3, dw * 3 * dh
    sentinel = np.full(slot * n_max, 0xCD, np.uint8)
    dst = DevBuf.from_numpy(sentinel)
    frames = {}
    for fmt in ("nv12", "yuy2", "i444"):
        planes = frontend.yuv_planes(ref.random_frame(fmt, YW, YH, 3), fmt, YW, YH)
        bufs, strides = frontend.yuv_upload(planes, fmt, 0)
        frames[fmt] = (frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, YW, YH), bufs)
    bgr_dev = DevBuf.from_numpy(np.zeros((YH, YW, 3), np.uint8))

    def yuv(fmt, rois, n=None, slot_stride=slot, image=None):
        arr = (Roi * max(1, len(rois)))(*[Roi(*r) for r in rois])
        rc = L.hp_resize_rois_yuv(C.byref(image or frames[fmt][0]), arr, len(rois) if n is None else n, 0, 0, 0, 0, dst.ptr, dw, dh, dst_stride,
                                  C.c_size_t(slot_stride), None)
        return rc, L.hp_last_error().decode()

    def bgr(rois, n=None, slot_stride=slot):
        arr = (Roi * max(1, len(rois)))(*[Roi(*r) for r in rois])
        rc = L.hp_resize_rois_u8c3(bgr_dev.ptr, YW, YH, YW * 3, arr, len(rois) if n is None else n, 0, 0, 0, 0, dst.ptr, dw, dh, dst_stride,
                                   C.c_size_t(slot_stride), None)
        return rc, L.hp_last_error().decode()

    ok = (0, 0, 32, 24)
    refused = [yuv("nv12", [ok, (3, 0, 32, 24)]),                 # an odd x
               yuv("nv12", [(0, 5, 32, 24)]),                     # an odd y
               yuv("nv12", [(0, 0, 31, 24)]), yuv("nv12", [(0, 0, 32, 23)]), yuv("yuy2", [(1, 0, 32, 24)]),
               yuv("nv12", [ok, (34, 0, 32, 24)]),                # one column outside
               yuv("nv12", [(0, 26, 32, 24)]), yuv("nv12", [(-2, 0, 32, 24)]), yuv("nv12", [(0, 0, 0, 24)]), yuv("i444", [(33, 0, 32, 24)]),
               yuv("nv12", [ok], n=0), yuv("nv12", [ok] * 65), yuv("nv12", [ok], n=-1),
               yuv("nv12", [ok, ok], slot_stride=slot - 1)]
    for rc, msg in refused:
        assert rc == hp.HP_ERR_INVALID and "HP_YUV_" in msg, (rc, msg)
    assert "HP_YUV_NV12" in refused[0][1] and "region 1" in refused[0][1]
    assert "HP_YUV_YUY2" in refused[4][1] and "region 0" in refused[4][1]
    bad_frame = frontend.yuv_image("nv12", [frames["nv12"][1][0].ptr, frames["nv12"][1][1].ptr], [YW - 2, YW], YW, YH)
    rc, msg = yuv("nv12", [ok], image=bad_frame)  # what hp_resize_yuv rejects for the frame itself
    assert rc == hp.HP_ERR_INVALID and "HP_YUV_NV12" in msg
    for rc, msg in [bgr([(33, 0, 32, 24)]), bgr([(0, 25, 32, 24)]), bgr([ok], n=0), bgr([ok] * 65), bgr([ok, ok], slot_stride=slot - 1), bgr([(0, 0, 32, 0)])]:
        assert rc == hp.HP_ERR_INVALID and len(msg) > 0, (rc, msg)
    hp.check(L.hp_device_synchronize())
    assert np.array_equal(dst.to_numpy(np.uint8, sentinel.shape), sentinel), "a refused call wrote to the destination"
    # what the refusals were derived from is accepted: an odd y is fine where chroma has full height, odd everything on 4:4:4
    assert yuv("nv12", [ok, (32, 24, 32, 24)])[0] == hp.HP_OK and yuv("yuy2", [(0, 5, 32, 24)])[0] == hp.HP_OK
    assert yuv("i444", [(31, 5, 33, 43)])[0] == hp.HP_OK and yuv("nv12", [ok] * 64)[0] == hp.HP_OK and bgr([(32, 24, 32, 24)] * 64)[0] == hp.HP_OK
    hp.check(L.hp_device_synchronize())
