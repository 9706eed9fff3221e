"""GPU: hp_resize_yuv_hdr / hp_letterbox_yuv_hdr / hp_resize_rois_yuv_hdr (resize_yuv_hdr.hip) and the overlay on HDR frames.  Every picture is
byte-equal to "tests/hdr_ref.to_bgr with the library's own tables, then the restated cv::resize / non_scaling_resize (oracle/resize_oracle.cpp)":
the bar every other feed of the front end meets, zero mismatches allowed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_ref  # noqa: E402
import yuv_formats_ref as ref  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from hyperpose_amd._lib import HUMAN_DTYPE, DevBuf  # noqa: E402
from oracle import loader  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
FILL = (3, 250, 77)
PREFILL = 0xA5
MATRIX, RANGE = "bt2020", "limited"
# (dw, dh, letterbox): linear, the exact 2 x area case, copy, up-scale, letter-box with a non-black border
CASES = [(40, 36, False), (32, 24, False), (64, 48, False), (100, 70, False), (48, 48, True)]
COMBOS = [(f, t, p) for f in ("p010", "i010") for t in hdr_ref.TRANSFERS for p in (True, False)]


def _assert_same(got, want, what=""):
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ, first at {bad[0].tolist()}"


@pytest.fixture(scope="module")
def world(hp):
    """Per (format, transfer, to_bt709): the frame, its planes, the handle and the CPU-converted BGR frame (computed once, never written)."""
    out = {}
    for fmt, transfer, to_bt709 in COMBOS:
        frame = hdr_ref.ramp_frame(fmt, W, H)
        A, M, O = frontend.tonemap_tables(transfer, to_bt709)
        bgr = hdr_ref.to_bgr(frame, fmt, W, H, MATRIX, RANGE, A, M, O, to_bt709)
        bgr.setflags(write=False)
        out[(fmt, transfer, to_bt709)] = (frame, frontend.yuv_planes(frame, fmt, W, H), frontend.Tonemap(transfer, to_bt709), bgr)
    yield out
    for _, _, tm, _ in out.values():
        tm.close()


def _expect(bgr, dw, dh, letterbox):
    return loader.letterbox_u8(bgr, dw, dh, bgcolor=FILL) if letterbox else loader.resize_linear_u8(bgr, dw, dh)


@pytest.mark.parametrize("fmt,transfer,to_bt709", COMBOS)
def test_per_frame_calls_equal_convert_then_resize(hp, world, fmt, transfer, to_bt709):
    _, planes, tm, bgr = world[(fmt, transfer, to_bt709)]
    for dw, dh, letterbox in CASES:
        got = frontend.resize_yuv_host(planes, dw, dh, fmt, MATRIX, RANGE, letterbox, FILL, tonemap=tm)
        _assert_same(got, _expect(bgr, dw, dh, letterbox), f"{fmt} {transfer} to_bt709={to_bt709} -> {dw}x{dh} letterbox={letterbox}")
    # and it is not what the SDR kernel makes of the same samples
    assert not np.array_equal(frontend.resize_yuv_host(planes, 64, 48, fmt, MATRIX, RANGE, tonemap=tm), frontend.resize_yuv_host(planes, 64, 48, fmt, MATRIX, RANGE))


def test_host_twin_equals_the_copy_mode_kernel(hp, world):
    for (fmt, transfer, to_bt709), (_, planes, tm, bgr) in world.items():
        assert np.array_equal(frontend.tonemap_host(planes, fmt, MATRIX, RANGE, transfer, to_bt709), bgr)


@pytest.mark.parametrize("fmt,pitch", [("p010", 34), ("p010", (2, 6)), ("i010", 26), ("i010", (2, 70, 6)), ("i010", (4, 0, 128))])
def test_padded_pitch_and_a_v_pitch_of_its_own(hp, world, fmt, pitch):
    _, planes, tm, bgr = world[(fmt, "pq", True)]
    for dw, dh, letterbox in CASES:
        got = frontend.resize_yuv_host(planes, dw, dh, fmt, MATRIX, RANGE, letterbox, FILL, pitch=pitch, tonemap=tm)
        _assert_same(got, _expect(bgr, dw, dh, letterbox), f"{fmt} pitch {pitch} -> {dw}x{dh}")


def test_every_matrix_and_range(hp, world):
    frame, planes, tm, _ = world[("i010", "hlg", True)]
    A, M, O = frontend.tonemap_tables("hlg", True)
    for matrix in ref.MATRICES:
        for range_ in ref.RANGES:
            bgr = hdr_ref.to_bgr(frame, "i010", W, H, matrix, range_, A, M, O)
            for dw, dh in [(64, 48), (40, 36)]:
                _assert_same(frontend.resize_yuv_host(planes, dw, dh, "i010", matrix, range_, tonemap=tm), loader.resize_linear_u8(bgr, dw, dh), f"{matrix} {range_}")


def test_low_six_bits_of_p010_are_ignored(hp, world):
    frame, planes, tm, bgr = world[("p010", "pq", True)]
    words = frame.view("<u2")
    dirty = (words | np.random.default_rng(8).integers(0, 64, words.size).astype("<u2")).astype("<u2")
    assert (dirty != words).mean() > 0.9
    dirty_planes = frontend.yuv_planes(dirty.view(np.uint8), "p010", W, H)
    for dw, dh, letterbox in CASES:
        got = frontend.resize_yuv_host(dirty_planes, dw, dh, "p010", MATRIX, RANGE, letterbox, FILL, tonemap=tm)
        _assert_same(got, _expect(bgr, dw, dh, letterbox), f"P016 -> {dw}x{dh}")


def test_other_peak_and_white(hp):
    frame = hdr_ref.ramp_frame("p010", W, H)
    planes = frontend.yuv_planes(frame, "p010", W, H)
    for peak, white in [(4000.0, 100.0), (600.0, 600.0)]:
        tm = frontend.Tonemap("pq", True, peak, white)
        A, M, O = frontend.tonemap_tables("pq", True, peak, white)
        bgr = hdr_ref.to_bgr(frame, "p010", W, H, MATRIX, RANGE, A, M, O)
        _assert_same(frontend.resize_yuv_host(planes, 40, 36, "p010", MATRIX, RANGE, tonemap=tm), loader.resize_linear_u8(bgr, 40, 36), f"{peak} {white}")
        tm.close()


# ---- regions ------------------------------------------------------------------------------------------------------------------------------

# origins and sizes are multiples of 2; 24 x 20 slots: copy (24 x 20), area (48 x 40) and linear modes, the corners, one more than a launch
ROIS = [(0, 0, 64, 48), (0, 0, 32, 24), (32, 0, 32, 24), (0, 24, 32, 24), (32, 24, 32, 24), (2, 2, 48, 40), (16, 8, 24, 20), (62, 46, 2, 2),
        (0, 0, 2, 2), (10, 6, 40, 36), (0, 46, 64, 2), (62, 0, 2, 48), (8, 4, 48, 40), (40, 28, 24, 20), (20, 10, 30, 28), (6, 2, 52, 44),
        (2, 2, 48, 40)]
assert len(ROIS) == 17


def _sub_planes(planes, fmt, x, y, w, h):
    if len(planes) == 2:
        return [planes[0][y:y + h, x:x + w], planes[1][y // 2:(y + h) // 2, x:x + w]]
    return [planes[0][y:y + h, x:x + w], planes[1][y // 2:(y + h) // 2, x // 2:(x + w) // 2], planes[2][y // 2:(y + h) // 2, x // 2:(x + w) // 2]]


@pytest.mark.parametrize("fmt,transfer,to_bt709", [("p010", "pq", True), ("i010", "hlg", False)])
@pytest.mark.parametrize("n", [3, 17])
def test_regions_equal_the_per_frame_call_on_the_sub_planes(hp, world, fmt, transfer, to_bt709, n):
    _, planes, tm, bgr = world[(fmt, transfer, to_bt709)]
    bufs, strides = frontend.yuv_upload(planes, fmt, (34, 6) if fmt == "p010" else (2, 70, 6), fill=0x5A)
    im = frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, W, H, MATRIX, RANGE)
    rois = ROIS[5:8] if n == 3 else ROIS
    dw, dh = 24, 20
    dst_stride, slot_stride = dw * 3 + 7, (dw * 3 + 7) * dh + 11
    for keep_ratio in (False, True):
        dst = DevBuf.from_numpy(np.full(n * slot_stride, PREFILL, np.uint8))
        frontend.resize_rois(im, rois, dst, dw, dh, keep_ratio, FILL, dst_stride=dst_stride, slot_stride=slot_stride, tonemap=tm)
        hp.check(hp.lib().hp_device_synchronize())
        flat = dst.to_numpy(np.uint8, (n, slot_stride))
        rows = flat[:, :dh * dst_stride].reshape(n, dh, dst_stride)
        assert (rows[:, :, dw * 3:] == PREFILL).all() and (flat[:, dh * dst_stride:] == PREFILL).all(), "bytes outside the slots' pictures were written"
        got = rows[:, :, :dw * 3].reshape(n, dh, dw, 3)
        for i, (x, y, w, h) in enumerate(rois):
            what = f"{fmt} {transfer} region {i} {(x, y, w, h)} keep_ratio={keep_ratio}"
            sub = [np.ascontiguousarray(p) for p in _sub_planes(planes, fmt, x, y, w, h)]
            _assert_same(got[i], frontend.resize_yuv_host(sub, dw, dh, fmt, MATRIX, RANGE, keep_ratio, FILL, pitch=2, tonemap=tm), what + " vs the per-frame kernel")
            _assert_same(got[i], _expect(np.ascontiguousarray(bgr[y:y + h, x:x + w]), dw, dh, keep_ratio), what + " vs the CPU conversion and oracle")


# ---- refusals on the device ---------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing(hp, world):
    L = hp.lib()
    tm = world[("p010", "pq", True)][2]
    src = DevBuf(W * H * 6 + 16)
    sentinel = np.full(3 * 32 * 32 * 3, 0xCD, np.uint8)
    dst = DevBuf.from_numpy(sentinel)
    base = src.ptr.value
    p1, p2 = base + W * H * 2, base + W * H * 4
    rois = (hp.Roi * 3)(hp.Roi(0, 0, 32, 24), hp.Roi(2, 2, 48, 40), hp.Roi(32, 24, 32, 24))

    def calls(fmt, planes, strides, handle=tm.h, **raw):
        im = frontend.yuv_image(fmt, planes, strides, W, H, MATRIX, RANGE)
        for k, v in raw.items():
            setattr(im, k, v)
        out = [L.hp_resize_yuv_hdr(C.byref(im), handle, dst.ptr, 32, 32, 96, None),
               L.hp_letterbox_yuv_hdr(C.byref(im), handle, dst.ptr, 32, 32, 96, 1, 2, 3, None),
               L.hp_resize_rois_yuv_hdr(C.byref(im), handle, rois, 3, 0, 1, 2, 3, dst.ptr, 32, 32, 96, C.c_size_t(96 * 32), None)]
        return out, L.hp_last_error().decode()

    good = {"p010": ([base, p1], [W * 2, W * 2]), "i010": ([base, p1, p2], [W * 2, W, W])}
    eight = {"nv12": ([base, p1], [W, W]), "i420": ([base, p1, p2], [W, W // 2, W // 2]), "yuy2": ([base], [W * 2]), "i444": ([base, p1, p2], [W, W, W])}
    bad = []
    for fmt, (planes, strides) in eight.items():  # an 8-bit format: the message names it
        rcs, msg = calls(fmt, planes, strides)
        assert "HP_YUV_" + fmt.upper() in msg, msg
        bad += rcs
    for fmt, (planes, strides) in good.items():
        bad += calls(fmt, [planes[0] + 1] + planes[1:], strides)[0]              # an odd plane pointer
        bad += calls(fmt, planes[:1] + [planes[1] + 1] + planes[2:], strides)[0]
        bad += calls(fmt, planes, [strides[0] + 1] + strides[1:])[0]             # an odd stride
        bad += calls(fmt, planes, strides, handle=None)[0]                        # a null handle
        bad += calls(fmt, planes, [strides[0] - 2] + strides[1:])[0]             # what the SDR twin refuses: a short stride, a bad matrix, an odd width
        bad += calls(fmt, planes, strides, matrix=3)[0]
        bad += calls(fmt, planes, strides, width=63)[0]
    assert bad and all(rc == hp.HP_ERR_INVALID for rc in bad), bad
    assert len(L.hp_last_error()) > 0
    # region rules of the SDR twin: an odd origin, a region outside the frame, too many regions, a slot stride smaller than a slot
    im = frontend.yuv_image("p010", *good["p010"], W, H, MATRIX, RANGE)
    for r, n, ss in [(hp.Roi(1, 0, 32, 24), 1, 96 * 32), (hp.Roi(40, 0, 32, 24), 1, 96 * 32), (rois[0], 65, 96 * 32), (rois[0], 1, 96 * 32 - 1)]:
        arr = (hp.Roi * 65)(*([r] * 65))
        assert L.hp_resize_rois_yuv_hdr(C.byref(im), tm.h, arr, n, 0, 0, 0, 0, dst.ptr, 32, 32, 96, C.c_size_t(ss), None) == hp.HP_ERR_INVALID
    hp.check(L.hp_device_synchronize())
    assert np.array_equal(dst.to_numpy(np.uint8, sentinel.shape), sentinel), "a refused call wrote to the destination"
    for fmt, (planes, strides) in good.items():  # and the descriptions the refusals were derived from are accepted
        assert calls(fmt, planes, strides)[0] == [hp.HP_OK] * 3, fmt
    hp.check(L.hp_device_synchronize())


# ---- overlay ------------------------------------------------------------------------------------------------------------------------------

def _human():
    hs = np.zeros(1, HUMAN_DTYPE)
    for k, (x, y) in enumerate([(0.5, 0.15), (0.5, 0.35), (0.3, 0.4), (0.2, 0.6), (0.15, 0.8), (0.7, 0.4), (0.8, 0.6), (0.85, 0.8)]):
        hs[0]["parts"][k] = (1, x, y, 1.0)
    hs[0]["score"] = 1.0
    return hs


@pytest.mark.parametrize("transfer", hdr_ref.TRANSFERS)
def test_overlay_draws_hdr_colours_on_a_device_frame(hp, transfer):
    frame = ref.pack(np.full((H, W), 300), np.full((H // 2, W // 2), 512), np.full((H // 2, W // 2), 512), "p010")
    humans = _human()
    host_sdr = [p.copy() for p in frontend.yuv_planes(frame, "p010", W, H)]
    host_hdr = [p.copy() for p in frontend.yuv_planes(frame, "p010", W, H)]
    frontend.draw_humans_host(host_sdr, humans, "p010", MATRIX, RANGE, opacity=0.75)
    frontend.draw_humans_host(host_hdr, humans, "p010", MATRIX, RANGE, opacity=0.75, hdr=frontend.hdr_desc(transfer))
    assert not np.array_equal(host_sdr[0], host_hdr[0])
    ov = frontend.Overlay(4)

    def device():
        bufs, strides = frontend.yuv_upload(frontend.yuv_planes(frame, "p010", W, H), "p010", 6, fill=0x5A)
        im = frontend.yuv_image("p010", [b.ptr for b in bufs], strides, W, H, MATRIX, RANGE)
        frontend.draw_humans(im, humans, opacity=0.75, overlay=ov)
        hp.check(hp.lib().hp_device_synchronize())
        out = []
        for b, s, p in zip(bufs, strides, host_sdr):
            raw = b.to_numpy(np.uint8, (p.shape[0], s))
            assert (raw[:, s - 6:] == 0x5A).all()
            out.append(np.ascontiguousarray(raw[:, :s - 6]).view("<u2"))
        return out

    ov.set_transfer(transfer)
    for got, want in zip(device(), host_hdr):
        assert np.array_equal(got, want)
    ov.set_transfer(None)
    for got, want in zip(device(), host_sdr):
        assert np.array_equal(got, want)
    with pytest.raises(hp.HpError):
        ov.set_transfer("pq", white_nits=-1.0)
    ov.close()
