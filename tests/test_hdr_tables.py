"""CPU: the host side of "HDR video in" (include/hp_hip.h) - hp_tonemap_tables against a second, independent float64 derivation
(tests/hdr_ref.py), the whole-frame host twin hp_tonemap_convert_host byte for byte against the integer rule restated in numpy,
hp_yuv_colours_hdr, and every refusal of the host-only calls.  No device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_ref  # noqa: E402
import yuv_formats_ref as ref  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402

PAIRS = [(1000.0, 203.0), (4000.0, 100.0), (600.0, 600.0)]  # (peak, white): the defaults, a brighter grade on a dimmer white, peak == white
W, H = 64, 48


@pytest.mark.parametrize("transfer", hdr_ref.TRANSFERS)
@pytest.mark.parametrize("peak,white", PAIRS)
@pytest.mark.parametrize("to_bt709", [True, False])
def test_tables_against_the_second_derivation(transfer, peak, white, to_bt709):
    A, M, O = frontend.tonemap_tables(transfer, to_bt709, peak, white)
    a, m, o = hdr_ref.tables(transfer, to_bt709, peak, white)
    # the two sides use different pow / exp implementations: a last-bit difference can flip a rint at a tie, so +-1 is the derivable bound
    assert np.abs(A.astype(np.int64) - a.astype(np.int64)).max() <= 1
    assert np.abs(O.astype(np.int64) - o.astype(np.int64)).max() <= 1
    assert np.array_equal(M, m)
    assert (M.sum(axis=1) == 4096).all()
    if to_bt709:
        assert M.tolist() == [[6801, -2407, -298], [-510, 4640, -34], [-74, -412, 4582]]
    else:
        assert M.tolist() == [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]]
    assert (np.diff(A.astype(np.int64)) >= 0).all() and (np.diff(O.astype(np.int64)) >= 0).all()
    assert set(np.diff(O.astype(np.int64)).tolist()) <= {0, 1}
    assert A[0] == 0 and len(set(A[1020:].tolist())) == 1 and O[0] == 0 and O[4095] == 255
    at_peak = hdr_ref.nits(transfer, np.minimum(np.arange(1024), 1020) / 1020.0) >= float(np.float32(peak))
    assert (A[at_peak] == 65535).all()
    if transfer == "pq":  # (the HLG signal ends at 1000 cd/m2: only a peak at or below that is reached)
        assert at_peak.any()


def _library_tables(transfer, to_bt709):
    return frontend.tonemap_tables(transfer, to_bt709)


@pytest.mark.parametrize("fmt", ["p010", "i010"])
@pytest.mark.parametrize("transfer", hdr_ref.TRANSFERS)
@pytest.mark.parametrize("to_bt709", [True, False])
def test_host_twin_is_the_integer_rule(fmt, transfer, to_bt709):
    frame = hdr_ref.ramp_frame(fmt, W, H)
    A, M, O = _library_tables(transfer, to_bt709)
    e_raw, p_raw, idx, want = hdr_ref.stages(frame, fmt, W, H, "bt2020", "limited", A, M, O, to_bt709)
    # what the frame must contain for this test to mean something: every luma value, both clamp branches of step 1 and of step 3, both ends of O
    y, _, _ = ref.unpack(frame, fmt, W, H)
    assert set(np.unique(y).tolist()) == set(range(1024))
    assert e_raw.min() < 0 and e_raw.max() > 1023
    if to_bt709:
        assert p_raw.min() < 0 and p_raw.max() > 65535
    assert idx.min() == 0 and idx.max() == 4095
    # padded strides: every plane is a view into a wider array whose padding holds other values
    planes = []
    for k, p in enumerate(frontend.yuv_planes(frame, fmt, W, H)):
        wide = np.full((p.shape[0], p.shape[1] + 3 + 2 * k), 0xA5A5, p.dtype)
        wide[:, :p.shape[1]] = p
        planes.append(wide[:, :p.shape[1]])
    got = frontend.tonemap_host(planes, fmt, "bt2020", "limited", transfer, to_bt709)
    assert np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} pixels differ"
    assert np.array_equal(got, hdr_ref.to_bgr(frame, fmt, W, H, "bt2020", "limited", A, M, O, to_bt709))


def test_host_twin_every_matrix_and_range_and_unaligned_planes():
    frame = hdr_ref.ramp_frame("i010", W, H)
    A, M, O = _library_tables("hlg", True)
    for matrix in ref.MATRICES:
        for range_ in ref.RANGES:
            want = hdr_ref.to_bgr(frame, "i010", W, H, matrix, range_, A, M, O)
            raw = np.zeros(frame.size + 1, np.uint8)  # the planes at odd addresses: host frames are read bytewise
            raw[1:] = frame
            im = frontend.yuv_image("i010", [raw.ctypes.data + 1, raw.ctypes.data + 1 + W * H * 2, raw.ctypes.data + 1 + W * H * 2 + W * H // 2],
                                    [W * 2, W, W], W, H, matrix, range_)
            d = frontend.hdr_desc("hlg")
            got = np.zeros((H, W * 3 + 5), np.uint8)
            _lib.check(_lib.lib().hp_tonemap_convert_host(C.byref(im), C.byref(d), got.ctypes.data_as(C.c_void_p), W * 3 + 5))
            assert np.array_equal(got[:, :W * 3].reshape(H, W, 3), want), (matrix, range_)
            assert (got[:, W * 3:] == 0).all()


@pytest.mark.parametrize("matrix", ref.MATRICES)
@pytest.mark.parametrize("range_", ref.RANGES)
@pytest.mark.parametrize("transfer", hdr_ref.TRANSFERS)
def test_colours_against_the_second_derivation(matrix, range_, transfer):
    for to_bt709 in (True, False):
        got = frontend.yuv_colours_hdr(matrix, range_, transfer, to_bt709)
        want = hdr_ref.colours(matrix, range_, transfer, to_bt709)
        assert np.abs(got - want).max() <= 1, (to_bt709, np.abs(got - want).max())
    assert not np.array_equal(frontend.yuv_colours_hdr(matrix, range_, transfer), frontend.yuv_colours(matrix, range_, 10))


@pytest.mark.parametrize("transfer", hdr_ref.TRANSFERS)
@pytest.mark.parametrize("range_", ref.RANGES)
@pytest.mark.parametrize("white", [203.0, 100.0])
def test_graphics_white_sits_at_white_nits(transfer, range_, white):
    """A neutral colour c (R = G = B; the table's grey, 127) has neutral chroma exactly, so its luma code alone carries it: decoded, it is
    white_nits * sRGB_EOTF(c / 255) - graphics white itself scaled by the colour's linear value - to within what one 10-bit code is worth there."""
    y, u, v = frontend.yuv_colours_hdr("bt2020", range_, transfer, True, 1000.0, white)[18]
    assert u == 512 and v == 512
    scale, off = (876.0, 64.0) if range_ == "limited" else (1023.0, 0.0)
    decode = lambda code: float(hdr_ref.nits(transfer, (code - off) / scale))
    want = white * float(hdr_ref.srgb_eotf(127 / 255.0))
    assert decode(y - 1) <= want <= decode(y + 1), (decode(y), want)
    # and a full-scale channel without the primaries step: red's R' = Y' + 2 (1 - Kr) Cr decodes to white_nits.  Y and Cr are each rounded to a
    # code, so the signal is off by at most delta = (0.5 + 2 (1 - Kr) 0.5) luma codes, and the transfer function is monotone
    yr, _, vr = frontend.yuv_colours_hdr("bt2020", range_, transfer, False, 1000.0, white)[0]
    cscale = 896.0 if range_ == "limited" else 1023.0
    r_signal = (yr - off) / scale + 2 * (1 - 0.2627) * (vr - 512) / cscale
    delta = (0.5 + (1 - 0.2627)) / scale
    assert float(hdr_ref.nits(transfer, r_signal - delta)) <= white <= float(hdr_ref.nits(transfer, r_signal + delta))


def _refused(rc):
    msg = _lib.lib().hp_last_error().decode()
    return rc == _lib.HP_ERR_INVALID and len(msg) > 0, (rc, msg)


BAD_DESCS = [dict(transfer=0), dict(transfer=3), dict(transfer=-1), dict(peak_nits=float("nan")), dict(white_nits=float("inf")),
             dict(peak_nits=float("inf")), dict(white_nits=0.0), dict(white_nits=-5.0), dict(white_nits=1200.0, peak_nits=1000.0),
             dict(peak_nits=10001.0)]


@pytest.mark.parametrize("bad", BAD_DESCS)
def test_descriptions_are_refused_by_every_host_call(bad):
    L = _lib.lib()
    d = frontend.hdr_desc("pq")
    for k, v in bad.items():
        setattr(d, k, v)
    lin, m, out = (C.c_uint16 * 1024)(), (C.c_int32 * 9)(), (C.c_uint8 * 4096)()
    frame = hdr_ref.ramp_frame("p010", W, H)
    planes = frontend.yuv_planes(frame, "p010", W, H)
    im = frontend.yuv_image("p010", [p.ctypes.data for p in planes], [p.strides[0] for p in planes], W, H, "bt2020", "limited")
    bgr = np.full((H, W, 3), 0xCD, np.uint8)
    cols = np.full((19, 3), -7, np.int32)
    humans = np.zeros(1, _lib.HUMAN_DTYPE)
    calls = [lambda: L.hp_tonemap_tables(C.byref(d), lin, m, out),
             lambda: L.hp_tonemap_convert_host(C.byref(im), C.byref(d), bgr.ctypes.data_as(C.c_void_p), W * 3),
             lambda: L.hp_yuv_colours_hdr(2, 0, C.byref(d), cols.ctypes.data_as(C.c_void_p)),
             lambda: L.hp_overlay_draw_yuv_host_hdr(C.byref(im), C.byref(d), humans.ctypes.data_as(C.c_void_p), 1, C.c_float(1.0), 0),
             lambda: L.hp_tonemap_create(C.byref(C.c_void_p()), C.byref(d)), lambda: L.hp_pipeline_set_tonemap(None, C.byref(d))]
    for i, call in enumerate(calls):
        ok, what = _refused(call())
        assert ok, (i, what)
    assert _refused(L.hp_tonemap_tables(C.byref(d), lin, m, out))[0]
    msg = L.hp_last_error().decode()
    assert ("transfer" in msg) if "transfer" in bad else ("nits" in msg), msg
    assert (bgr == 0xCD).all() and (cols == -7).all() and np.array_equal(frame, hdr_ref.ramp_frame("p010", W, H))


def test_other_refusals_of_the_host_calls():
    L = _lib.lib()
    d = frontend.hdr_desc("pq")
    lin, m, out = (C.c_uint16 * 1024)(), (C.c_int32 * 9)(), (C.c_uint8 * 4096)()
    bgr = np.zeros((H, W, 3), np.uint8)
    dst = bgr.ctypes.data_as(C.c_void_p)
    assert _refused(L.hp_tonemap_tables(None, lin, m, out))[0]
    for args in [(None, m, out), (lin, None, out), (lin, m, None)]:
        assert _refused(L.hp_tonemap_tables(C.byref(d), *args))[0]
    p010 = frontend.yuv_planes(hdr_ref.ramp_frame("p010", W, H), "p010", W, H)
    good = frontend.yuv_image("p010", [p.ctypes.data for p in p010], [p.strides[0] for p in p010], W, H, "bt2020", "limited")
    assert L.hp_tonemap_convert_host(C.byref(good), C.byref(d), dst, W * 3) == _lib.HP_OK
    assert _refused(L.hp_tonemap_convert_host(None, C.byref(d), dst, W * 3))[0]
    assert _refused(L.hp_tonemap_convert_host(C.byref(good), None, dst, W * 3))[0]
    assert _refused(L.hp_tonemap_convert_host(C.byref(good), C.byref(d), None, W * 3))[0]
    assert _refused(L.hp_tonemap_convert_host(C.byref(good), C.byref(d), dst, W * 3 - 1))[0]
    # an 8-bit layout: the message names the format
    for fmt in ["nv12", "i420", "nv16", "i422", "yuy2", "uyvy", "i444"]:
        planes = frontend.yuv_planes(ref.random_frame(fmt, W, H, 1), fmt, W, H)
        im = frontend.yuv_image(fmt, [p.ctypes.data for p in planes], [p.strides[0] for p in planes], W, H, "bt2020", "limited")
        ok, (rc, msg) = _refused(L.hp_tonemap_convert_host(C.byref(im), C.byref(d), dst, W * 3))
        assert ok and "HP_YUV_" + fmt.upper() in msg, (fmt, rc, msg)
        humans = np.zeros(1, _lib.HUMAN_DTYPE)
        # (the overlay paints 8-bit frames of an HDR stream as before: nothing to refuse there)
        assert L.hp_overlay_draw_yuv_host_hdr(C.byref(im), C.byref(d), humans.ctypes.data_as(C.c_void_p), 1, C.c_float(1.0), 0) == _lib.HP_OK
    # what the SDR description checks refuse: matrix, range, size, a short stride, a null plane
    for field, value in [("matrix", 3), ("range", 2), ("width", 63), ("height", 0)]:
        im = frontend.yuv_image("p010", [p.ctypes.data for p in p010], [p.strides[0] for p in p010], W, H, "bt2020", "limited")
        setattr(im, field, value)
        assert _refused(L.hp_tonemap_convert_host(C.byref(im), C.byref(d), dst, W * 3))[0], field
    im = frontend.yuv_image("p010", [p.ctypes.data for p in p010], [W * 2 - 2, W * 2], W, H, "bt2020", "limited")
    assert _refused(L.hp_tonemap_convert_host(C.byref(im), C.byref(d), dst, W * 3))[0]
    im = frontend.yuv_image("p010", [p010[0].ctypes.data, 0], [W * 2, W * 2], W, H, "bt2020", "limited")
    im.plane[1] = None
    assert _refused(L.hp_tonemap_convert_host(C.byref(im), C.byref(d), dst, W * 3))[0]
    cols = np.zeros((19, 3), np.int32)
    assert _refused(L.hp_yuv_colours_hdr(3, 0, C.byref(d), cols.ctypes.data_as(C.c_void_p)))[0]
    assert _refused(L.hp_yuv_colours_hdr(2, 2, C.byref(d), cols.ctypes.data_as(C.c_void_p)))[0]
    assert _refused(L.hp_yuv_colours_hdr(2, 0, None, cols.ctypes.data_as(C.c_void_p)))[0]
    assert _refused(L.hp_yuv_colours_hdr(2, 0, C.byref(d), None))[0]
    # handles: null everywhere (nothing here needs a device - the checks come before any launch)
    assert _refused(L.hp_tonemap_create(None, C.byref(d)))[0]
    h = C.c_void_p()
    assert _refused(L.hp_tonemap_create(C.byref(h), None))[0] and not h
    assert _refused(L.hp_resize_yuv_hdr(C.byref(good), None, dst, 32, 32, 96, None))[0]
    assert _refused(L.hp_letterbox_yuv_hdr(C.byref(good), None, dst, 32, 32, 96, 0, 0, 0, None))[0]
    roi = _lib.Roi(0, 0, 32, 32)
    assert _refused(L.hp_resize_rois_yuv_hdr(C.byref(good), None, C.byref(roi), 1, 0, 0, 0, 0, dst, 32, 32, 96, C.c_size_t(96 * 32), None))[0]
    assert _refused(L.hp_overlay_set_transfer(None, C.byref(d)))[0]
    assert _refused(L.hp_pipeline_set_tonemap(None, C.byref(d)))[0]


def test_host_overlay_draws_hdr_colours():
    """hp_overlay_draw_yuv_host_hdr paints what hp_overlay_draw_yuv_host paints, with hp_yuv_colours_hdr's table: the covered samples are the
    same, their values are the HDR codes."""
    humans = np.zeros(1, _lib.HUMAN_DTYPE)
    for k, (x, y) in enumerate([(0.5, 0.2), (0.5, 0.4), (0.3, 0.45), (0.25, 0.7)]):
        humans[0]["parts"][k] = (1, x, y, 1.0)
    humans[0]["score"] = 1.0
    for fmt in ("p010", "i010"):
        base = ref.pack(np.full((H, W), 300), np.full((H // 2, W // 2), 512), np.full((H // 2, W // 2), 512), fmt)
        sdr = [p.copy() for p in frontend.yuv_planes(base, fmt, W, H)]
        hdr = [p.copy() for p in frontend.yuv_planes(base, fmt, W, H)]
        off = [p.copy() for p in frontend.yuv_planes(base, fmt, W, H)]
        frontend.draw_humans_host(sdr, humans, fmt, "bt2020", "limited")
        frontend.draw_humans_host(hdr, humans, fmt, "bt2020", "limited", hdr=frontend.hdr_desc("pq"))
        shift = 6 if fmt == "p010" else 0
        cs, ch = frontend.yuv_colours("bt2020", "limited", 10), frontend.yuv_colours_hdr("bt2020", "limited", "pq")
        painted = sdr[0] != off[0]
        assert painted.any() and np.array_equal(painted, hdr[0] != off[0])
        assert set(np.unique(sdr[0][painted]).tolist()) <= {int(c) << shift for c in cs[:, 0]}
        assert set(np.unique(hdr[0][painted]).tolist()) <= {int(c) << shift for c in ch[:, 0]}
        assert not np.array_equal(sdr[0], hdr[0])
