"""CPU: the host half of the map view (include/hp_hip.h, hp_mapview_*): the taps, the palettes, the index plane and the host twins, against the tests'
own statement of DESIGN.md 1.1 "Map view" (tests/mapview_ref.py).  Byte equality everywhere; no device is needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapview_ref as ref  # noqa: E402
import overlay_ref  # noqa: E402
from test_overlay_host import COLOURS, MATRICES, RANGES  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402

FORMATS = [None] + overlay_ref.FORMATS
PAD = 10
MAPS = ref.blob_maps(7, 3, 9, 7, 5)        # three frames that differ, C = 9, 7 rows, 5 columns
BIG_MAPS = ref.blob_maps(8, 1, 4, 50, 40)  # larger than the frames below
LETTERBOX = ref.letterbox_cover(200, 150, 160, 128)


def size_of(fmt):
    return (71, 45) if fmt in (None, "i444") else (70, 46)


def colour_of(fmt):
    return COLOURS.get(fmt, ("bt601", "limited"))


def host_case(fmt, W, H, maps, index=0, seed=3, must_change=True, **kw):
    """the host twin and the numpy painter on two copies of one frame with padded rows: every byte equal, padding untouched"""
    matrix, rng = colour_of(fmt)
    got_view, got = ref.random_frame(seed, fmt, W, H, pad=PAD)
    want_view, want = ref.random_frame(seed, fmt, W, H, pad=PAD)
    before = [b.copy() for b in got]
    pal = kw.pop("pal", None)
    pal = ref.palette() if pal is None else pal
    ref.paint(want_view, maps[index], fmt, matrix, rng, pal=pal, **kw)
    frontend.draw_maps_host(got_view, maps, fmt, matrix, rng, index=index, palette=pal, **kw)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{fmt} plane {k}: {len(bad)} samples differ, first at {bad[0].tolist()}"
    views = [got_view.reshape(H, -1)] if fmt is None else got_view
    for g, b, v in zip(got, before, views):
        assert np.array_equal(g[:, v.shape[1]:], b[:, v.shape[1]:]), "row padding was written"
    changed = any(not np.array_equal(g, b) for g, b in zip(got, before))
    assert changed == must_change
    return got


# ---- taps, palettes, colours ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cover", [1.0, 0.75, LETTERBOX[1]])
@pytest.mark.parametrize("m", [1, 2, 7, 9])
@pytest.mark.parametrize("U", [1, 2, 5, 7, 70, 8192])
def test_taps_equal_double_restatement(U, m, cover):
    got = frontend.map_taps(U, m, cover)
    want = ref.taps(U, m, cover)
    assert [tuple(int(v) for v in t) for t in got] == want
    assert all(0 <= a <= b <= m - 1 and b - a <= 1 and 0 <= w <= 2048 for a, b, w in want)


def test_letterbox_cover_is_inner_over_input():
    assert LETTERBOX == (1.0, 120 / 128)
    assert frontend.map_cover(200, 150, 160, 128, True) == LETTERBOX
    assert frontend.map_cover(200, 150, 160, 128, False) == (1.0, 1.0)
    assert frontend.map_cover(150, 200, 160, 128, True) == ref.letterbox_cover(150, 200, 160, 128) != (1.0, 1.0)


@pytest.mark.parametrize("alpha", ["constant", "scaled"])
@pytest.mark.parametrize("kind", ["jet", "heat", "grey"])
def test_palettes_equal_float64_formulas(kind, alpha):
    got = frontend.map_palette(kind, alpha)
    assert got.tolist() == ref.palette(kind, alpha).tolist()
    assert got.min() >= 0 and got.max() == 255


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_yuv_palettes_equal_float64_formulas(matrix, rng, depth):
    for kind, alpha in [("jet", "scaled"), ("heat", "constant")]:
        got = frontend.map_palette(kind, alpha, matrix=matrix, range=rng, depth=depth)
        assert got.tolist() == ref.palette_yuv(ref.palette(kind, alpha), matrix, rng, depth).tolist()
        assert got[:, :3].min() >= 0 and got[:, :3].max() <= (1 << depth) - 1


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_skeleton_colours_through_the_shared_conversion(matrix, rng, depth):
    """the 19 draw_human colours pushed through the conversion the palettes use are what hp_yuv_colours returns"""
    rgba = np.zeros((256, 4), np.int32)
    rgba[:19, :3] = overlay_ref.RGB
    got = frontend.map_palette(rgba, matrix=matrix, range=rng, depth=depth)
    assert got[:19, :3].tolist() == frontend.yuv_colours(matrix, rng, depth).tolist() == overlay_ref.colours(matrix, rng, depth).tolist()


# ---- index plane ------------------------------------------------------------------------------------------------------------------------------

def special_maps():
    m = ref.blob_maps(5, 2, 12, 6, 8)
    m[1, 0, 0, 0], m[1, 1, 0, 1], m[1, 2, 0, 2], m[1, 3, 0, 3] = np.nan, np.inf, -np.inf, -3.0
    m[1, 4, 1, :] = [1.5, 2.0, 1e30, 3e38, 0.999, 1.0, 1.001, 0.5]
    m[1, :, 2, 0] = np.nan   # every channel NaN: the index is 0
    m[1, :, 2, 1] = -1.0     # every channel negative
    m[1, 5, 3, 0], m[1, 6, 3, 0] = 3e38, 3e38  # a FIELD energy that overflows to inf
    m[1, 5, 3, 1], m[1, 6, 3, 1] = np.nan, 0.3
    m[1, 10, 3, 2], m[1, 11, 3, 2] = 0.6, -0.8  # magnitude 1 exactly
    return m


@pytest.mark.parametrize("gain", [1.0, 0.5, 4.0])
@pytest.mark.parametrize("mode,channels", [("max", None), ("max", (1, 3, 5)), ("max", (4, 1, 1)), ("field", None), ("field", (0, 3, 5)), ("field", (10, 1, 1))])
def test_index_plane_equals_float32_restatement(mode, channels, gain):
    maps = special_maps()
    got = frontend.map_index_host(maps, 1, mode, channels, gain)
    want = ref.index_plane(maps[1], mode, channels, gain)
    assert got.tolist() == want.tolist()
    assert got.dtype == np.uint8
    if channels is None:
        assert want[2, 0] == 0 and (mode == "field" or want[2, 1] == 0)
        assert want.max() == 255
        assert gain > 0.5 or len(np.unique(want)) > 10  # the maximum of 12 channels saturates nearly everywhere unless the gain is low
    if mode == "max" and channels is None and gain == 1.0:
        assert want[0, 1] == 255 and want[1, 2] == 255  # +inf and 1e30 saturate


# ---- host painting ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opacity", [1.0, 0.5, 1.0 / 256])
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_twin_equals_numpy_painter(fmt, opacity):
    W, H = size_of(fmt)
    host_case(fmt, W, H, MAPS, index=1, opacity=opacity)


@pytest.mark.parametrize("fmt", FORMATS)
def test_smallest_frame_one_cell_map(fmt):
    """2 x 2 pixels - one 4:2:0 chroma block - and a 1 x 1 map: every tap is (0, 0, w)"""
    maps = np.full((1, 2, 1, 1), 0.7, np.float32)
    host_case(fmt, 2, 2, maps, opacity=1.0, pal=ref.palette("heat"))


@pytest.mark.parametrize("alpha", ["constant", "scaled"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_alpha_modes_field_mode_and_letterbox_cover(fmt, alpha):
    W, H = size_of(fmt)
    host_case(fmt, W, H, MAPS, index=2, mode="field", channels=(0, 2, 5), gain=0.5 if alpha == "scaled" else 4.0, cover=LETTERBOX,
              pal=ref.palette("jet", alpha), opacity=0.5)


@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2", "i010"])
def test_map_larger_than_the_frame(fmt):
    host_case(fmt, 16, 12, BIG_MAPS, pal=ref.palette("grey", "scaled"), opacity=1.0)


@pytest.mark.parametrize("orientation", range(8))
@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2", "p010", "i444"])
def test_every_orientation(fmt, orientation):
    W, H = size_of(fmt)
    host_case(fmt, W, H, MAPS, orientation=orientation, cover=(0.75, LETTERBOX[1]), opacity=0.5)


def test_orientations_give_different_pictures():
    W, H = size_of("nv12")
    seen = {b"".join(p.tobytes() for p in host_case("nv12", W, H, MAPS, orientation=o)) for o in range(8)}
    assert len(seen) == 8


# rois with odd offsets and odd sizes (partial chroma blocks on 4:2:0 and 4:2:2), and one at the right and bottom edge
ROIS = [(1, 1, 7, 5), (3, 2, 33, 17), (2, 3, 1, 1), (0, 5, 70, 1), (5, 0, 1, 46)]


@pytest.mark.parametrize("roi", ROIS + ["edge"])
@pytest.mark.parametrize("fmt", [None, "nv12", "i420", "nv16", "uyvy", "p010"])
def test_rois_with_partial_chroma_blocks(fmt, roi):
    W, H = size_of(fmt)
    if roi == "edge":
        roi = (W - 9, H - 7, 9, 7)
    roi = (roi[0], roi[1], min(roi[2], W - roi[0]), min(roi[3], H - roi[1]))
    host_case(fmt, W, H, MAPS, roi=roi, orientation=5, opacity=1.0, pal=ref.palette("heat"))


def test_weight_zero_leaves_the_frame_alone():
    """a palette whose every alpha is 0, and index 0 of a scaled palette: nothing is written"""
    pal = ref.palette("jet")
    pal[:, 3] = 0
    host_case("p010", 70, 46, MAPS, pal=pal, must_change=False)
    zero = np.full((1, 1, 3, 3), -1.0, np.float32)
    host_case("nv12", 70, 46, zero, pal=ref.palette("jet", "scaled"), must_change=False)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def refusal_cases():
    """(keyword arguments of draw_maps / draw_maps_host that must be refused, a word of the message)"""
    inf, nan = float("inf"), float("nan")
    bad_pal = ref.palette().copy()
    bad_pal[200, 1] = 256
    neg_pal = ref.palette().copy()
    neg_pal[3, 3] = -1
    return [(dict(opacity=0.0), "opacity"), (dict(opacity=1.01), "opacity"), (dict(opacity=nan), "opacity"),
            (dict(gain=0.0), "gain"), (dict(gain=-1.0), "gain"), (dict(gain=inf), "gain"), (dict(gain=nan), "gain"),
            (dict(cover=(0.0, 1.0)), "cover"), (dict(cover=(1.0, 1.5)), "cover"), (dict(cover=(nan, 1.0)), "cover"),
            (dict(channels=(0, 0, 1)), "cn"), (dict(channels=(0, 1, 0)), "c_step"),
            (dict(channels=(0, 10, 1)), "channels"), (dict(channels=(9, 1, 1)), "channels"), (dict(channels=(-1, 1, 1)), "channels"),
            (dict(mode="field", channels=(8, 1, 1)), "channels"), (dict(mode="field", channels=(0, 3, 4)), "channels"),
            (dict(index=-1), "frame"), (dict(orientation=8), "orientation"), (dict(orientation=-1), "orientation"),
            (dict(roi=(0, 0, 0, 5)), "roi"), (dict(roi=(0, 0, 5, -1)), "roi"), (dict(roi=(60, 0, 20, 5)), "roi"), (dict(roi=(0, 40, 5, 10)), "roi"),
            (dict(roi=(-1, 0, 5, 5)), "roi"), (dict(pal=bad_pal), "256"), (dict(pal=neg_pal), "-1")]


@pytest.mark.parametrize("fmt", [None, "nv12"])
def test_host_twin_refuses_bad_arguments(fmt):
    W, H = 70, 46
    view, backs = ref.random_frame(1, fmt, W, H, pad=PAD)
    before = [b.copy() for b in backs]
    name = "BGR" if fmt is None else "HP_YUV_NV12"
    for kw, word in refusal_cases():
        kw = dict(kw)
        pal = kw.pop("pal", "jet")
        with pytest.raises(_lib.HpError) as e:
            frontend.draw_maps_host(view, MAPS, fmt, palette=pal, **kw)
        assert e.value.code == _lib.HP_ERR_INVALID and name in str(e.value) and word in str(e.value), (kw, str(e.value))
    L = _lib.lib()
    d = frontend._map_desc(MAPS.ctypes.data, MAPS.shape[1:], 0, "max", None, 1.0, (1.0, 1.0), 0, None)
    d.mode = 2
    pal = frontend.map_palette("jet")
    big = np.zeros((4, 8200 * 3), np.uint8)
    pp = pal.ctypes.data_as(C.c_void_p)
    for args, word in [((C.c_void_p(backs[0].ctypes.data), 23, 46, 70 * 3 + PAD), "mode"), ((C.c_void_p(big.ctypes.data), 8200, 4, 8200 * 3), "8192")]:
        rc = L.hp_mapview_draw_u8c3_host(*args, C.byref(d), pp, C.c_float(0.5))
        assert rc == _lib.HP_ERR_INVALID and word in L.hp_last_error().decode()
    assert all(np.array_equal(b, a) for b, a in zip(before, backs)) and not big.any()
