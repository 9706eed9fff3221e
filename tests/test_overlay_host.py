"""CPU: the host half of the overlay renderer (include/hp_hip.h, hp_overlay_*): the primitive list, the YUV colour tables and the host twins,
against the tests' own numpy statement of DESIGN.md 1.1 (tests/overlay_ref.py).  Byte equality everywhere; no device is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as ref  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402

MATRICES, RANGES = ["bt601", "bt709", "bt2020"], ["limited", "full"]


def special_humans():
    """parts missing, a human with no parts, coordinates below 0 and above 1, NaN / inf, an end point beyond the drop range"""
    hs = ref.make_humans([
        {0: (0.5, 0.2), 1: (0.5, 0.35), 2: (0.4, 0.36), 5: (0.6, 0.36), 8: (0.45, 0.6), 11: (0.55, 0.6)},       # parts missing
        {},                                                                                                   # no parts at all
        {1: (-0.05, 0.5), 2: (0.1, 0.45), 3: (0.08, 1.08), 5: (1.04, 0.3), 6: (0.9, 0.4), 0: (-0.02, -0.03)},    # below 0 and above 1
        {1: (0.3, 0.3), 2: (float("nan"), 0.3), 5: (0.35, float("inf")), 8: (0.3, 0.5), 11: (0.33, 0.52)},      # not finite = absent
        {1: (0.7, 0.7), 2: (200.0, 0.7), 5: (0.7, -130.0), 8: (0.72, 0.8), 11: (-90.0, 0.9), 0: (0.7, 0.6)},      # beyond [-8192, 16383] at 98 x 66
    ])
    hs[3]["parts"][9] = (0, 0.5, 0.5, 0.0)  # coordinates present, has_value clear
    return hs


def base_humans():
    """what the painting tests draw: the human with end points beyond the drop range is left to the list test - the reference's thickness rule
    makes its discs wider than these frames"""
    return np.concatenate([ref.seeded_humans(11, 3, extent=0.12), special_humans()[:4]])


@pytest.mark.parametrize("W,H,thickness", [(98, 66, 0), (97, 65, 0), (1920, 1080, 0), (8192, 8192, 0), (98, 66, 3), (640, 480, 16384)])
def test_primitive_list_equals_float32_restatement(W, H, thickness):
    hs = np.concatenate([ref.seeded_humans(11, 3, extent=0.12), special_humans(), ref.seeded_humans(5, 6, extent=0.3, keep=0.6, lo=-0.5, hi=1.5)])
    got = frontend.overlay_primitives(hs, W, H, thickness)
    want = ref.primitives(hs, W, H, thickness)
    assert [tuple(int(v) for v in p) for p in got] == want
    assert len(want) > 40 and {p[0] for p in want} == {0, 1}
    # the cases the list must contain: a human that contributes nothing, and dropped / absent parts
    assert 4 not in {p[7] for p in want}
    assert {p[6] for p in want if p[7] == 6 and p[0] == 1} == {1, 8, 11}             # NaN / inf / has_value clear: absent
    assert {p[6] for p in want if p[7] == 7 and p[0] == 1} == {0, 1, 8}              # parts 2, 5, 11 lie beyond the drop range
    assert {p[6] for p in want if p[7] == 7 and p[0] == 0} == {6, 12}
    assert any(p[1] < 0 for p in want) and any(p[2] > H for p in want)


def test_primitive_list_huge_coordinates_and_cap():
    hs = ref.make_humans([{0: (3e38, 0.5), 1: (-3e38, 0.5), 2: (0.5, 0.5), 3: (0.6, 0.5)}, {0: (1e30, 1e30), 1: (0.2, 0.2)}])
    got = frontend.overlay_primitives(hs, 1920, 1080)
    want = ref.primitives(hs, 1920, 1080)
    assert [tuple(int(v) for v in p) for p in got] == want and want and all(p[5] == 16384 for p in want)  # the capped thickness
    # the count is returned whole, only `cap` entries are written
    import ctypes as C
    out = np.zeros(2, _lib.OVERLAY_PRIM_DTYPE)
    n = _lib.lib().hp_overlay_primitives(hs.ctypes.data_as(C.c_void_p), len(hs), 1920, 1080, 0, out.ctypes.data_as(C.c_void_p), 2)
    assert n == len(want) > 2 and [tuple(int(v) for v in p) for p in out] == want[:2]
    for bad in [dict(w=8193, h=10), dict(w=0, h=10), dict(w=10, h=10, thickness=16385)]:
        with pytest.raises(_lib.HpError) as e:
            frontend.overlay_primitives(hs, bad["w"], bad["h"], bad.get("thickness", 0))
        assert e.value.code == _lib.HP_ERR_INVALID


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_yuv_colours_equal_float64_formulas(matrix, rng, depth):
    got = frontend.yuv_colours(matrix, rng, depth)
    assert got.tolist() == ref.colours(matrix, rng, depth).tolist()
    assert got.min() >= 0 and got.max() <= (1 << depth) - 1


# worst |channel error| (8-bit levels) over the 19 colours of "table -> hp_yuv_coefficients' integer form -> BGR" against the RGB the table was
# made from, measured by this test on the CPU (DESIGN.md 1.1 quotes it): 1 for each of the six 8-bit tables (three samples quantised to 8 bits
# cannot do better), 0 for each of the six 10-bit ones.  Every table is held to its measured value plus one level.
ROUND_TRIP_WORST = {8: 1, 10: 0}


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_yuv_colours_round_trip_through_the_front_end(matrix, rng, depth):
    y_off, c_off, CY, CUB, CUG, CVG, CVR = frontend.yuv_coefficients(matrix, rng, depth)
    worst = 0
    for (Y, U, V), (r, g, b) in zip(frontend.yuv_colours(matrix, rng, depth).tolist(), ref.RGB):
        u, v, yy = U - c_off, V - c_off, max(0, Y - y_off) * CY + (1 << 19)
        sat = lambda x: min(255, max(0, x))  # noqa: E731
        back = (sat((yy + CVR * v) >> 20), sat((yy + CVG * v + CUG * u) >> 20), sat((yy + CUB * u) >> 20))
        worst = max(worst, max(abs(p - q) for p, q in zip(back, (r, g, b))))
    print(f"round trip {matrix} {rng} {depth}-bit: worst channel error {worst}")
    assert worst <= ROUND_TRIP_WORST[depth] + 1


SIZES = {None: (97, 65), "i444": (97, 65), "nv16": (98, 65), "i422": (98, 65), "yuy2": (98, 65), "uyvy": (98, 65)}  # every other layout: 98 x 66
COLOURS = {"nv12": ("bt601", "limited"), "i420": ("bt709", "full"), "p010": ("bt2020", "limited"), "i010": ("bt709", "limited"),
           "nv16": ("bt601", "full"), "i422": ("bt2020", "full"), "yuy2": ("bt709", "limited"), "uyvy": ("bt601", "limited"), "i444": ("bt2020", "limited")}


@pytest.mark.parametrize("opacity", [1.0, 0.5, 1.0 / 256])
@pytest.mark.parametrize("fmt", [None] + ref.FORMATS)
def test_host_twin_equals_numpy_painter(fmt, opacity):
    W, H = SIZES.get(fmt, (98, 66))
    matrix, rng = COLOURS.get(fmt, ("bt601", "limited"))
    hs = base_humans()
    view, backs = ref.random_frame(3, fmt, W, H, pad=10)
    want = [b.copy() for b in backs]
    before = [b.copy() for b in backs]
    if fmt is None:
        ref.paint(want[0][:, :W * 3].reshape(H, W, 3), hs, opacity=opacity)
        frontend.draw_humans_host(view, hs, opacity=opacity)
    else:
        ref.paint([b[:, :v.shape[1]] for b, v in zip(want, view)], hs, fmt, matrix, rng, opacity)
        frontend.draw_humans_host(view, hs, fmt, matrix, rng, opacity)
    for k, (g, w, b) in enumerate(zip(backs, want, before)):
        assert np.array_equal(g, w), f"plane {k}: {np.count_nonzero(g != w)} samples differ"
    assert any(not np.array_equal(w, b) for w, b in zip(want, before)), "the case paints nothing"
    # padding: the columns beyond the picture are what they were (also implied by equality with `want`, stated for the reader)
    for g, b, v in zip(backs, before, view if fmt else [view.reshape(H, -1)]):
        assert np.array_equal(g[:, v.shape[1]:], b[:, v.shape[1]:])


def test_opacity_below_one_512th_rewrites_covered_samples_with_themselves():
    """w = nearbyint(opacity * 256) is 0 there: a valid call that leaves every byte as it was"""
    assert ref.weight(1.0 / 1024) == 0
    planes, backs = ref.random_frame(2, "p010", 98, 66, pad=6)
    before = [b.copy() for b in backs]
    frontend.draw_humans_host(planes, base_humans(), "p010", opacity=1.0 / 1024)
    assert all(np.array_equal(b, a) for b, a in zip(before, backs))


def test_host_twin_refuses_bad_arguments():
    hs = base_humans()
    planes, _ = ref.random_frame(1, "nv12", 32, 16)
    before = [p.copy() for p in planes]
    for kw, word in [(dict(opacity=0.0), "opacity"), (dict(opacity=1.5), "opacity"), (dict(opacity=float("nan")), "opacity"), (dict(thickness=20000), "thickness")]:
        with pytest.raises(_lib.HpError) as e:
            frontend.draw_humans_host(planes, hs, "nv12", **kw)
        assert e.value.code == _lib.HP_ERR_INVALID and "HP_YUV_NV12" in str(e.value) and word in str(e.value)
    assert all(np.array_equal(p, b) for p, b in zip(planes, before))
    frontend.draw_humans_host(planes, hs[:0], "nv12")  # no humans: nothing happens
    assert all(np.array_equal(p, b) for p, b in zip(planes, before))
