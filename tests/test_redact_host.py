"""CPU: the host half of redaction (include/hp_hip.h, hp_redact_*): the region list and the host twins, against the tests' own numpy statement of
DESIGN.md 1.1 "Redaction" (tests/redact_ref.py).  Byte equality everywhere; no device is needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_ref as ref  # noqa: E402
from test_overlay_host import COLOURS, SIZES  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402

FORMATS = [None] + list(ref.LAYOUT)
CELLS = [2, 6, 16, 128]
EFFECTS = ["pixelate", "black"]


def special_humans():
    nan, inf = float("nan"), float("inf")
    hs = ref.make_humans([
        {0: (0.5, 0.2), 1: (0.5, 0.35), 2: (0.4, 0.36), 5: (0.6, 0.36), 14: (0.48, 0.18), 15: (0.52, 0.18), 8: (0.45, 0.6)},  # a whole upper body
        {},                                                                                                             # no parts at all
        {0: (nan, 0.3), 14: (0.3, inf), 15: (0.31, 0.3), 1: (0.3, 0.4), 2: (-inf, 0.4), 5: (0.35, 0.41)},              # not finite = absent
        {0: (200.0, 0.5), 16: (0.7, -130.0), 17: (0.71, 0.52), 1: (0.7, 0.6), 8: (0.7, 300.0)},                          # points beyond the range
        {1: (0.2, 0.6), 2: (0.15, 0.61), 5: (0.25, 0.61), 8: (0.18, 0.8), 11: (0.22, 0.8)},                              # no face points
        {0: (0.8, 0.3)},                                                                                                # only a nose
        {k: (0.6, 0.7) for k in range(18)},                                                                             # all points coincident: b = 1
        {0: (-0.02, -0.03), 1: (-0.05, 0.1), 16: (1.04, 0.3), 2: (0.9, 1.08)},                                          # below 0 and above 1
    ])
    hs[4]["parts"][0] = (0, 0.2, 0.5, 0.0)  # coordinates present, has_value clear
    return hs


def all_humans():
    return np.concatenate([special_humans(), ref.seeded_humans(11, 4, extent=0.12), ref.seeded_humans(5, 6, extent=0.3, keep=0.6, lo=-0.5, hi=1.5)])


def listed(regs):
    return [tuple(int(v) for v in r) for r in regs]


@pytest.mark.parametrize("W,H", [(97, 65), (1920, 1080)])
@pytest.mark.parametrize("margin", [0.5, 1.0, 3.0])
@pytest.mark.parametrize("what", ["head", "body"])
def test_region_list_equals_restatement(what, margin, W, H):
    hs = all_humans()
    want = ref.regions(hs, W, H, what, margin)
    assert listed(frontend.redact_regions(hs, W, H, what, margin)) == want
    by_human = {i: [r for r in want if r[5] == i] for i in range(len(hs))}
    assert by_human[1] == []                                                     # no parts: nothing
    assert [r[0] for r in by_human[4]] == ([ref.RECT] if what == "body" else [])  # no face points: no disc
    assert [r[0] for r in by_human[0]] == ([ref.RECT, ref.DISC] if what == "body" else [ref.DISC])
    m = int(np.rint(margin * 256))
    assert by_human[6][-1][3] == max(1, (m + 128) >> 8)                          # coincident points: b = 1
    assert by_human[5][-1][1:3] == (int(np.float32(0.8) * np.float32(W)), int(np.float32(0.3) * np.float32(H)))
    assert len(by_human[3]) == (2 if what == "body" else 1) and by_human[3][-1][3] == max(1, (m + 128) >> 8)  # only part 17 of the face is in range
    assert any(r[1] < 0 for r in want)


def test_region_list_cap_huge_coordinates_and_refusals():
    hs = np.concatenate([all_humans(), ref.make_humans([{0: (3e38, 0.5), 14: (-3e38, 0.5), 15: (0.5, 0.5), 1: (0.6, 0.5)}, {0: (1e30, 1e30), 1: (0.2, 0.2)},
                                                        {1: (-3.0, 0.5), 8: (8.0, 0.5)}])])  # 21 120 pixels wide at margin 8: the RECT is clamped
    want = ref.regions(hs, 1920, 1080, "body", 8.0)
    assert listed(frontend.redact_regions(hs, 1920, 1080, "body", 8.0)) == want
    assert want[-1] == (ref.RECT, -8192, -8192, 16383, 16383, len(hs) - 1) and all(-8192 <= v <= 16383 for r in want for v in r[1:3])
    # the count is returned whole, only `cap` entries are written
    out = np.zeros(3, _lib.REDACT_REGION_DTYPE)
    n = _lib.lib().hp_redact_regions(hs.ctypes.data_as(C.c_void_p), len(hs), 1920, 1080, 1, C.c_float(8.0), out.ctypes.data_as(C.c_void_p), 2)
    assert n == len(want) > 3 and listed(out[:2]) == want[:2] and listed(out[2:]) == [(0, 0, 0, 0, 0, 0)]
    for bad, word in [(dict(w=8193, h=10), "8193"), (dict(w=0, h=10), "0 x 10"), (dict(w=10, h=10, margin=0.0), "margin"), (dict(w=10, h=10, margin=8.5), "margin"),
                      (dict(w=10, h=10, margin=float("nan")), "margin"), (dict(w=10, h=10, margin=-1.0), "margin")]:
        with pytest.raises(_lib.HpError) as e:
            frontend.redact_regions(hs, bad["w"], bad["h"], "head", bad.get("margin", 1.0))
        assert e.value.code == _lib.HP_ERR_INVALID and word in str(e.value)
    rc = _lib.lib().hp_redact_regions(hs.ctypes.data_as(C.c_void_p), len(hs), 10, 10, 2, C.c_float(1.0), out.ctypes.data_as(C.c_void_p), 2)
    assert rc == _lib.HP_ERR_INVALID and "what" in _lib.lib().hp_last_error().decode()


def case_regions(W, H):
    """what the painting tests redact: heads and bodies of seeded humans, the special cases, and two regions of the caller's own"""
    hs = np.concatenate([ref.seeded_humans(11, 3, extent=0.12), special_humans()[:2]])
    return (ref.regions(hs, W, H, "head", 0.5) + ref.regions(hs[:1], W, H, "body", 0.5)
            + [(ref.RECT, 70, 50, 200, 51, -1), (ref.DISC, 3, 60, 0, 0, -1), (ref.DISC, 80, 20, 9, 0, -1)])


def run_host(view, regs, fmt, rng, effect, cell):
    if fmt is None:
        frontend.redact_host(view, ref.as_records(regs), effect=effect, cell=cell)
    else:
        frontend.redact_host(view, ref.as_records(regs), fmt, "bt601", rng, effect, cell)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("effect", EFFECTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_twin_equals_numpy_painter(fmt, effect, cell):
    W, H = SIZES.get(fmt, (98, 66))
    rng = COLOURS.get(fmt, ("bt601", "limited"))[1]
    regs = case_regions(W, H)
    view, backs = ref.random_frame(3, fmt, W, H, pad=10)
    want = [b.copy() for b in backs]
    before = [b.copy() for b in backs]
    want_views = want[0][:, :W * 3].reshape(H, W, 3) if fmt is None else [b[:, :v.shape[1]] for b, v in zip(want, view)]
    cells = ref.paint(want_views, regs, fmt, rng, effect, cell)
    run_host(view, regs, fmt, rng, effect, cell)
    for k, (g, w) in enumerate(zip(backs, want)):
        assert np.array_equal(g, w), f"plane {k}: {np.count_nonzero(g != w)} samples differ"
    assert cells and any(not np.array_equal(w, b) for w, b in zip(want, before)), "the case redacts nothing"
    if cell < 128:
        assert len(cells) < -(-W // cell) * -(-H // cell), "the case redacts every cell"
    # padding: the columns beyond the picture are what they were (also implied by equality with `want`, stated for the reader)
    for g, b, v in zip(backs, before, view if fmt else [view.reshape(H, -1)]):
        assert np.array_equal(g[:, v.shape[1]:], b[:, v.shape[1]:])
    # redacting twice gives the bytes of redacting once
    run_host(view, regs, fmt, rng, effect, cell)
    assert all(np.array_equal(g, w) for g, w in zip(backs, want))


def test_host_twin_refuses_bad_arguments_and_leaves_the_frame_alone():
    planes, _ = ref.random_frame(1, "nv12", 32, 16)
    bgr, _ = ref.random_frame(1, None, 31, 17)
    before, bgr_before = [p.copy() for p in planes], bgr.copy()
    good = [(ref.DISC, 10, 8, 5, 0, -1)]
    cases = [(dict(cell=15), good, "15"), (dict(cell=0), good, "cell"), (dict(cell=130), good, "130"), (dict(cell=-2), good, "cell"),
             ({}, [(2, 1, 1, 2, 2, -1)], "kind"), ({}, [(-1, 1, 1, 2, 2, -1)], "kind"),
             ({}, good + [(ref.RECT, 5, 5, 4, 9, -1)], "x0 > x1"), ({}, [(ref.RECT, 5, 5, 9, 4, -1)], "y0 > y1"),
             ({}, [(ref.RECT, -8193, 5, 9, 9, -1)], "-8193"), ({}, [(ref.RECT, 0, 5, 16384, 9, -1)], "16384"), ({}, [(ref.RECT, 0, -9000, 3, 9, -1)], "-9000"),
             ({}, [(ref.DISC, 16384, 5, 3, 0, -1)], "centre"), ({}, [(ref.DISC, 5, 5, -1, 0, -1)], "radius"), ({}, [(ref.DISC, 5, 5, 16385, 0, -1)], "16385"),
             ({}, [(ref.DISC, 5, 5, 3, 1, -1)], "y1")]
    for kw, regs, word in cases:
        with pytest.raises(_lib.HpError) as e:
            frontend.redact_host(planes, ref.as_records(regs), "nv12", **kw)
        assert e.value.code == _lib.HP_ERR_INVALID and "HP_YUV_NV12" in str(e.value) and word in str(e.value), str(e.value)
        with pytest.raises(_lib.HpError) as e:
            frontend.redact_host(bgr, ref.as_records(regs), **kw)
        assert e.value.code == _lib.HP_ERR_INVALID and "BGR" in str(e.value) and word in str(e.value), str(e.value)
    L = _lib.lib()
    rs = ref.as_records(good)
    im = frontend.yuv_image("nv12", [p.ctypes.data for p in planes], [p.strides[0] for p in planes], 32, 16)
    assert L.hp_redact_yuv_host(C.byref(im), rs.ctypes.data_as(C.c_void_p), 1, 2, 16) == _lib.HP_ERR_INVALID and "effect" in L.hp_last_error().decode()
    assert L.hp_redact_u8c3_host(C.c_void_p(bgr.ctypes.data), 31, 17, 31 * 3, rs.ctypes.data_as(C.c_void_p), 1, -1, 16) == _lib.HP_ERR_INVALID
    assert "effect" in L.hp_last_error().decode()
    assert L.hp_redact_yuv_host(C.byref(im), None, 1, 0, 16) == _lib.HP_ERR_INVALID
    assert all(np.array_equal(p, b) for p, b in zip(planes, before)) and np.array_equal(bgr, bgr_before)
    frontend.redact_host(planes, ref.as_records([]), "nv12")  # no regions: nothing happens
    frontend.redact_host(planes, ref.as_records([(ref.DISC, -50, -50, 10, 0, -1)]), "nv12")  # a region that reaches no cell
    assert all(np.array_equal(p, b) for p, b in zip(planes, before))
