"""GPU: the overlay kernels (hyperpose_amd/csrc/overlay.hip) through hp_overlay_draw_u8c3 / hp_overlay_draw_yuv, byte-equal to the tests' own
numpy painter (tests/overlay_ref.py) on device frames with padded rows, padding included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as ref  # noqa: E402
from test_overlay_host import COLOURS, SIZES, base_humans  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 10


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.init(0)


class DeviceFrame:
    """a seeded frame on the device, every plane with rows PAD bytes longer than the picture, and its host copy for the painter"""

    def __init__(self, fmt, W, H, seed=3, matrix="bt601", rng="limited"):
        self.fmt, self.W, self.H, self.matrix, self.rng = fmt, W, H, matrix, rng
        view, backs = ref.random_frame(seed, fmt, W, H, pad=PAD)
        self.host = [b.copy() for b in backs]  # what the painter paints (padded backing arrays)
        self.cols = [W * 3] if fmt is None else [v.shape[1] for v in view]
        if fmt is None:
            self.bufs, self.strides = [_lib.DevBuf.from_numpy(backs[0])], [backs[0].shape[1]]
            self.image = None
        else:
            self.bufs, self.strides = frontend.yuv_upload(view, fmt, pitch=PAD)
            self.image = frontend.yuv_image(fmt, [b.ptr for b in self.bufs], self.strides, W, H, matrix, rng)
        self.before = self.download()

    def views(self):
        return self.host[0][:, :self.W * 3].reshape(self.H, self.W, 3) if self.fmt is None else [b[:, :c] for b, c in zip(self.host, self.cols)]

    def paint(self, humans, opacity=1.0, thickness=0):
        ref.paint(self.views(), humans, self.fmt, self.matrix, self.rng, opacity, thickness)

    def draw(self, humans, opacity=1.0, thickness=0, overlay=None, stream=None):
        if self.fmt is None:
            frontend.draw_humans(self.bufs[0], humans, opacity, thickness, w=self.W, h=self.H, stride=self.strides[0], overlay=overlay, stream=stream)
        else:
            frontend.draw_humans(self.image, humans, opacity, thickness, overlay=overlay, stream=stream)

    def download(self):
        _lib.check(_lib.lib().hp_device_synchronize())
        return [b.to_numpy(np.uint8, (h.shape[0], s)) for b, h, s in zip(self.bufs, self.host, self.strides)]

    def check(self, must_change=True):
        got = self.download()
        for k, (g, h, b) in enumerate(zip(got, self.host, self.before)):
            want = h.view(np.uint8).reshape(h.shape[0], -1)
            assert g.shape == want.shape
            bad = np.argwhere(g != want)
            assert bad.size == 0, f"{self.fmt} plane {k}: {len(bad)} bytes differ, first at (row, byte) {bad[0].tolist()}"
            row = self.cols[k] * h.itemsize
            assert np.array_equal(g[:, row:], b[:, row:]), f"{self.fmt} plane {k}: row padding was written"
        if must_change:
            assert any(not np.array_equal(g, b) for g, b in zip(got, self.before)), "the case paints nothing"
        return got


def frame_for(fmt, W=None, H=None, **kw):
    w, h = SIZES.get(fmt, (98, 66))
    matrix, rng = COLOURS.get(fmt, ("bt601", "limited"))
    return DeviceFrame(fmt, W or w, H or h, matrix=matrix, rng=rng, **kw)


def run(fmt, humans, opacity=1.0, thickness=0, W=None, H=None, must_change=True, overlay=None):
    f = frame_for(fmt, W, H)
    f.paint(humans, opacity, thickness)
    f.draw(humans, opacity, thickness, overlay)
    return f.check(must_change)


@pytest.mark.parametrize("opacity", [1.0, 0.5, 1.0 / 256])
@pytest.mark.parametrize("fmt", [None] + ref.FORMATS)
def test_device_equals_numpy_painter(fmt, opacity):
    run(fmt, base_humans(), opacity)


@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2", "p010"])
def test_primitives_across_tile_corners(fmt):
    """a limb and discs that run through several 32 x 8-block tiles diagonally, and a disc centred on a tile corner of the grid (the grid starts at
    the list's rectangle: with a part at the frame's origin that is pixel (0, 0), so corners lie at multiples of the tile)"""
    W, H = 194, 66
    tile = (32, 8) if fmt is None else (64, 16) if fmt in ("nv12", "p010") else (64, 8)
    hs = ref.make_humans([{1: (0.0, 0.0), 2: ((tile[0] + 0.5) / W, (tile[1] + 0.5) / H), 3: (0.97, 0.95)},
                          {0: ((2 * tile[0] + 0.5) / W, (2 * tile[1] + 0.5) / H)}])
    prims = ref.primitives(hs, W, H, 5)
    assert (1, tile[0], tile[1], tile[0], tile[1], 5, 2, 0) in prims and (1, 2 * tile[0], 2 * tile[1], 2 * tile[0], 2 * tile[1], 5, 0, 1) in prims
    run(fmt, hs, 1.0, 5, W, H)
    run(fmt, hs, 0.5, 0, W, H)


@pytest.mark.parametrize("fmt", [None, "i420", "uyvy", "i010", "i444"])
def test_primitives_partly_and_wholly_outside(fmt):
    partly = ref.make_humans([{1: (-0.3, 0.5), 2: (0.2, 0.45)}, {1: (0.8, 0.5), 5: (1.4, 0.6)}, {1: (0.5, -0.4), 8: (0.45, 0.2)}, {1: (0.5, 0.7), 11: (0.55, 1.5)},
                              {0: (-0.01, -0.01)}, {0: (1.0, 1.0)}, {2: (-0.2, -0.3), 3: (1.2, 1.3)}])
    run(fmt, partly, 1.0, 4)
    run(fmt, partly, 0.5, 0)
    wholly = ref.make_humans([{1: (-0.5, 0.5), 2: (-0.3, 0.45)}, {1: (1.3, 0.5), 5: (1.4, 0.6)}, {1: (0.5, -0.4), 8: (0.45, -0.2)}, {1: (0.5, 1.7), 11: (0.55, 1.5)},
                              {0: (-80.0, 0.5), 1: (0.5, 300.0)}])
    assert len(ref.primitives(wholly, 98, 66, 3)) == 13
    run(fmt, wholly, 1.0, 3, must_change=False)


@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2"])
def test_degenerate_limb(fmt):
    hs = ref.make_humans([{1: (0.5, 0.5), 2: (0.501, 0.501), 5: (0.3, 0.3), 6: (0.3, 0.3)}])
    prims = ref.primitives(hs, 98, 66, 7)
    assert any(p[0] == 0 and p[1:3] == p[3:5] for p in prims)
    run(fmt, hs, 1.0, 7)


@pytest.mark.parametrize("fmt", [None, "nv12", "i422", "p010"])
def test_capsule_wider_than_a_tile(fmt):
    hs = ref.make_humans([{1: (0.3, 0.4), 2: (0.7, 0.6), 3: (0.75, 0.2)}])
    run(fmt, hs, 1.0, 40, 128, 96)
    run(fmt, hs, 0.5, 40, 128, 96)


@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2", "i010"])
def test_more_primitives_than_the_lds_list_keep_painters_order(fmt):
    """64 humans with all 18 parts on one spot of a 96 x 64 frame: 2 368 primitives through one tile, more than the kernel's LDS list holds, so
    the tile is painted in chunks.  Identical humans first (the picture is the last human's), then with the LAST human mirrored, whose colours
    land elsewhere: painted over all the others it proves a later chunk wins over an earlier one."""
    r = np.random.default_rng(5)
    one = {k: (0.5 + float(r.uniform(-0.06, 0.06)), 0.5 + float(r.uniform(-0.08, 0.08))) for k in range(18)}
    mirrored = {k: (1.0 - x, y) for k, (x, y) in one.items()}
    ov = frontend.Overlay(64)
    same = ref.make_humans([one] * 64)
    assert len(ref.primitives(same, 96, 64)) == 64 * 37
    a = run(fmt, same, 1.0, 0, 96, 64, overlay=ov)
    single = frame_for(fmt, 96, 64)
    single.paint(same[63:], 1.0)
    assert all(np.array_equal(g, h.view(np.uint8).reshape(g.shape)) for g, h in zip(a, single.host)), "64 identical humans at opacity 1 = the last one"
    last_differs = ref.make_humans([one] * 63 + [mirrored])
    b = run(fmt, last_differs, 1.0, 0, 96, 64, overlay=ov)
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))
    run(fmt, last_differs, 0.5, 0, 96, 64, overlay=ov)
    with pytest.raises(_lib.HpError) as e:  # one more than the handle was made for
        frame_for(fmt, 96, 64).draw(ref.make_humans([one] * 65), overlay=ov)
    assert e.value.code == _lib.HP_ERR_INVALID and "65" in str(e.value)
    ov.close()


@pytest.mark.parametrize("fmt", ["nv12", "yuy2"])
def test_one_pixel_lines_at_odd_columns(fmt):
    """T = 1 capsules are one pixel wide; at an odd x0 (and an odd y0 for the horizontal one) they cover one pixel of each chroma sample they cross,
    which is written all the same: the 'any covered' rule"""
    W, H = 98, 66
    hs = ref.make_humans([{1: (33.5 / W, 9.5 / H), 8: (33.5 / W, 50.5 / H)}, {2: (41.5 / W, 21.5 / H), 3: (80.5 / W, 21.5 / H)}])
    prims, last = ref.coverage(hs, W, H, 1)
    assert (0, 33, 9, 33, 50, 1, 6, 0) in prims and (last[30, 32:35] >= 0).tolist() == [False, True, False] and (last[20:23, 60] >= 0).tolist() == [False, True, False]
    run(fmt, hs, 1.0, 1, W, H)
    run(fmt, hs, 0.5, 1, W, H)


@pytest.mark.parametrize("fmt", [None, "nv12"])
def test_no_humans_leaves_the_frame_alone(fmt):
    f = frame_for(fmt)
    f.draw(base_humans()[:0])
    f.draw(ref.make_humans([{}, {}]))  # humans without parts: an empty list
    f.check(must_change=False)


@pytest.mark.parametrize("fmt", [None, "nv12", "p010"])
def test_back_to_back_calls_on_one_stream(fmt):
    """six calls with different human lists and no synchronise in between: more calls than the handle has staging slots, so a slot is reused while
    earlier calls may still be running; at opacity 0.5 the result depends on every call having drawn its own list, in order"""
    lists = [ref.seeded_humans(20 + k, 2, extent=0.15, lo=0.2, hi=0.8) for k in range(6)]
    f = frame_for(fmt)
    ov = frontend.Overlay(4)
    for hs in lists:
        f.paint(hs, 0.5)
        f.draw(hs, 0.5, overlay=ov)
    f.check()
    ov.close()


def test_invalid_arguments_are_refused_and_nothing_is_written():
    hs = base_humans()
    ov = frontend.Overlay(len(hs))
    L = _lib.lib()
    hp = hs.ctypes.data_as(C.c_void_p)

    def refused(rc, *words):
        msg = L.hp_last_error().decode()
        assert rc == _lib.HP_ERR_INVALID and all(w in msg for w in words), (rc, msg)

    f = frame_for("nv12")
    im = f.image
    for op in (0.0, -0.5, 1.0001, float("nan")):
        refused(L.hp_overlay_draw_yuv(ov.h, C.byref(im), hp, len(hs), C.c_float(op), 0, None), "HP_YUV_NV12", "opacity")
    small = frontend.Overlay(2)
    refused(L.hp_overlay_draw_yuv(small.h, C.byref(im), hp, len(hs), C.c_float(1.0), 0, None), "HP_YUV_NV12", "humans")
    refused(L.hp_overlay_draw_yuv(ov.h, C.byref(im), hp, -1, C.c_float(1.0), 0, None), "HP_YUV_NV12")
    refused(L.hp_overlay_draw_yuv(ov.h, C.byref(im), None, 2, C.c_float(1.0), 0, None), "HP_YUV_NV12")

    def image(fmt="nv12", w=98, h=66, strides=None, planes=None, matrix="bt601"):
        return frontend.yuv_image(fmt, planes or [b.ptr for b in f.bufs], strides or f.strides, w, h, matrix)

    for bad, words in [(image(w=97), ("HP_YUV_NV12", "even")), (image(h=65), ("HP_YUV_NV12", "even")), (image(strides=[97, 108]), ("HP_YUV_NV12", "stride")),
                       (image(strides=[108, 90]), ("HP_YUV_NV12", "stride")), (image(planes=[f.bufs[0].ptr, 0]), ("HP_YUV_NV12", "null")),
                       (image("p010", strides=[213, 214]), ("HP_YUV_P010", "even")), (image("p010", strides=[212, 212], planes=[f.bufs[0].ptr.value + 1, f.bufs[1].ptr]), ("HP_YUV_P010", "even")),
                       (image(w=8194, h=66, strides=[8194, 8194]), ("HP_YUV_NV12", "8192")), (image(w=98, h=8194), ("HP_YUV_NV12", "8192")),
                       (image("yuy2", w=97), ("HP_YUV_YUY2", "even"))]:
        refused(L.hp_overlay_draw_yuv(ov.h, C.byref(bad), hp, len(hs), C.c_float(1.0), 0, None), *words)
    bad = image()
    bad.format = 9
    refused(L.hp_overlay_draw_yuv(ov.h, C.byref(bad), hp, len(hs), C.c_float(1.0), 0, None), "format")
    bad = image()
    bad.matrix = 3
    refused(L.hp_overlay_draw_yuv(ov.h, C.byref(bad), hp, len(hs), C.c_float(1.0), 0, None), "HP_YUV_NV12", "matrix")
    refused(L.hp_overlay_draw_yuv(None, C.byref(im), hp, len(hs), C.c_float(1.0), 0, None), "handle")
    refused(L.hp_overlay_draw_yuv(ov.h, C.byref(im), hp, len(hs), C.c_float(1.0), 16385, None), "HP_YUV_NV12", "thickness")
    f.check(must_change=False)

    g = frame_for(None)
    ptr, stride = g.bufs[0].ptr, g.strides[0]
    for args, words in [((ptr, 97, 65, stride, hp, len(hs), C.c_float(0.0), 0, None), ("BGR", "opacity")),
                        ((ptr, 97, 65, 97 * 3 - 1, hp, len(hs), C.c_float(1.0), 0, None), ("BGR", "stride")),
                        ((ptr, 8193, 65, 8193 * 3, hp, len(hs), C.c_float(1.0), 0, None), ("BGR", "8192")),
                        ((ptr, 97, 8193, stride, hp, len(hs), C.c_float(1.0), 0, None), ("BGR", "8192")),
                        ((ptr, 0, 65, stride, hp, len(hs), C.c_float(1.0), 0, None), ("BGR", "empty")),
                        ((None, 97, 65, stride, hp, len(hs), C.c_float(1.0), 0, None), ("BGR", "null"))]:
        refused(L.hp_overlay_draw_u8c3(ov.h, *args), *words)
    refused(L.hp_overlay_draw_u8c3(small.h, ptr, 97, 65, stride, hp, len(hs), C.c_float(1.0), 0, None), "BGR", "humans")
    g.check(must_change=False)
    ov.close()
    small.close()
