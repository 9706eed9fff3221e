"""GPU: the redaction kernels (hyperpose_amd/csrc/redact.hip) through hp_redact_u8c3 / hp_redact_yuv, byte-equal to the tests' own numpy painter
(tests/redact_ref.py) on device frames with padded rows, padding included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_ref as ref  # noqa: E402
from test_overlay_host import COLOURS, SIZES  # noqa: E402
from test_redact_host import CELLS, EFFECTS, FORMATS, case_regions  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 10


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.init(0)


class DeviceFrame:
    """a frame on the device, every plane with rows PAD bytes longer than the picture, and its host copy for the painter"""

    def __init__(self, fmt, W, H, seed=3, rng="limited", full_scale=False):
        self.fmt, self.W, self.H, self.rng = fmt, W, H, rng
        view, backs = ref.random_frame(seed, fmt, W, H, pad=PAD)
        if full_scale:
            for v in ([view] if fmt is None else view):
                v[...] = 255 if v.dtype == np.uint8 else 1023 << ref.LAYOUT[fmt][3]
        self.host = [b.copy() for b in backs]  # what the painter paints (padded backing arrays)
        self.cols = [W * 3] if fmt is None else [v.shape[1] for v in view]
        if fmt is None:
            self.bufs, self.strides = [_lib.DevBuf.from_numpy(backs[0])], [backs[0].shape[1]]
            self.image = None
        else:
            self.bufs, self.strides = frontend.yuv_upload(view, fmt, pitch=PAD)
            self.image = frontend.yuv_image(fmt, [b.ptr for b in self.bufs], self.strides, W, H, "bt601", rng)
        self.before = self.download()

    def views(self):
        return self.host[0][:, :self.W * 3].reshape(self.H, self.W, 3) if self.fmt is None else [b[:, :c] for b, c in zip(self.host, self.cols)]

    def paint(self, regs, effect="pixelate", cell=16):
        return ref.paint(self.views(), regs, self.fmt, self.rng, effect, cell)

    def redact(self, regs, effect="pixelate", cell=16, redactor=None, stream=None):
        rs = regs if isinstance(regs, np.ndarray) else ref.as_records(regs)
        if self.fmt is None:
            frontend.redact(self.bufs[0], rs, effect, cell, w=self.W, h=self.H, stride=self.strides[0], redactor=redactor, stream=stream)
        else:
            frontend.redact(self.image, rs, effect, cell, redactor=redactor, stream=stream)

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
        changed = any(not np.array_equal(g, b) for g, b in zip(got, self.before))
        if must_change:
            assert changed, "the case changes nothing"
            assert any(np.any(g == b) for g, b in zip(got, self.before)), "the case leaves nothing unchanged"
        else:
            assert not changed
        return got


def frame_for(fmt, W=None, H=None, **kw):
    w, h = SIZES.get(fmt, (98, 66))
    return DeviceFrame(fmt, W or w, H or h, rng=COLOURS.get(fmt, ("bt601", "limited"))[1], **kw)


def run(fmt, regs, effect="pixelate", cell=16, W=None, H=None, must_change=True, **kw):
    f = frame_for(fmt, W, H, **kw)
    f.paint(regs, effect, cell)
    f.redact(regs, effect, cell)
    return f.check(must_change)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("effect", EFFECTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_device_equals_numpy_painter(fmt, effect, cell):
    W, H = SIZES.get(fmt, (98, 66))
    run(fmt, case_regions(W, H), effect, cell)


@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2", "p010"])
def test_disc_boundary_is_inclusive(fmt):
    """a: a disc at (45, 44) and cell 16: the nearest pixel of cell (3, 3) is (48, 48), 3-4-5 away, so r = 5 reaches it exactly and r = 4 does not"""
    cell33 = (48, 48, 63, 63)
    with_5, with_4 = [(ref.DISC, 45, 44, 5, 0, -1)], [(ref.DISC, 45, 44, 4, 0, -1)]
    assert cell33 in ref.hit_cells(with_5, 98, 66, 16) and cell33 not in ref.hit_cells(with_4, 98, 66, 16)
    assert len(ref.hit_cells(with_5, 98, 66, 16)) == 4 and len(ref.hit_cells(with_4, 98, 66, 16)) == 3
    a = run(fmt, with_5, W=98, H=66)
    b = run(fmt, with_4, W=98, H=66)
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt", [None, "i420", "uyvy", "i010"])
@pytest.mark.parametrize("effect", EFFECTS)
def test_overlapping_regions_of_two_humans(fmt, effect):
    """b: two humans whose heads and bodies reach the same cells: a union, in either order"""
    hs = ref.make_humans([{0: (0.45, 0.3), 1: (0.45, 0.45), 14: (0.43, 0.28), 15: (0.47, 0.28), 8: (0.42, 0.8)},
                          {0: (0.52, 0.35), 1: (0.52, 0.5), 16: (0.5, 0.33), 17: (0.55, 0.33), 11: (0.56, 0.85)}])
    W, H = SIZES.get(fmt, (98, 66))
    regs = ref.regions(hs, W, H, "body", 1.0)
    assert len(regs) == 4
    shared = set(ref.hit_cells(regs[:2], W, H, 6)) & set(ref.hit_cells(regs[2:], W, H, 6))
    assert len(shared) > 4
    a = run(fmt, regs, effect, 6)
    b = run(fmt, regs[::-1], effect, 6)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    got = frontend.redact_regions(hs, W, H, "body", 1.0)  # the library's list of the same humans
    assert [tuple(int(v) for v in r) for r in got] == regs


@pytest.mark.parametrize("fmt", [None, "nv12", "i422", "p010", "i444"])
def test_regions_partly_and_wholly_outside(fmt):
    """c: regions over every edge of the frame; regions wholly outside launch nothing and change nothing"""
    W, H = SIZES.get(fmt, (98, 66))
    partly = [(ref.DISC, -3, 30, 6, 0, -1), (ref.DISC, W + 2, 20, 5, 0, -1), (ref.DISC, 40, -4, 4, 0, -1), (ref.DISC, 60, H + 3, 4, 0, -1),
              (ref.RECT, -8192, 50, 1, 51, -1), (ref.RECT, W - 1, H - 1, 16383, 16383, -1), (ref.RECT, 20, -50, 21, 0, -1)]
    for effect in EFFECTS:
        run(fmt, partly, effect, 6)
    run(fmt, partly, "pixelate", 16)
    wholly = [(ref.DISC, -6, 30, 5, 0, -1), (ref.DISC, W + 5, 20, 5, 0, -1), (ref.DISC, 40, -5, 4, 0, -1), (ref.DISC, 60, H + 4, 4, 0, -1),
              (ref.RECT, -8192, -8192, -1, 16383, -1), (ref.RECT, W, 0, 16383, 10, -1), (ref.RECT, 0, H, 50, H + 10, -1), (ref.RECT, 5, -10, 50, -1, -1),
              (ref.DISC, -4, -3, 4, 0, -1)]  # the last one is 5 away from pixel (0, 0)
    assert ref.hit_cells(wholly, W, H, 2) == []
    run(fmt, wholly, "black", 2, must_change=False)


@pytest.mark.parametrize("fmt", [None, "nv16"])
def test_as_many_regions_as_the_handle_holds(fmt):
    """d: n == max_regions is served, one more is refused"""
    W, H = SIZES.get(fmt, (98, 66))
    r = np.random.default_rng(9)
    regs = [(ref.DISC, int(r.integers(0, W)), int(r.integers(0, H)), 1, 0, -1) for _ in range(12)]
    rd = frontend.Redactor(12)
    f = frame_for(fmt)
    f.paint(regs, "pixelate", 6)
    f.redact(regs, "pixelate", 6, redactor=rd)
    f.check()
    with pytest.raises(_lib.HpError) as e:
        f.redact(regs + regs[:1], "pixelate", 6, redactor=rd)
    assert e.value.code == _lib.HP_ERR_INVALID and "13" in str(e.value) and "12" in str(e.value)
    f.check()
    rd.close()


@pytest.mark.parametrize("fmt", [None, "nv12", "p010"])
def test_back_to_back_calls_on_one_stream(fmt):
    """e: six calls with different region lists on a stream of their own and no synchronise in between - more calls than the handle has staging
    slots.  Lists overlap and the cell size changes from call to call, so a later call averages what an earlier one wrote: the result depends on
    every call having been applied, in order"""
    W, H = SIZES.get(fmt, (98, 66))
    r = np.random.default_rng(4)
    lists = [[(ref.DISC, int(r.integers(10, W - 10)), int(r.integers(10, H - 10)), int(r.integers(3, 15)), 0, -1) for _ in range(3)] for _ in range(6)]
    cells = [6, 16, 2, 16, 6, 2]
    L = _lib.lib()
    owner = C.c_void_p()  # a stream that is not the default one: a parser's own
    _lib.check(L.hp_paf_create(C.byref(owner), C.c_float(0.05), C.c_float(0.05), -1, -1, 1))
    L.hp_paf_stream.restype = C.c_void_p
    stream = L.hp_paf_stream(owner)
    assert stream
    f = frame_for(fmt)
    rd = frontend.Redactor(4)
    for regs, cell in zip(lists, cells):
        f.paint(regs, "pixelate", cell)
    for regs, cell in zip(lists, cells):
        f.redact(regs, "pixelate", cell, redactor=rd, stream=stream)
    f.check()  # synchronises the device
    L.hp_paf_destroy(owner)
    # the order matters for this case: the same calls the other way round give another picture
    other = frame_for(fmt)
    for regs, cell in list(zip(lists, cells))[::-1]:
        other.paint(regs, "pixelate", cell)
    assert any(not np.array_equal(a, b) for a, b in zip(other.host, f.host))
    rd.close()


@pytest.mark.parametrize("fmt", ["p010", "nv12", None])
def test_full_scale_cell_of_128_keeps_full_scale(fmt):
    """f: 128 x 128 samples of full scale in one cell: sum = 16384 * 1023 (or 255) needs more than 16 bits - and more than 24 for the 10-bit frame"""
    f = frame_for(fmt, 128, 128, full_scale=True)
    regs = [(ref.DISC, 64, 64, 3, 0, -1)]
    assert f.paint(regs, "pixelate", 128) == [(0, 0, 127, 127)]
    f.redact(regs, "pixelate", 128)
    got = f.download()
    for k, (g, h, b) in enumerate(zip(got, f.host, f.before)):
        assert np.array_equal(g, h.view(np.uint8).reshape(h.shape[0], -1)), f"{fmt} plane {k}"
        assert np.array_equal(g, b), "the mean of full-scale samples is full scale: the frame is as it was"


def test_forty_humans_body_nv12():
    """g: 642 x 362 (no multiple of the cell, 41 x 23 cells, 11 blocks across), 40 seeded humans, BODY, cell 16"""
    W, H = 642, 362
    hs = ref.seeded_humans(31, 40, extent=0.03)
    regs = ref.regions(hs, W, H, "body", 1.0)
    assert len(regs) > 60
    got = frontend.redact_regions(hs, W, H, "body", 1.0)
    assert [tuple(int(v) for v in r) for r in got] == regs
    f = frame_for("nv12", W, H)
    cells = f.paint(regs, "pixelate", 16)
    assert 100 < len(cells) < 41 * 23
    f.redact(got, "pixelate", 16)
    f.check()


def test_invalid_arguments_are_refused_and_nothing_is_written():
    rd = frontend.Redactor(8)
    L = _lib.lib()
    good = ref.as_records([(ref.DISC, 40, 30, 9, 0, -1), (ref.RECT, 5, 5, 30, 20, 0)])
    gp = good.ctypes.data_as(C.c_void_p)

    def refused(rc, *words):
        msg = L.hp_last_error().decode()
        assert rc == _lib.HP_ERR_INVALID and all(w in msg for w in words), (rc, msg)

    f = frame_for("nv12")
    im = f.image
    for cell in (0, 1, 15, 130, -16):
        refused(L.hp_redact_yuv(rd.h, C.byref(im), gp, 2, 0, cell, None), "HP_YUV_NV12", "cell", str(cell))
    for effect in (-1, 2):
        refused(L.hp_redact_yuv(rd.h, C.byref(im), gp, 2, effect, 16, None), "HP_YUV_NV12", "effect")
    for bad, word in [((2, 1, 1, 2, 2, -1), "kind"), ((ref.RECT, 9, 1, 8, 2, -1), "x0 > x1"), ((ref.RECT, 1, 1, 2, 16384, -1), "16384"),
                      ((ref.DISC, -8193, 1, 2, 0, -1), "-8193"), ((ref.DISC, 1, 1, 16385, 0, -1), "radius"), ((ref.DISC, 1, 1, -1, 0, -1), "radius"),
                      ((ref.DISC, 1, 1, 2, 3, -1), "y1")]:
        rs = ref.as_records([tuple(good[0]), bad])
        refused(L.hp_redact_yuv(rd.h, C.byref(im), rs.ctypes.data_as(C.c_void_p), 2, 0, 16, None), "HP_YUV_NV12", "region 1", word)
    small = frontend.Redactor(1)
    refused(L.hp_redact_yuv(small.h, C.byref(im), gp, 2, 0, 16, None), "HP_YUV_NV12", "regions")
    refused(L.hp_redact_yuv(rd.h, C.byref(im), gp, -1, 0, 16, None), "HP_YUV_NV12")
    refused(L.hp_redact_yuv(rd.h, C.byref(im), None, 2, 0, 16, None), "HP_YUV_NV12")
    refused(L.hp_redact_yuv(None, C.byref(im), gp, 2, 0, 16, None), "handle")

    def image(fmt="nv12", w=98, h=66, strides=None, planes=None):
        return frontend.yuv_image(fmt, planes or [b.ptr for b in f.bufs], strides or f.strides, w, h)

    for bad, words in [(image(w=97), ("HP_YUV_NV12", "even")), (image(strides=[97, 108]), ("HP_YUV_NV12", "stride")), (image(planes=[f.bufs[0].ptr, 0]), ("HP_YUV_NV12", "null")),
                       (image("p010", strides=[213, 214]), ("HP_YUV_P010", "even")), (image(w=8194, h=66, strides=[8194, 8194]), ("HP_YUV_NV12", "8192")),
                       (image(w=98, h=8194), ("HP_YUV_NV12", "8192"))]:
        refused(L.hp_redact_yuv(rd.h, C.byref(bad), gp, 2, 0, 16, None), *words)
    bad = image()
    bad.format = 9
    refused(L.hp_redact_yuv(rd.h, C.byref(bad), gp, 2, 0, 16, None), "format")
    f.redact(good[:0])  # no regions: HP_OK, nothing launched
    f.check(must_change=False)

    g = frame_for(None)
    ptr, stride = g.bufs[0].ptr, g.strides[0]
    for args, words in [((ptr, 97, 65, stride, gp, 2, 0, 14 + 1, None), ("BGR", "cell")), ((ptr, 97, 65, stride, gp, 2, 3, 16, None), ("BGR", "effect")),
                        ((ptr, 97, 65, 97 * 3 - 1, gp, 2, 0, 16, None), ("BGR", "stride")), ((ptr, 8193, 65, 8193 * 3, gp, 2, 0, 16, None), ("BGR", "8192")),
                        ((ptr, 0, 65, stride, gp, 2, 0, 16, None), ("BGR", "empty")), ((None, 97, 65, stride, gp, 2, 0, 16, None), ("BGR", "null"))]:
        refused(L.hp_redact_u8c3(rd.h, *args), *words)
    refused(L.hp_redact_u8c3(small.h, ptr, 97, 65, stride, gp, 2, 0, 16, None), "BGR", "regions")
    g.check(must_change=False)
    rd.close()
    small.close()
