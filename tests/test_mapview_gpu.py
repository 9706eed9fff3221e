"""GPU: the map view's kernels (hyperpose_amd/csrc/mapview.hip) through hp_mapview_draw_u8c3 / hp_mapview_draw_yuv, byte-equal to the tests' own numpy
painter (tests/mapview_ref.py) on device frames whose rows are padded by 10 poisoned bytes, padding included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapview_ref as ref  # noqa: E402
from test_mapview_host import BIG_MAPS, FORMATS, LETTERBOX, MAPS, ROIS, colour_of, refusal_cases, size_of  # noqa: E402

from hyperpose_amd import _lib, frontend  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 10
# the painter gives a lane a run of 4 chroma blocks - 4 pixels of BGR, 8 of every layout with 2 x N chroma blocks - and a block 64 runs across
RUN_PIXELS = {None: 4, "nv12": 8, "p010": 8, "yuy2": 8}
DENSE = (1030, 18)  # more than two block tiles wide (256 / 512 pixels), no multiple of a tile or a run


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.init(0)


@pytest.fixture(scope="module")
def dev_maps():
    return {id(m): _lib.DevBuf.from_numpy(m) for m in (MAPS, BIG_MAPS)}


class DeviceFrame:
    """a frame on the device, every plane with rows PAD bytes longer than the picture, and its host copy for the painter"""

    def __init__(self, fmt, W, H, seed=3):
        self.fmt, self.W, self.H = fmt, W, H
        self.matrix, self.rng = colour_of(fmt)
        view, backs = ref.random_frame(seed, fmt, W, H, pad=PAD)
        self.host = [b.copy() for b in backs]
        self.cols = [W * 3] if fmt is None else [v.shape[1] for v in view]
        if fmt is None:
            self.bufs, self.strides, self.image = [_lib.DevBuf.from_numpy(backs[0])], [backs[0].shape[1]], None
        else:
            self.bufs, self.strides = frontend.yuv_upload(view, fmt, pitch=PAD)
            self.image = frontend.yuv_image(fmt, [b.ptr for b in self.bufs], self.strides, W, H, self.matrix, self.rng)
        self.before = self.download()

    def views(self):
        return self.host[0][:, :self.W * 3].reshape(self.H, self.W, 3) if self.fmt is None else [b[:, :c] for b, c in zip(self.host, self.cols)]

    def paint(self, maps, index=0, **kw):
        return ref.paint(self.views(), maps[index], self.fmt, self.matrix, self.rng, **kw)

    def paint_host_twin(self, maps, index=0, pal=None, **kw):
        frontend.draw_maps_host(self.views(), maps, self.fmt, self.matrix, self.rng, index=index, palette=ref.palette() if pal is None else pal, **kw)

    def draw(self, maps_dev, maps, index=0, pal=None, view=None, stream=None, **kw):
        pal = ref.palette() if pal is None else pal
        common = dict(frame=index, palette=pal, view=view, stream=stream, **kw)
        if self.fmt is None:
            frontend.draw_maps(self.bufs[0], maps_dev, maps.shape[1:], w=self.W, h=self.H, stride=self.strides[0], **common)
        else:
            frontend.draw_maps(self.image, maps_dev, maps.shape[1:], **common)

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
        assert any(not np.array_equal(g, b) for g, b in zip(got, self.before)) == must_change
        return got


def run(fmt, W, H, maps, dev_maps, index=0, must_change=True, **kw):
    f = DeviceFrame(fmt, W, H)
    f.paint(maps, index, **kw)
    f.draw(dev_maps[id(maps)], maps, index, **kw)
    return f.check(must_change)


@pytest.mark.parametrize("opacity", [1.0, 0.5])
@pytest.mark.parametrize("fmt", FORMATS)
def test_device_equals_numpy_painter(fmt, opacity, dev_maps):
    """every layout; frame 2 of a three-frame batch whose frames differ"""
    W, H = size_of(fmt)
    run(fmt, W, H, MAPS, dev_maps, index=2, opacity=opacity, cover=LETTERBOX)


@pytest.mark.parametrize("fmt", FORMATS)
def test_smallest_frame_one_cell_map(fmt):
    maps = np.full((1, 2, 1, 1), 0.7, np.float32)
    run(fmt, 2, 2, maps, {id(maps): _lib.DevBuf.from_numpy(maps)}, opacity=1.0, pal=ref.palette("heat"))


@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2", "i010"])
def test_map_larger_than_the_frame(fmt, dev_maps):
    run(fmt, 16, 12, BIG_MAPS, dev_maps, pal=ref.palette("grey", "scaled"), opacity=1.0)


@pytest.mark.parametrize("orientation", range(8))
@pytest.mark.parametrize("fmt", [None, "nv12", "yuy2"])
def test_every_orientation(fmt, orientation, dev_maps):
    W, H = size_of(fmt)
    run(fmt, W, H, MAPS, dev_maps, orientation=orientation, cover=(0.75, LETTERBOX[1]))


@pytest.mark.parametrize("roi", ROIS + ["edge"])
@pytest.mark.parametrize("fmt", [None, "nv12", "i420", "nv16", "uyvy", "p010"])
def test_rois_with_partial_chroma_blocks(fmt, roi, dev_maps):
    W, H = size_of(fmt)
    if roi == "edge":
        roi = (W - 9, H - 7, 9, 7)
    roi = (roi[0], roi[1], min(roi[2], W - roi[0]), min(roi[3], H - roi[1]))
    run(fmt, W, H, MAPS, dev_maps, roi=roi, orientation=5, opacity=1.0, pal=ref.palette("heat"))


@pytest.mark.parametrize("alpha", ["constant", "scaled"])
@pytest.mark.parametrize("fmt", [None, "i420", "i422", "uyvy", "i010", "i444"])
def test_channel_step_and_field_mode(fmt, alpha, dev_maps):
    W, H = size_of(fmt)
    run(fmt, W, H, MAPS, dev_maps, index=1, mode="field", channels=(0, 2, 5), gain=0.5 if alpha == "scaled" else 4.0, pal=ref.palette("jet", alpha))
    run(fmt, W, H, MAPS, dev_maps, index=1, mode="max", channels=(1, 2, 5), pal=ref.palette("heat", alpha))


@pytest.mark.parametrize("mode,channels,gain", [("max", None, 1.0), ("max", (1, 3, 5), 0.5), ("field", None, 4.0), ("field", (0, 3, 5), 1.0)])
def test_index_plane_on_the_device(mode, channels, gain):
    """NaN, infinities, negatives and values above 1: the reduce kernel's plane is the float32 restatement's"""
    from test_mapview_host import special_maps
    maps = special_maps()
    dev = _lib.DevBuf.from_numpy(maps)
    view = frontend.MapView(maps.shape[2] * maps.shape[3])
    f = DeviceFrame("nv12", 16, 12)
    plane = f.paint(maps, 1, mode=mode, channels=channels, gain=gain)
    f.draw(dev, maps, 1, view=view, mode=mode, channels=channels, gain=gain)
    assert view.debug_plane().reshape(plane.shape).tolist() == plane.tolist()
    f.check()
    view.close()


def test_p010_low_six_bits_are_zero(dev_maps):
    W, H = size_of("p010")
    got = run("p010", W, H, MAPS, dev_maps, opacity=1.0)
    for g, cols in zip(got, (W, W)):
        words = g[:, :cols * 2].copy().view(np.uint16)
        assert not (words & 63).any()


# ---- the dense-store path -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [None, "nv12", "p010", "yuy2"])
def test_dense_frame_wider_than_two_tiles(fmt, dev_maps):
    run(fmt, *DENSE, MAPS, dev_maps, cover=LETTERBOX)
    run(fmt, *DENSE, MAPS, dev_maps, orientation=3, pal=ref.palette("heat", "scaled"), opacity=1.0)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("fmt", [None, "nv12", "p010", "yuy2"])
def test_dense_roi_heads_and_tails_off_a_run_boundary(fmt, k, dev_maps):
    """the roi starts k pixels past a run boundary and ends k pixels before one: whole-word runs inside, sample-by-sample heads and tails"""
    run_px = RUN_PIXELS[fmt]
    x0, x1 = 512 + k, 1024 - k
    assert 512 % run_px == 0 and 1024 % run_px == 0 and 0 < k < run_px
    run(fmt, *DENSE, MAPS, dev_maps, roi=(x0, 1, x1 - x0, 15), opacity=1.0)


# ---- ordering -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [None, "nv12", "p010"])
def test_two_calls_back_to_back_on_one_frame(fmt, dev_maps):
    """different maps, no synchronise in between: the second call blends over what the first wrote"""
    W, H = size_of(fmt)
    f = DeviceFrame(fmt, W, H)
    steps = [dict(index=0, pal=ref.palette("jet")), dict(index=1, pal=ref.palette("heat", "scaled"), mode="field", channels=(0, 4, 2))]
    for kw in steps:
        f.paint(MAPS, **kw)
    for kw in steps:
        f.draw(dev_maps[id(MAPS)], MAPS, **kw)
    f.check()
    other = DeviceFrame(fmt, W, H)
    for kw in steps[::-1]:
        other.paint(MAPS, **kw)
    assert any(not np.array_equal(a, b) for a, b in zip(other.host, f.host)), "the order does not matter for this case"


def test_six_calls_six_palettes_six_frames(dev_maps):
    """more calls than the ring has slots, each with its own palette and tables, before anything is synchronised"""
    view = frontend.MapView(64)
    fmts = [None, "nv12", "yuy2", "p010", "i444", "i420"]
    pals = [ref.palette(k, a) for k in ("jet", "heat", "grey") for a in ("constant", "scaled")]
    frames = [DeviceFrame(fmt, *size_of(fmt), seed=10 + i) for i, fmt in enumerate(fmts)]
    for i, (f, pal) in enumerate(zip(frames, pals)):
        f.paint(MAPS, i % 3, pal=pal, orientation=i)
    for i, (f, pal) in enumerate(zip(frames, pals)):
        f.draw(dev_maps[id(MAPS)], MAPS, i % 3, pal=pal, orientation=i, view=view)
    for f in frames:
        f.check()
    view.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_equals_host_twin(fmt, dev_maps):
    W, H = size_of(fmt)
    f = DeviceFrame(fmt, W, H)
    kw = dict(orientation=6, cover=LETTERBOX, roi=(3, 1, W - 8, H - 4), mode="field", pal=ref.palette("jet", "scaled"), opacity=0.75)
    f.paint_host_twin(MAPS, 1, **kw)
    f.draw(dev_maps[id(MAPS)], MAPS, 1, **kw)
    f.check()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [None, "nv12"])
def test_invalid_arguments_are_refused_and_nothing_is_written(fmt, dev_maps):
    f = DeviceFrame(fmt, 70, 46)
    name = "BGR" if fmt is None else "HP_YUV_NV12"
    for kw, word in refusal_cases():
        with pytest.raises(_lib.HpError) as e:
            f.draw(dev_maps[id(MAPS)], MAPS, **kw)
        assert e.value.code == _lib.HP_ERR_INVALID and name in str(e.value) and word in str(e.value), (kw, str(e.value))
    small = frontend.MapView(34)  # the maps have 35 cells
    with pytest.raises(_lib.HpError) as e:
        f.draw(dev_maps[id(MAPS)], MAPS, view=small)
    assert e.value.code == _lib.HP_ERR_INVALID and "35" in str(e.value) and "34" in str(e.value)
    L = _lib.lib()
    d = frontend._map_desc(dev_maps[id(MAPS)].ptr.value, MAPS.shape[1:], 0, "max", None, 1.0, (1.0, 1.0), 0, None)
    pp = frontend.map_palette("jet").ctypes.data_as(C.c_void_p)
    if fmt is None:
        rc = L.hp_mapview_draw_u8c3(None, f.bufs[0].ptr, 70, 46, f.strides[0], C.byref(d), pp, C.c_float(0.5), None)
    else:
        rc = L.hp_mapview_draw_yuv(None, C.byref(f.image), C.byref(d), pp, C.c_float(0.5), None)
    assert rc == _lib.HP_ERR_INVALID and "handle" in L.hp_last_error().decode()
    f.check(must_change=False)
    small.close()
