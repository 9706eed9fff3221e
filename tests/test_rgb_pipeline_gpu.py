"""GPU: Pipeline.submit_rgb_images against Pipeline.submit of the same frames converted to BGR on the CPU (tests/rgb_ref.py).  The network inputs are
byte-equal (tests/test_rgb_resize_gpu.py, tests/test_rgb_rois_gpu.py), so the humans must be bit-identical: no tolerance anywhere in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgb_ref  # noqa: E402

from hyperpose_amd import frontend, synth  # noqa: E402
from hyperpose_amd._lib import DevBuf  # noqa: E402
from hyperpose_amd.engine import Model  # noqa: E402
from hyperpose_amd.pipeline import Pipeline  # noqa: E402

pytestmark = pytest.mark.gpu

# the network size of tests/test_yuv_formats_pipeline_gpu.py: on its 20 x 16 feature map a part has at most 80 maxima, so the loose thresholds below
# cannot overflow the parser's candidate lists whatever the random-weight maps look like
NET_W, NET_H = 160, 128


def _frames(n, w, h, fmt, seed):
    """n seeded frames of layout ``fmt`` (uniform-noise BGR pictures through the input generator, random alpha) + their CPU-converted BGR."""
    rng = np.random.default_rng(seed)
    frames = [rgb_ref.from_bgr(p, fmt, rng) for p in synth.images_u8(synth.rng_for(1, salt=seed), n, h, w)]
    return frames, [rgb_ref.to_bgr(f, fmt) for f in frames]


def _device_images(frames, fmt, extra=12):
    """The frames uploaded with a padded, poisoned pitch: (RgbImage list, the buffers to keep alive)."""
    images, keep = [], []
    for f in frames:
        _, whole = rgb_ref.padded(f, extra, 0x5A)
        keep.append(DevBuf.from_numpy(whole))
        images.append(frontend.rgb_image(fmt, keep[-1], f.shape[1], f.shape[0], whole.shape[1]))
    return images, keep


def _same(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert fa.tobytes() == fb.tobytes()


def _humans(batch):
    return sum(len(f) for f in batch)


@pytest.fixture(scope="module")
def lw(hp):
    from hyperpose_amd import engine as E
    m = Model("lw_openpose_mobilenet", NET_W, NET_H)
    w = m.init_weights(11)
    for L in m.layers:  # blow up the two output convolutions: random weights then give O(1) maps, peaks, limbs and humans (tests/test_pipeline_gpu.py)
        if L.op == E.OP_CONV and L.cout in (19, 38) and L.out in [o.tensor for o in m.outputs]:
            w[L.w_off:L.w_off + L.cout * L.cin] *= 400.0
    return m, w


def _pipeline(lw, **kw):
    m, weights = lw
    args = dict(max_batch=8, n_pipes=2, keep_ratio=False, dtype="f32", conf_thresh=0.05, paf_thresh=-1e9, max_frame_wh=(1280, 960))  # a 720p 4-byte frame
    args.update(kw)
    return Pipeline(m, weights, **args)


@pytest.mark.parametrize("keep_ratio", [False, True])
@pytest.mark.parametrize("w,h", [(1280, 720), (NET_W, NET_H)])
def test_host_strided_and_device_feeds_equal_submit_of_converted_frames(hp, lw, w, h, keep_ratio):
    pl = _pipeline(lw, keep_ratio=keep_ratio)
    try:
        for fmt in ("argb", "rgb24"):
            frames, bgr = _frames(4, w, h, fmt, seed=3 + keep_ratio)
            pl.submit(bgr)
            want = pl.collect()
            pl.submit_rgb_images(frames, fmt)  # host, tight, pageable
            host = pl.collect()
            views = [rgb_ref.padded(f, 13, 0x5A)[0] for f in frames]  # host, strided, unpinned: an odd pitch is fine for a host frame
            assert not views[0].flags.c_contiguous
            pl.submit_rgb_images(views, fmt)
            strided = pl.collect()
            images, keep = _device_images(frames, fmt)
            hp.check(hp.lib().hp_device_synchronize())  # the surfaces are complete before the call
            pl.submit_rgb_images(images, on_device=True)
            dev = pl.collect()
            del keep
            print(f"{fmt} {w}x{h} keep_ratio={keep_ratio}: {_humans(want)} humans")
            assert len(host) == len(dev) == len(strided) == 4
            _same(host, want)
            _same(strided, want)
            _same(dev, want)
            assert _humans(want) > 0  # the comparison is not vacuous
    finally:
        pl.close()


def test_tight_pinned_frames_go_up_from_where_they_lie(hp, lw):
    pl = _pipeline(lw, keep_ratio=True)
    try:
        frames, bgr = _frames(3, 640, 480, "bgra", seed=9)
        pl.submit(bgr)
        want = pl.collect()
        size = frames[0].nbytes
        ptr = C.c_void_p()
        hp.check(hp.lib().hp_malloc_host(C.byref(ptr), C.c_size_t(3 * size)))
        pinned = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(3 * size,))
        for i, f in enumerate(frames):
            pinned[i * size:(i + 1) * size] = f.ravel()
        pl.submit_rgb_images([frontend.rgb_image("bgra", ptr.value + i * size, 640, 480) for i in range(3)])
        _same(pl.collect(), want)
        hp.lib().hp_free_host(ptr)
        assert _humans(want) > 0
    finally:
        pl.close()


def test_grey_equals_the_replicated_bgr_frame(hp, lw):
    pl = _pipeline(lw, keep_ratio=True)
    try:
        frames, bgr = _frames(4, 641, 479, "gray", seed=17)
        assert frames[0].ndim == 2 and (bgr[0][..., 0] == frames[0]).all() and (bgr[0][..., 2] == frames[0]).all()
        pl.submit(bgr)
        want = pl.collect()
        pl.submit_rgb_images(frames, "gray")
        _same(pl.collect(), want)
        images, keep = _device_images(frames, "gray", extra=3)
        hp.check(hp.lib().hp_device_synchronize())
        pl.submit_rgb_images(images, on_device=True)
        _same(pl.collect(), want)
        assert _humans(want) > 0
    finally:
        pl.close()


def test_one_batch_mixes_layouts_and_sizes(hp, lw):
    pl = _pipeline(lw, keep_ratio=True)
    try:
        spec = [("bgra", 1280, 720), ("rgb24", 333, 251), ("gray", 640, 480), ("abgr", NET_W, NET_H), ("rgba", 321, 241), ("bgr24", 200, 150)]
        frames, bgr = [], []
        for k, (fmt, w, h) in enumerate(spec):
            f, b = _frames(1, w, h, fmt, seed=40 + k)
            frames += f
            bgr += b
        pl.submit(bgr)
        want = pl.collect()
        pl.submit_rgb_images(frames, [s[0] for s in spec])
        _same(pl.collect(), want)
        images, keep = [], []
        for f, (fmt, w, h) in zip(frames, spec):
            im, bufs = _device_images([f], fmt, extra=8)
            images += im
            keep += bufs
        hp.check(hp.lib().hp_device_synchronize())
        pl.submit_rgb_images(images, on_device=True)
        _same(pl.collect(), want)
        assert _humans(want) > 0
    finally:
        pl.close()


def test_tiling_two_by_two_with_a_quarter_turn(hp, lw):
    pl = _pipeline(lw, keep_ratio=True)
    try:
        pl.set_tiling(2, 2, overlap=(24, 16))
        pl.set_orientation(1)
        frames, bgr = _frames(2, 641, 479, "rgba", seed=23)
        pl.submit(bgr)
        want = pl.collect()
        pl.submit_rgb_images(frames, "rgba")
        _same(pl.collect(), want)
        images, keep = _device_images(frames, "rgba")
        hp.check(hp.lib().hp_device_synchronize())
        pl.submit_rgb_images(images, on_device=True)
        _same(pl.collect(), want)
        assert len(want) == 2 and _humans(want) > 0
    finally:
        pl.close()


def test_flip_ensemble(hp, lw):
    pl = _pipeline(lw)
    try:
        pl.set_flip_ensemble(True)
        frames, bgr = _frames(4, 640, 480, "abgr", seed=29)
        pl.submit(bgr)
        want = pl.collect()
        pl.submit_rgb_images(frames, "abgr")
        _same(pl.collect(), want)
        assert _humans(want) > 0
    finally:
        pl.close()


def test_a_tonemap_on_the_pipeline_does_not_touch_rgb_frames(hp, lw):
    pl = _pipeline(lw)
    try:
        frames, bgr = _frames(2, 320, 240, "bgra", seed=31)
        pl.submit_rgb_images(frames, "bgra")
        want = pl.collect()
        pl.set_tonemap("pq")
        pl.submit_rgb_images(frames, "bgra")
        _same(pl.collect(), want)
    finally:
        pl.close()


def test_rgb_yuv_and_bgr_submits_alternate_with_two_batches_in_flight(hp, lw):
    pl = _pipeline(lw, n_pipes=2)
    try:
        batches = []
        for k, (kind, n, w, h) in enumerate([("bgra", 4, 1280, 720), ("bgr", 3, 640, 480), ("yuy2", 2, 640, 480), ("gray-dev", 4, 641, 479),
                                              ("rgb24", 1, 333, 251), ("nv12", 3, 320, 240), ("bgr", 2, NET_W, NET_H), ("argb-dev", 4, 320, 255)]):
            fmt = kind.split("-")[0]
            if fmt in ("yuy2", "nv12"):
                yuv = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=60 + k), n, h, w), fmt, "bt709", "limited")
                batches.append((kind, fmt, yuv, None))
            else:
                frames, bgr = _frames(n, w, h, "bgr24" if fmt == "bgr" else fmt, seed=60 + k)
                batches.append((kind, fmt, frames, bgr))

        def submit(kind, fmt, frames, keep):
            if fmt in ("yuy2", "nv12"):
                pl.submit_yuv_images(frames, fmt, "bt709", "limited")
            elif kind == "bgr":
                pl.submit(frames)
            elif kind.endswith("-dev"):
                images, bufs = _device_images(frames, fmt)
                keep.append(bufs)
                hp.check(hp.lib().hp_device_synchronize())
                pl.submit_rgb_images(images, on_device=True)
            else:
                pl.submit_rgb_images(frames, fmt)

        alone, keep = [], []
        for kind, fmt, frames, bgr in batches:  # one at a time: YUV batches as themselves, everything else as its converted BGR frames
            submit(kind, fmt, frames, keep) if bgr is None else pl.submit(bgr)
            alone.append(pl.collect())
        got = []
        for start in range(0, 8, 2):
            for kind, fmt, frames, bgr in batches[start:start + 2]:
                submit(kind, fmt, frames, keep)
            assert pl.in_flight == 2
            got += [pl.collect() for _ in range(2)]
        assert [len(g) for g in got] == [len(b[2]) for b in batches]
        for g, a in zip(got, alone):
            _same(g, a)
        assert sum(_humans(a) for a in alone) > 0
    finally:
        pl.close()


def test_max_frame_bytes_bounds_host_frames_only(hp, lw):
    from hyperpose_amd._lib import HP_ERR_CAPACITY, HP_ERR_INVALID, HpError
    pl = _pipeline(lw, max_batch=2, n_pipes=1, max_frame_wh=(640, 480))  # 921 600 bytes
    try:
        frames, bgr = _frames(1, 640, 480, "bgra", seed=50)  # 1 228 800 bytes packed: too many, although the picture is 640 x 480
        with pytest.raises(HpError) as e:
            pl.submit_rgb_images(frames, "bgra")
        assert e.value.code == HP_ERR_CAPACITY and pl.in_flight == 0
        for needle in ("HP_RGB_BGRA32", "640x480", "1228800", "921600"):
            assert needle in str(e.value), str(e.value)
        images, keep = _device_images(frames, "bgra")
        hp.check(hp.lib().hp_device_synchronize())
        pl.submit_rgb_images(images, on_device=True)
        got = pl.collect()
        pl.submit(bgr)  # the BGR form is 921 600 bytes: it fits
        want = pl.collect()
        _same(got, want)
        assert _humans(want) > 0
        grey, _ = _frames(1, 1280, 720, "gray", seed=51)  # 921 600 bytes in its own form: fits, its BGR form would not
        pl.submit_rgb_images(grey, "gray")
        assert len(pl.collect()) == 1
        with pytest.raises(HpError) as e:  # batch 3 > max_batch 2
            pl.submit_rgb_images(grey * 3, "gray")
        assert e.value.code == HP_ERR_CAPACITY
        with pytest.raises(HpError) as e:  # a device plane of 4-byte pixels at an odd pitch
            pl.submit_rgb_images([frontend.rgb_image("bgra", images[0].data, 600, 480, images[0].stride - 2)], on_device=True)
        assert e.value.code == HP_ERR_INVALID and "HP_RGB_BGRA32" in str(e.value)
        with pytest.raises(ValueError):
            pl.submit_rgb_images(frames, "bgra", on_device=True)  # host arrays are not device surfaces
        with pytest.raises(ValueError):
            pl.submit_rgb_images(frames, "rgb24")  # [h, w, 4] is no 3-byte frame
        assert pl.in_flight == 0
    finally:
        pl.close()
