"""GPU: Pipeline.set_orientation - stored frames that are turned / mirrored, read upright inside the fused resize - against Pipeline.submit of the
same frames oriented on the CPU (tests/orient_ref.py) with orientation 0.  The network inputs are byte-equal (tests/test_resize_oriented_gpu.py), so
the humans must be bit-identical: no tolerance anywhere in this file.  The fixture, the weights trick and the thresholds are those of
tests/test_hdr_pipeline_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_ref  # noqa: E402
import orient_ref  # noqa: E402
import yuv_formats_ref as ref  # noqa: E402

from hyperpose_amd import frontend, synth  # noqa: E402
from hyperpose_amd._lib import HP_ERR_INVALID, HP_ERR_STATE, DevBuf, HpError  # noqa: E402
from hyperpose_amd.engine import Model  # noqa: E402
from hyperpose_amd.pipeline import Pipeline  # noqa: E402

pytestmark = pytest.mark.gpu

NET_W, NET_H = 160, 128
W, H = 320, 240
CODES = [1, 2, 3, 5]


def _flat(planes):
    return np.concatenate([p.view(np.uint8).ravel() for p in planes])


def _same(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert fa.tobytes() == fb.tobytes()


def _humans(batch):
    return sum(len(f) for f in batch)


def _device_images(frames, fmt, matrix, range_, pitch=34):
    images, keep = [], []
    for planes in frames:
        w, h = frontend.yuv_size_of_planes(fmt, planes)
        bufs, strides = frontend.yuv_upload(planes, fmt, pitch)
        images.append(frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, w, h, matrix, range_))
        keep.append(bufs)
    return images, keep


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
    args = dict(max_batch=8, n_pipes=2, keep_ratio=False, dtype="f32", conf_thresh=0.05, paf_thresh=-1e9, max_frame_wh=(1280, 720))
    args.update(kw)
    return Pipeline(m, weights, **args)


@pytest.fixture(scope="module")
def stored(hp):
    """Four stored BGR frames, the same pictures as NV12 (plane lists) and what the library makes of those (their BGR reading)."""
    bgr = list(synth.images_u8(synth.rng_for(1, salt=31), 4, H, W))
    nv12 = synth.bgr_to_yuv(np.stack(bgr), "nv12", "bt709", "limited")
    nv12_bgr = [ref.to_bgr(_flat(f), "nv12", W, H, "bt709", "limited") for f in nv12]
    return bgr, nv12, nv12_bgr


@pytest.mark.parametrize("keep_ratio", [False, True])
def test_stored_frames_equal_submit_of_upright_frames(hp, lw, stored, keep_ratio):
    bgr, nv12, nv12_bgr = stored
    pl = _pipeline(lw, keep_ratio=keep_ratio)
    try:
        images, keep = _device_images(nv12, "nv12", "bt709", "limited")
        hp.check(hp.lib().hp_device_synchronize())  # the surfaces are complete before the call
        seen = []
        for code in CODES:
            pl.set_orientation(0)
            pl.submit([orient_ref.orient(f, code) for f in bgr])
            want = pl.collect()
            pl.submit([orient_ref.orient(f, code) for f in nv12_bgr])
            want_nv12 = pl.collect()
            pl.set_orientation(code)
            pl.submit(bgr)
            _same(pl.collect(), want)
            pl.submit_yuv_images(nv12, "nv12", "bt709", "limited")
            _same(pl.collect(), want_nv12)
            pl.submit_yuv_images(images, on_device=True)
            _same(pl.collect(), want_nv12)
            print(f"code {code} keep_ratio={keep_ratio}: {_humans(want)} / {_humans(want_nv12)} humans")
            assert len(want) == 4 and _humans(want) > 0 and _humans(want_nv12) > 0  # the comparison is not vacuous
            seen.append(b"".join(f.tobytes() for f in want))
        assert len(set(seen)) == len(CODES), "two orientations gave the same humans: the test frames are too tame"
        del keep
    finally:
        pl.close()


def test_tiled_and_oriented(hp, lw, stored):
    bgr, nv12, nv12_bgr = stored
    pl = _pipeline(lw, keep_ratio=True)
    try:
        pl.set_tiling(2, 1, overlap=16)
        for code in (1, 2):
            pl.set_orientation(0)
            pl.submit([orient_ref.orient(f, code) for f in bgr[:2]])
            want = pl.collect()
            pl.submit([orient_ref.orient(f, code) for f in nv12_bgr[:2]])
            want_nv12 = pl.collect()
            pl.set_orientation(code)
            pl.submit(bgr[:2])
            _same(pl.collect(), want)
            pl.submit_yuv_images(nv12[:2], "nv12", "bt709", "limited")
            _same(pl.collect(), want_nv12)
            assert len(want) == 2 and _humans(want) > 0 and _humans(want_nv12) > 0
    finally:
        pl.close()


def test_p010_with_a_tonemap_and_an_orientation(hp, lw):
    pl = _pipeline(lw)
    try:
        yuv = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=33), 4, H, W), "p010", "bt2020", "limited")
        A, M, O = frontend.tonemap_tables("pq", True)
        hdr = [hdr_ref.to_bgr(_flat(f), "p010", W, H, "bt2020", "limited", A, M, O, True) for f in yuv]
        pl.submit([orient_ref.orient(f, 3) for f in hdr])
        want = pl.collect()
        pl.set_tonemap("pq", True)
        pl.set_orientation(3)
        pl.submit_yuv_images(yuv, "p010", "bt2020", "limited")
        _same(pl.collect(), want)
        assert _humans(want) > 0
    finally:
        pl.close()


def test_set_orientation_rules(hp, lw, stored):
    bgr, nv12, nv12_bgr = stored
    pl, fresh = _pipeline(lw), _pipeline(lw)
    try:
        for bad in (8, -1):
            with pytest.raises(HpError) as e:
                pl.set_orientation(bad)
            assert e.value.code == HP_ERR_INVALID and "orientation" in str(e.value)
        pl.set_orientation(1)
        pl.submit(bgr)
        with pytest.raises(HpError) as e:  # not while batches are in flight
            pl.set_orientation(0)
        assert e.value.code == HP_ERR_STATE
        pl.collect()
        with pytest.raises(HpError) as e:  # the legacy 4:2:0 submit is not available while oriented
            pl.submit_yuv([_flat(nv12[0]).reshape(H * 3 // 2, W)], "nv12")
        assert e.value.code == HP_ERR_STATE and "orientation" in str(e.value)
        pl.set_orientation(0)  # off again: as a fresh pipeline
        pl.submit(bgr)
        fresh.submit(bgr)
        _same(pl.collect(), fresh.collect())
        pl.submit_yuv([_flat(nv12[0]).reshape(H * 3 // 2, W)], "nv12")
        fresh.submit_yuv([_flat(nv12[0]).reshape(H * 3 // 2, W)], "nv12")
        _same(pl.collect(), fresh.collect())
    finally:
        pl.close()
        fresh.close()


def test_overlay_draws_upright_humans_into_the_stored_frame(hp, lw, stored):
    bgr, nv12, nv12_bgr = stored
    pl = _pipeline(lw)
    try:
        for code in (1, 5):
            pl.set_orientation(code)
            pl.submit(bgr[:1])
            upright = pl.collect()[0]
            assert len(upright) > 0
            to_stored = frontend.humans_orient(upright, code, True)
            assert to_stored.tobytes() == orient_ref.humans_orient(upright, code, True).tobytes()
            host = bgr[0].copy()
            frontend.draw_humans_host(host, to_stored)
            dev = DevBuf.from_numpy(bgr[0])
            frontend.draw_humans(dev, to_stored, w=W, h=H)
            hp.check(hp.lib().hp_device_synchronize())
            assert dev.to_numpy(np.uint8, (H, W, 3)).tobytes() == host.tobytes()
            assert host.tobytes() != bgr[0].tobytes(), "nothing was drawn"
    finally:
        pl.close()
