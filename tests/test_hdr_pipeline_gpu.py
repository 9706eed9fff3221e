"""GPU: Pipeline.set_tonemap - P010 / I010 frames of submit_yuv_images tone-mapped inside the fused resize - against Pipeline.submit of the same
frames converted on the CPU (tests/hdr_ref.py with the library's tables).  The network inputs are byte-equal (tests/test_hdr_gpu.py), so the
humans must be bit-identical: no tolerance anywhere in this file.  The fixture, the weights trick and the thresholds are those of
tests/test_yuv_formats_pipeline_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_ref  # noqa: E402
import yuv_formats_ref as ref  # noqa: E402

from hyperpose_amd import frontend, synth  # noqa: E402
from hyperpose_amd._lib import HP_ERR_INVALID, HP_ERR_STATE, HpError  # noqa: E402
from hyperpose_amd.engine import Model  # noqa: E402
from hyperpose_amd.pipeline import Pipeline  # noqa: E402

pytestmark = pytest.mark.gpu

NET_W, NET_H = 160, 128
MATRIX, RANGE = "bt2020", "limited"


def _flat(planes):
    return np.concatenate([p.view(np.uint8).ravel() for p in planes])


def _frames(n, w, h, fmt, seed, transfer="pq", to_bt709=True):
    """n seeded frames as plane lists (the input generator's pictures, their code values read as PQ / HLG), their CPU tone-mapped BGR and their
    CPU SDR-converted BGR."""
    yuv = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=seed), n, h, w), fmt, MATRIX, RANGE)
    A, M, O = frontend.tonemap_tables(transfer, to_bt709)
    hdr = [hdr_ref.to_bgr(_flat(f), fmt, w, h, MATRIX, RANGE, A, M, O, to_bt709) for f in yuv]
    sdr = [ref.to_bgr(_flat(f), fmt, w, h, MATRIX, RANGE) for f in yuv]
    return yuv, hdr, sdr


def _device_images(frames, fmt, pitch=34):
    images, keep = [], []
    for planes in frames:
        w, h = frontend.yuv_size_of_planes(fmt, planes)
        bufs, strides = frontend.yuv_upload(planes, fmt, pitch)
        images.append(frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, w, h, MATRIX, RANGE))
        keep.append(bufs)
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
    args = dict(max_batch=8, n_pipes=2, keep_ratio=False, dtype="f32", conf_thresh=0.05, paf_thresh=-1e9, max_frame_wh=(1280, 720))
    args.update(kw)
    return Pipeline(m, weights, **args)


@pytest.mark.parametrize("keep_ratio", [False, True])
@pytest.mark.parametrize("w,h", [(320, 240), (NET_W, NET_H)])
def test_host_and_device_feeds_equal_submit_of_tone_mapped_frames(hp, lw, w, h, keep_ratio):
    pl = _pipeline(lw, keep_ratio=keep_ratio)
    try:
        for fmt, transfer, to_bt709 in [("p010", "pq", True), ("p010", "hlg", False), ("i010", "hlg", True)]:
            yuv, hdr, sdr = _frames(4, w, h, fmt, seed=3 + keep_ratio, transfer=transfer, to_bt709=to_bt709)
            pl.submit(hdr)
            want = pl.collect()
            pl.submit(sdr)
            want_sdr = pl.collect()
            pl.set_tonemap(transfer, to_bt709)
            pl.submit_yuv_images(yuv, fmt, MATRIX, RANGE)
            host = pl.collect()
            images, keep = _device_images(yuv, fmt)
            hp.check(hp.lib().hp_device_synchronize())  # the surfaces are complete before the call
            pl.submit_yuv_images(images, on_device=True)
            dev = pl.collect()
            print(f"{fmt} {transfer} to_bt709={to_bt709} {w}x{h} keep_ratio={keep_ratio}: {_humans(want)} humans (SDR reading: {_humans(want_sdr)})")
            assert len(host) == len(dev) == 4
            _same(host, want)
            _same(dev, want)
            assert _humans(want) > 0  # the comparison is not vacuous
            # off again: the SDR bytes are back
            pl.set_tonemap(None)
            pl.submit_yuv_images(yuv, fmt, MATRIX, RANGE)
            _same(pl.collect(), want_sdr)
            pl.submit_yuv_images(images, on_device=True)
            _same(pl.collect(), want_sdr)
            del keep
            assert any(a.tobytes() != b.tobytes() for a, b in zip(want, want_sdr)), "tone-mapping changed nothing: the test frames are too tame"
    finally:
        pl.close()


@pytest.mark.parametrize("keep_ratio", [False, True])
def test_tiled_with_a_tonemap_equals_tiled_converted_frames(hp, lw, keep_ratio):
    pl = _pipeline(lw, keep_ratio=keep_ratio)
    try:
        yuv, hdr, _ = _frames(2, 320, 240, "p010", seed=9)
        pl.set_tiling(2, 2, overlap=16)
        pl.submit(hdr)
        want = pl.collect()
        pl.set_tonemap("pq")
        pl.submit_yuv_images(yuv, "p010", MATRIX, RANGE)
        _same(pl.collect(), want)
        images, keep = _device_images(yuv, "p010")
        hp.check(hp.lib().hp_device_synchronize())
        pl.submit_yuv_images(images, on_device=True)
        _same(pl.collect(), want)
        assert len(want) == 2 and _humans(want) > 0
    finally:
        pl.close()


def test_a_batch_mixing_nv12_and_p010_converts_nv12_as_before(hp, lw):
    pl = _pipeline(lw)
    try:
        p010, hdr, _ = _frames(2, 320, 240, "p010", seed=21)
        nv12 = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=22), 2, 240, 320), "nv12", "bt709", "limited")
        nv12_bgr = [ref.to_bgr(_flat(f), "nv12", 320, 240, "bt709", "limited") for f in nv12]
        pl.submit([nv12_bgr[0], hdr[0], hdr[1], nv12_bgr[1]])
        want = pl.collect()
        pl.set_tonemap("pq")
        pl.submit_yuv_images([nv12[0], p010[0], p010[1], nv12[1]], ["nv12", "p010", "p010", "nv12"], ["bt709", MATRIX, MATRIX, "bt709"], RANGE)
        _same(pl.collect(), want)
        assert _humans(want) > 0
    finally:
        pl.close()


def test_set_tonemap_rules(hp, lw):
    pl = _pipeline(lw)
    try:
        yuv, hdr, _ = _frames(1, NET_W, NET_H, "p010", seed=5)
        pl.submit(hdr)
        want = pl.collect()
        pl.set_tonemap("pq")
        with pytest.raises(HpError) as e:  # a refused description leaves the pipeline as it was
            pl.set_tonemap("pq", white_nits=2000.0, peak_nits=1000.0)
        assert e.value.code == HP_ERR_INVALID
        with pytest.raises(HpError) as e:
            pl.set_tonemap(7)
        assert e.value.code == HP_ERR_INVALID and "transfer" in str(e.value)
        pl.submit_yuv_images(yuv, "p010", MATRIX, RANGE)
        with pytest.raises(HpError) as e:  # not while batches are in flight
            pl.set_tonemap(None)
        assert e.value.code == HP_ERR_STATE
        with pytest.raises(HpError) as e:
            pl.set_tonemap("hlg")
        assert e.value.code == HP_ERR_STATE
        _same(pl.collect(), want)
    finally:
        pl.close()
