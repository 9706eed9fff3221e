"""GPU: the stream pipeline's tiled mode (hp_pipeline_set_tiling).  A 1 x 1 tiling is tiling off, byte for byte; any other tiling equals
the same result composed by hand from the public pieces: hp_tile_plan -> hp_resize_rois_* -> hp_engine_infer_u8 -> the parser's blocking
call -> hp_resume_ratio -> hp_humans_to_frame -> hp_humans_merge.  No tolerance anywhere in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hyperpose_amd import engine as E  # noqa: E402
from hyperpose_amd import frontend, synth  # noqa: E402
from hyperpose_amd._lib import HP_ERR_CAPACITY, HP_ERR_STATE, HUMAN_DTYPE, DevBuf, HpError, Human  # noqa: E402
from hyperpose_amd.parser import Paf  # noqa: E402
from hyperpose_amd.pipeline import Pipeline  # noqa: E402

pytestmark = pytest.mark.gpu

# the recipe of tests/test_yuv_formats_pipeline_gpu.py: on the 20 x 16 feature map of a 160 x 128 input a part has at most 80 maxima, so the
# loose thresholds cannot overflow the parser's candidate lists whatever the random-weight maps look like
NET_W, NET_H = 160, 128
FW, FH = 640, 360
MERGE = dict(min_common=3, tol=0.25)
PLANS = [dict(cols=2, rows=2, overlap=(32, 32), with_full=False), dict(cols=2, rows=1, overlap=(0, 0), with_full=True)]


@pytest.fixture(scope="module")
def lw(hp):
    m = E.Model("lw_openpose_mobilenet", NET_W, NET_H)
    w = m.init_weights(11)
    for L in m.layers:  # blow up the two output convolutions: random weights then give O(1) maps, peaks, limbs and humans
        if L.op == E.OP_CONV and L.cout in (19, 38) and L.out in [o.tensor for o in m.outputs]:
            w[L.w_off:L.w_off + L.cout * L.cin] *= 400.0
    return m, w


@pytest.fixture(scope="module")
def by_hand_stages(hp, lw):
    m, w = lw
    return E.Engine.from_model(m, w, max_batch=4, dtype="f32"), Paf(conf_thresh=0.05, paf_thresh=-1e9, max_batch=4)


def _pipeline(lw, **kw):
    m, weights = lw
    args = dict(max_batch=8, n_pipes=2, keep_ratio=False, dtype="f32", conf_thresh=0.05, paf_thresh=-1e9, max_frame_wh=(1280, 720))
    args.update(kw)
    return Pipeline(m, weights, **args)


def _bgr(n, w, h, seed):
    return list(synth.images_u8(synth.rng_for(1, salt=seed), n, h, w))


def _device_yuv(hp, bgr, fmt, pitch=34):
    """The frames as device-resident surfaces with padded pitch: (YuvImage list, buffers to keep alive)."""
    images, keep = [], []
    for planes in synth.bgr_to_yuv(np.stack(bgr), fmt, "bt709", "limited"):
        w, h = frontend.yuv_size_of_planes(fmt, planes)
        bufs, strides = frontend.yuv_upload(planes, fmt, pitch)
        images.append(frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, w, h, "bt709", "limited"))
        keep.append(bufs)
    hp.check(hp.lib().hp_device_synchronize())  # the surfaces are complete before a submit
    return images, keep


def _same(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert fa.tobytes() == fb.tobytes()


def _parse_paf(stages, slots):
    eng, paf = stages
    maps = eng.inference(slots)
    return paf.process_batch(np.stack([m[0][1] for m in maps]), np.stack([m[1][1] for m in maps]))


def _compose(hp, src, w, h, fmt, plan, keep_ratio, parse, net=(NET_W, NET_H)):
    """One frame by hand.  `src`: a device BGR buffer or a YuvImage.  Returns (merged humans, humans before the merge per region)."""
    rois = frontend.plan_tiles(w, h, plan["cols"], plan["rows"], plan["overlap"], plan["with_full"], fmt=fmt)
    dst = DevBuf(len(rois) * net[0] * net[1] * 3)
    frontend.resize_rois(src, rois, dst, net[0], net[1], keep_ratio, (0, 0, 0), sw=w, sh=h)
    hp.check(hp.lib().hp_device_synchronize())
    per_slot = parse(dst.to_numpy(np.uint8, (len(rois), net[1], net[0], 3)))
    cand, region = [], []
    for r, (roi, hs) in enumerate(zip(rois, per_slot)):
        hs = np.ascontiguousarray(hs, HUMAN_DTYPE).copy()
        if keep_ratio and len(hs):
            hp.lib().hp_resume_ratio(hs.ctypes.data_as(C.POINTER(Human)), len(hs), roi[2], roi[3], net[0], net[1])
        cand.append(frontend.humans_to_frame(hs, roi, w, h))
        region += [r] * len(hs)
    return frontend.merge_humans(np.concatenate(cand), region, w, h, **MERGE), [len(c) for c in cand]


@pytest.mark.parametrize("keep_ratio", [False, True])
def test_one_tile_is_tiling_off(hp, lw, keep_ratio):
    pl = _pipeline(lw, keep_ratio=keep_ratio)
    try:
        bgr = _bgr(5, FW, FH, 3) + _bgr(2, NET_W, NET_H, 4) + _bgr(1, 97, 61, 5)
        pl.submit(bgr)
        want = pl.collect()
        images = {fmt: _device_yuv(hp, _bgr(8, FW, FH, 6), fmt) for fmt in ("nv12", "p010")}
        want_yuv = {}
        for fmt, (ims, _) in images.items():
            pl.submit_yuv_images(ims, on_device=True)
            want_yuv[fmt] = pl.collect()
        pl.set_tiling(1, 1, overlap=(0, 0), with_full=False, **MERGE)
        pl.submit(bgr)
        _same(pl.collect(), want)
        for fmt, (ims, _) in images.items():
            pl.submit_yuv_images(ims, on_device=True)
            _same(pl.collect(), want_yuv[fmt])
        pl.set_tiling(None)
        pl.submit(bgr)
        _same(pl.collect(), want)
        assert sum(len(f) for f in want) > 0 and all(sum(len(f) for f in v) > 0 for v in want_yuv.values())
    finally:
        pl.close()


@pytest.mark.parametrize("keep_ratio", [False, True])
@pytest.mark.parametrize("plan", PLANS, ids=["2x2-overlap32", "2x1-with-full"])
def test_tiled_pipeline_equals_the_composition_by_hand(hp, lw, by_hand_stages, plan, keep_ratio):
    pl = _pipeline(lw, keep_ratio=keep_ratio)
    parse = lambda slots: _parse_paf(by_hand_stages, slots)  # noqa: E731
    try:
        pl.set_tiling(plan["cols"], plan["rows"], plan["overlap"], plan["with_full"], **MERGE)
        bgr = _bgr(2, FW, FH, 7 + keep_ratio)
        feeds = [("bgr", None)] + [(fmt, _device_yuv(hp, bgr, fmt)) for fmt in ("nv12", "p010")] + [("yuy2-host", None)]
        for kind, dev in feeds:
            if kind == "bgr":
                pl.submit(bgr)
                srcs, fmt = [DevBuf.from_numpy(f) for f in bgr], None
            elif kind == "yuy2-host":
                fmt = "yuy2"
                pl.submit_yuv_images(synth.bgr_to_yuv(np.stack(bgr), fmt, "bt709", "limited"), fmt, "bt709", "limited")
                srcs, keep = _device_yuv(hp, bgr, fmt, pitch=0)
            else:
                fmt = kind
                pl.submit_yuv_images(dev[0], on_device=True)
                srcs = dev[0]
            got = pl.collect()
            assert len(got) == len(bgr), "n_frames counts frames, not slots"
            for f, src in enumerate(srcs):
                want, before = _compose(hp, src, FW, FH, fmt, plan, keep_ratio, parse)
                print(f"{kind} keep_ratio={keep_ratio} frame {f}: {before} humans per region, {len(want)} after the merge")
                assert max(before) > 0  # the comparison is not vacuous
                assert got[f].tobytes() == want.tobytes()
                assert len(want) <= sum(before)
    finally:
        pl.close()


def test_capacity_and_call_order(hp, lw):
    pl = _pipeline(lw, max_batch=8, n_pipes=2)
    try:
        bgr = _bgr(3, FW, FH, 9)
        yuv = synth.bgr_to_yuv420(np.stack(bgr), "nv12")
        pl.set_tiling(2, 2, overlap=(32, 32))
        with pytest.raises(HpError) as e:  # 3 frames x 4 regions > 8
            pl.submit(bgr)
        assert e.value.code == HP_ERR_CAPACITY and "4" in str(e.value) and "8" in str(e.value) and pl.in_flight == 0
        images, keep = _device_yuv(hp, bgr, "nv12")
        with pytest.raises(HpError) as e:
            pl.submit_yuv_images(images, on_device=True)
        assert e.value.code == HP_ERR_CAPACITY and pl.in_flight == 0
        with pytest.raises(HpError) as e:  # the legacy 4:2:0 submit has no tiled form
            pl.submit_yuv([f for f in yuv[:2]], "nv12")
        assert e.value.code == HP_ERR_STATE and "hp_pipeline_submit_yuv_images" in str(e.value) and pl.in_flight == 0
        pl.submit(bgr[:2])
        for args in [(None,), (3, 1)]:
            with pytest.raises(HpError) as e:  # not while a batch is in flight
                pl.set_tiling(*args)
            assert e.value.code == HP_ERR_STATE
        assert len(pl.collect()) == 2
        with pytest.raises(HpError) as e:  # 9 regions per frame never fit a batch of 8
            pl.set_tiling(3, 3)
        assert e.value.code == HP_ERR_CAPACITY
        pl.set_tiling(None)
        pl.submit_yuv([f for f in yuv], "nv12")
        assert len(pl.collect()) == 3
    finally:
        pl.close()


def test_two_tiled_batches_in_flight_alternate_bgr_and_device_yuv(hp, lw):
    pl = _pipeline(lw, n_pipes=2)
    try:
        pl.set_tiling(2, 2, overlap=(32, 32), **MERGE)
        batches = [_bgr(2, FW, FH, 20 + k) if k != 2 else _bgr(1, 333, 251, 22) for k in range(4)]
        yuv = {k: _device_yuv(hp, batches[k], "nv12") for k in (1, 3)}
        feed = lambda k: pl.submit_yuv_images(yuv[k][0], on_device=True) if k in yuv else pl.submit(batches[k])  # noqa: E731
        alone = []
        for k in range(4):
            feed(k)
            alone.append(pl.collect())
        got = []
        for start in (0, 2):
            feed(start), feed(start + 1)
            assert pl.in_flight == 2
            got += [pl.collect(), pl.collect()]
        assert [len(g) for g in got] == [len(b) for b in batches]
        for g, a in zip(got, alone):
            _same(g, a)
        assert sum(len(f) for a in alone for f in a) > 0
    finally:
        pl.close()


def test_pose_proposal_parser_behind_the_shared_tail(hp):
    from hyperpose_amd.parser import PoseProposal
    in_w = in_h = 192
    m = E.Model("pose_proposal_resnet50", in_w, in_h)
    weights = m.init_weights(5)
    pl = Pipeline(m, weights, max_batch=4, n_pipes=1, keep_ratio=True, dtype="f32", parser="ppn", thresholds=(0.02, 0.01, 0.3), max_frame_wh=(1280, 720))
    eng = E.Engine.from_model(m, weights, max_batch=4, dtype="f32")
    par = PoseProposal((in_w, in_h), 0.02, 0.01, 0.3, max_batch=4)
    g6 = in_w // 32

    def parse(slots):
        maps = eng.inference(slots)
        n = len(slots)
        return par.process_batch([np.stack([fm[i][1] for fm in maps]) for i in range(6)] + [np.stack([fm[6][1] for fm in maps]).reshape(n, 17, 9, 9, g6, g6)])

    plan = dict(cols=2, rows=1, overlap=(64, 0), with_full=False)
    try:
        pl.set_tiling(plan["cols"], plan["rows"], plan["overlap"], **MERGE)
        bgr = _bgr(2, FW, FH, 11)
        pl.submit(bgr)
        got = pl.collect()
        assert len(got) == 2
        for f, frame in enumerate(bgr):
            want, before = _compose(hp, DevBuf.from_numpy(frame), FW, FH, None, plan, True, parse, net=(in_w, in_h))
            print(f"pose proposal frame {f}: {before} humans per region, {len(want)} after the merge")
            assert got[f].tobytes() == want.tobytes()
    finally:
        pl.close()
