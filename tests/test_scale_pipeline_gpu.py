"""GPU: Pipeline.set_scale_ensemble against the same steps taken by hand: every frame's network-sized slot (frontend.resize_host) through an
Engine with the scale ensemble on, the PAF parser on the merged device maps, resume_ratio when the aspect ratio is kept.  The humans must be
identical: no tolerance anywhere in this file.  The fixture, the weights trick and the thresholds are those of tests/test_flip_pipeline_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from hyperpose_amd import engine as E
from hyperpose_amd import frontend, synth
from hyperpose_amd._lib import HP_ERR_CAPACITY, HP_ERR_INVALID, HP_ERR_STATE, DevBuf, HpError, Human
from hyperpose_amd.engine import Model
from hyperpose_amd.parser import Paf
from hyperpose_amd.pipeline import Pipeline

pytestmark = pytest.mark.gpu

NET_W, NET_H = 160, 128
W, H = 1280, 720
MAX_BATCH = 8
SCALES = [0.5]
THRESH = dict(conf_thresh=0.05, paf_thresh=-1e9)


def _same(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert fa.tobytes() == fb.tobytes()


def _humans(batch):
    return sum(len(f) for f in batch)


@pytest.fixture(scope="module")
def lw(hp):
    m = Model("lw_openpose_mobilenet", NET_W, NET_H)
    w = m.init_weights(11)
    for L in m.layers:  # blow up the two output convolutions: random weights then give O(1) maps, peaks, limbs and humans (tests/test_pipeline_gpu.py)
        if L.op == E.OP_CONV and L.cout in (19, 38) and L.out in [o.tensor for o in m.outputs]:
            w[L.w_off:L.w_off + L.cout * L.cin] *= 400.0
    return m, w


def _pipeline(lw, **kw):
    m, weights = lw
    args = dict(max_batch=MAX_BATCH, n_pipes=2, keep_ratio=False, dtype="f32", max_frame_wh=(W, H), **THRESH)
    args.update(kw)
    return Pipeline(m, weights, **args)


@pytest.fixture(scope="module")
def pictures(hp):
    """Four 1280 x 720 BGR frames."""
    return list(synth.images_u8(synth.rng_for(1, salt=79), 4, H, W))


@pytest.fixture(scope="module")
def by_hand(hp, lw):
    """slots [n, NET_H, NET_W, 3] -> the humans of the ensemble, per slot: Engine with the scale ensemble on, the parser on the merged device maps."""
    m, weights = lw
    eng = E.Engine.from_model(m, weights, max_batch=MAX_BATCH, dtype="f32")
    eng.set_scale_ensemble(SCALES)
    paf = Paf(max_batch=MAX_BATCH, **THRESH)

    def run(slots, keep_ratio):
        dev = DevBuf.from_numpy(np.ascontiguousarray(slots))
        eng.enqueue_u8(dev, len(slots))
        eng.synchronize()
        (_, cs, dconf), (_, ps, dpaf) = eng.outputs
        out = paf.process_batch_device(dconf, dpaf, len(slots), cs, ps)
        if keep_ratio:
            for hs in out:
                if len(hs):
                    hp.lib().hp_resume_ratio(hs.ctypes.data_as(C.POINTER(Human)), len(hs), W, H, NET_W, NET_H)
        return out

    yield run
    paf.close()
    eng.close()


@pytest.mark.parametrize("keep_ratio", [False, True])
def test_pipeline_ensemble_equals_engine_ensemble_and_parser(hp, lw, pictures, by_hand, keep_ratio):
    bgr = pictures
    pl = _pipeline(lw, keep_ratio=keep_ratio)
    try:
        pl.submit(bgr)
        off = pl.collect()
        pl.set_scale_ensemble(SCALES)
        slots = np.stack([frontend.resize_host(f, NET_W, NET_H, keep_ratio) for f in bgr])
        want = by_hand(slots, keep_ratio)
        pl.submit(bgr)
        got = pl.collect()
        _same(got, want)
        print(f"keep_ratio={keep_ratio}: {_humans(off)} humans off, {_humans(want)} on")
        assert len(want) == 4 and _humans(want) > 0
        assert any(a.tobytes() != b.tobytes() for a, b in zip(got, off)), "the ensemble changed no frame's humans: the frames are too tame"
    finally:
        pl.close()


def test_capacity_rules(hp, lw, pictures):
    bgr = pictures
    pl = _pipeline(lw)
    try:
        pl.set_scale_ensemble(SCALES)
        with pytest.raises(HpError) as e:  # 5 frames untiled: 10 network images > 8
            pl.submit(bgr + bgr[:1])
        assert e.value.code == HP_ERR_CAPACITY and "scale ensemble" in str(e.value) and pl.in_flight == 0
        pl.set_tiling(2, 1, overlap=16)  # the tiling setter comes last: 2 regions x 2 scales per frame, 2 frames per submit
        pl.submit(bgr[:2])
        tiled = pl.collect()
        assert len(tiled) == 2 and _humans(tiled) > 0
        with pytest.raises(HpError) as e:
            pl.submit(bgr[:3])
        assert e.value.code == HP_ERR_CAPACITY and "2 frames per submit" in str(e.value) and pl.in_flight == 0
        pl.set_flip_ensemble(True)  # 2 regions x 2 scales x 2 = 8: one frame per submit
        pl.submit(bgr[:1])
        assert len(pl.collect()) == 1
        with pytest.raises(HpError) as e:
            pl.submit(bgr[:2])
        assert e.value.code == HP_ERR_CAPACITY and pl.in_flight == 0
        with pytest.raises(HpError) as e:  # 3 regions x 2 x 2 do not fit: the tiling setter refuses
            pl.set_tiling(3, 1)
        assert e.value.code == HP_ERR_CAPACITY and "scale ensemble" in str(e.value)
        with pytest.raises(HpError) as e:  # 2 regions x 3 scales x 2 do not fit: the scale setter refuses, the pipes keep K = 2
            pl.set_scale_ensemble([0.5, 0.75])
        assert e.value.code == HP_ERR_CAPACITY and "3 scales" in str(e.value)
        pl.submit(bgr[:1])
        assert len(pl.collect()) == 1
        pl.set_flip_ensemble(False)
        pl.set_scale_ensemble([])
        pl.set_tiling(3, 2)  # the scale setter comes last: 6 regions x 2 scales > 8
        with pytest.raises(HpError) as e:
            pl.set_scale_ensemble(SCALES)
        assert e.value.code == HP_ERR_CAPACITY and "6 regions" in str(e.value)
        pl.submit(bgr[:1])  # (still off, still tiled 3 x 2)
        assert len(pl.collect()) == 1
    finally:
        pl.close()


def test_state_rules_and_off_again(hp, lw, pictures):
    bgr = pictures
    pl, fresh = _pipeline(lw), _pipeline(lw)
    try:
        pl.set_scale_ensemble(SCALES)
        pl.submit(bgr)
        for scales in ([], SCALES):
            with pytest.raises(HpError) as e:  # not while batches are in flight
                pl.set_scale_ensemble(scales)
            assert e.value.code == HP_ERR_STATE and "in flight" in str(e.value)
        pl.collect()
        pl.set_scale_ensemble([])  # off again: as a fresh pipeline, full batches included
        for batch in (bgr, bgr + bgr):
            pl.submit(batch)
            fresh.submit(batch)
            a, b = pl.collect(), fresh.collect()
            _same(a, b)
            assert _humans(a) > 0
    finally:
        pl.close()
        fresh.close()


def test_a_pose_proposal_pipeline_is_refused(hp):
    m = Model("pose_proposal_resnet50", 96, 96)
    pl = Pipeline(m, m.init_weights(3), max_batch=2, n_pipes=1, parser="ppn", max_frame_wh=(96, 96))
    try:
        with pytest.raises(HpError) as e:
            pl.set_scale_ensemble(SCALES)
        assert e.value.code == HP_ERR_INVALID and "HP_PARSER_PPN" in str(e.value)
    finally:
        pl.close()
