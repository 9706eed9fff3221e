"""GPU: the engine's flip ensemble (hp_engine_set_flip_ensemble*) on lw_openpose_vggtiny at a small input, max_batch 4, in every arithmetic and
launch form: the merged outputs are hp_flip_merge_host of the plain engine's outputs on [frames, flipped frames], bit for bit; the ensemble is
equivariant; the capacity and state rules; off again the engine is the plain engine.

Equivariance is compared bit for bit; on the NEGATED channels (the PAF x components) after adding +0.0f to both sides, which changes one thing
only: -0 becomes +0.  Where a flipped-back map
equals the map exactly (a == b) a negated channel holds 0.5f * (a - b) = +0 on one side and -(+0) = -0 on the other; no function f with
f(a, b) == -f(b, a) bit for bit exists at a == b, so the sign of such a zero is the one bit the identity cannot fix."""
import ctypes as C

import numpy as np
import pytest

from hyperpose_amd import engine as E
from hyperpose_amd import frontend, synth
from hyperpose_amd._lib import HP_ERR_CAPACITY, HP_ERR_INVALID, HP_ERR_STATE, DevBuf, HpError

pytestmark = pytest.mark.gpu

NET_W, NET_H, MAX_BATCH = 88, 56, 4
# (dtype, captured graphs, hp_engine_set_concurrency)
VARIANTS = [("f16", True, 1), ("f32", True, 1), ("i8", True, 1), ("f32", False, 1), ("f32", True, 2), ("f32", False, 2)]


@pytest.fixture(scope="module")
def net(hp):
    m = E.Model("lw_openpose_vggtiny", NET_W, NET_H)
    return m, m.init_weights(5)


@pytest.fixture(scope="module")
def frames(hp):
    x = synth.images_u8(synth.rng_for(1, salt=71), 2, NET_H, NET_W)
    return x, frontend.hflip_u8c3_host(x)


def _engine(net, dtype, graph=True, parts=1, calib=None):
    m, w = net
    e = E.Engine.from_model(m, w, max_batch=MAX_BATCH, dtype=dtype)
    if dtype == "i8":
        e.calibrate(calib)
    e.set_graph(graph)
    e.set_concurrency(parts)
    assert e.concurrency == parts
    return e


def _tables(e):
    conf_perm, paf_perm, paf_sign = frontend.flip_tables_coco(e.outputs[0][1][0])
    return [(conf_perm, np.ones(conf_perm.size, np.int8)), (paf_perm, paf_sign)]


def _run_device(e, x):
    dev = DevBuf.from_numpy(x)
    e.enqueue_u8(dev, len(x))
    return [e.output_to_host(i, len(x)) for i in range(len(e.outputs))]


def _run_host(e, x):
    per_image = e.inference(x)
    return [np.stack([img[i][1] for img in per_image]) for i in range(len(e.outputs))]


def _canon(a):
    return (a + np.float32(0.0)).tobytes()


@pytest.mark.parametrize("dtype,graph,parts", VARIANTS)
def test_ensemble_equals_host_merge_and_is_equivariant(hp, net, frames, dtype, graph, parts):
    x, fx = frames
    e = _engine(net, dtype, graph, parts, calib=np.concatenate([x, fx]))
    try:
        assert [o[1][0] for o in e.outputs] == [19, 38] and not e.flip_ensemble
        plain = _run_device(e, np.concatenate([x, fx]))  # [x0, x1, flip x0, flip x1], ensemble off
        tabs = _tables(e)
        want = [frontend.flip_merge_host(p, 2, perm, sign)[:2] for p, (perm, sign) in zip(plain, tabs)]
        e.set_flip_ensemble(True)
        assert e.flip_ensemble and e.max_batch == MAX_BATCH and hp.lib().hp_engine_max_batch(e._h) == MAX_BATCH
        for run in (_run_device, _run_host, _run_device):  # (the second device run replays the captured graph)
            got = run(e, x)
            for g, w_ in zip(got, want):
                assert g.shape == w_.shape and g.tobytes() == w_.tobytes(), f"{run.__name__}: ensemble != host merge of the plain outputs"
        assert any(w_.tobytes() != p[:2].tobytes() for w_, p in zip(want, plain)), "the merge changed nothing: the frames are too tame"
        one = _run_device(e, x[:1])  # another batch size: frame 0 alone
        for g, w_ in zip(one, want):
            assert g.tobytes() == w_[:1].tobytes()
        # equivariance: E(flip x)[perm c](W-1-p) * sign c == E(x)[c](p)
        flipped = _run_device(e, fx)
        for g, w_, (perm, sign) in zip(flipped, want, tabs):
            mapped = (g[:, perm] * sign[None, :, None, None].astype(np.float32))[..., ::-1]
            plus = sign > 0  # a + b == b + a: the kept channels (all of conf, the PAF y channels) in every bit, zeros included
            assert np.ascontiguousarray(mapped[:, plus]).tobytes() == np.ascontiguousarray(w_[:, plus]).tobytes()
            assert _canon(mapped[:, ~plus]) == _canon(w_[:, ~plus])  # the negated channels: in every bit but the sign of a zero
        # an explicit table list is the COCO form
        e.set_flip_ensemble(True, [(1, *tabs[1]), (0, *tabs[0])])
        for g, w_ in zip(_run_device(e, x), want):
            assert g.tobytes() == w_.tobytes()
        if dtype == "i8":  # calibration runs the plain schedule whatever the setting
            before = e.int8_scales.copy()
            e.calibrate(np.concatenate([x, fx]))
            assert e.flip_ensemble and np.array_equal(e.int8_scales, before)
        # the rules while on
        with pytest.raises(HpError) as ex:
            _run_device(e, np.concatenate([x, fx[:1]]))
        assert ex.value.code == HP_ERR_CAPACITY and "3" in str(ex.value) and str(MAX_BATCH) in str(ex.value)
        with pytest.raises(HpError) as ex:
            e.inference_f32(np.zeros((1, 3, NET_H, NET_W), np.float32))
        assert ex.value.code == HP_ERR_STATE and "flip ensemble" in str(ex.value)
        # off again: the plain engine, and a fresh engine's outputs
        e.set_flip_ensemble(False)
        assert not e.flip_ensemble
        again = _run_device(e, np.concatenate([x, fx]))
        fresh = _engine(net, dtype, graph, parts, calib=np.concatenate([x, fx]))
        try:
            for a, p, f in zip(again, plain, _run_device(fresh, np.concatenate([x, fx]))):
                assert a.tobytes() == p.tobytes() == f.tobytes()
        finally:
            fresh.close()
    finally:
        e.close()


def test_setter_refusals(hp, net):
    e = _engine(net, "f16")
    try:
        tabs = _tables(e)
        for what, listing in [("twice", [(0, *tabs[0]), (0, *tabs[0])]), ("every output", [(1, *tabs[1])]), ("names output 2", [(0, *tabs[0]), (2, *tabs[1])]),
                              ("perm[3] = 38", [(0, *tabs[0]), (1, np.where(np.arange(38) == 3, 38, tabs[1][0]).astype(np.int32), tabs[1][1])]),
                              ("sign[5] = 0", [(0, *tabs[0]), (1, tabs[1][0], np.where(np.arange(38) == 5, 0, tabs[1][1]).astype(np.int8))])]:
            with pytest.raises(HpError) as ex:
                e.set_flip_ensemble(True, listing)
            assert ex.value.code == HP_ERR_INVALID and what in str(ex.value), str(ex.value)
            assert not e.flip_ensemble
    finally:
        e.close()


def test_coco_form_refuses_a_pose_proposal_network(hp):
    m = E.Model("pose_proposal_resnet50", 96, 96)
    e = E.Engine.from_model(m, m.init_weights(3), max_batch=2, dtype="f16")
    try:
        with pytest.raises(HpError) as ex:
            e.set_flip_ensemble(True)
        assert ex.value.code == HP_ERR_INVALID and "7" in str(ex.value) and not e.flip_ensemble
    finally:
        e.close()
