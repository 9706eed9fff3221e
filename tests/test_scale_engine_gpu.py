"""GPU: the engine's scale ensemble (hp_engine_set_scale_ensemble*) on lw_openpose_vggtiny at 88 x 56 (maps 11 x 7, cells of 8 x 8 pixels), max_batch 8,
in every arithmetic and launch form of the flip ensemble's tests: the merged outputs are hp_scale_merge_host of the plain engine's outputs on
[frames, host-staged slots], bit for bit - through the device call, the host call, a replayed graph and another batch size; the identity scale
reproduces the plain maps; with the flip ensemble as well the outputs are scale_merge_host(flip_merge_host(plain)); the capacity and state rules;
off again the engine is a fresh plain engine and the setter has dropped the captured graphs.

The identity scale (1.0) is compared after adding +0.0f to both sides: the staged slot is a copy and the weights are (0, 1, 0, 0), so every map
value comes back as (a + a) * 0.5f = a exactly, but 0 * p of a negative p is -0 and a + -0 turns a -0 into +0 - the sign of a zero is the one bit
the identity does not keep."""
import numpy as np
import pytest

from hyperpose_amd import engine as E
from hyperpose_amd import frontend, synth
from hyperpose_amd._lib import HP_ERR_CAPACITY, HP_ERR_INVALID, HP_ERR_STATE, DevBuf, HpError

pytestmark = pytest.mark.gpu

NET_W, NET_H, MAP_W, MAP_H, MAX_BATCH = 88, 56, 11, 7, 8
HALF = [0.5]
# (dtype, captured graphs, hp_engine_set_concurrency)
VARIANTS = [("f16", True, 1), ("f32", True, 1), ("i8", True, 1), ("f32", False, 1), ("f32", True, 2), ("f32", False, 2)]


@pytest.fixture(scope="module")
def net(hp):
    m = E.Model("lw_openpose_vggtiny", NET_W, NET_H)
    return m, m.init_weights(5)


@pytest.fixture(scope="module")
def frames(hp):
    x = synth.images_u8(synth.rng_for(1, salt=73), 2, NET_H, NET_W)
    return x, frontend.scale_stage_host(x, MAP_W, MAP_H, HALF)


def _engine(net, dtype, graph=True, parts=1, calib=None):
    m, w = net
    e = E.Engine.from_model(m, w, max_batch=MAX_BATCH, dtype=dtype)
    if dtype == "i8":
        e.calibrate(calib)
    e.set_graph(graph)
    e.set_concurrency(parts)
    assert e.concurrency == parts
    return e


def _run_device(e, x):
    dev = DevBuf.from_numpy(x)
    e.enqueue_u8(dev, len(x))
    return [e.output_to_host(i, len(x)) for i in range(len(e.outputs))]


def _run_host(e, x):
    per_image = e.inference(x)
    return [np.stack([img[i][1] for img in per_image]) for i in range(len(e.outputs))]


def _canon(a):
    return (a + np.float32(0.0)).tobytes()


def _flip_tables(e):
    conf_perm, paf_perm, paf_sign = frontend.flip_tables_coco(e.outputs[0][1][0])
    return [(conf_perm, np.ones(conf_perm.size, np.int8)), (paf_perm, paf_sign)]


@pytest.mark.parametrize("dtype,graph,parts", VARIANTS)
def test_ensemble_equals_host_merge_of_the_plain_outputs(hp, net, frames, dtype, graph, parts):
    x, sx = frames
    both = np.concatenate([x, sx])
    flipped = frontend.hflip_u8c3_host(both)
    e = _engine(net, dtype, graph, parts, calib=np.concatenate([both, flipped]))
    try:
        assert [o[1] for o in e.outputs] == [(19, MAP_H, MAP_W), (38, MAP_H, MAP_W)] and e.scale_ensemble == 1
        plain = _run_device(e, both)  # [x0, x1, x0 at 0.5, x1 at 0.5], ensemble off
        want = [frontend.scale_merge_host(p, 2, HALF)[:2] for p in plain]
        assert any(w_.tobytes() != p[:2].tobytes() for w_, p in zip(want, plain)), "the merge changed nothing: the frames are too tame"
        if graph:
            assert e.cached_graphs >= 1
        e.set_scale_ensemble(HALF)
        assert e.scale_ensemble == 2 and e.max_batch == MAX_BATCH and e.cached_graphs == 0
        for run in (_run_device, _run_host, _run_device):  # (the second device run replays the captured graph)
            got = run(e, x)
            for g, w_ in zip(got, want):
                assert g.shape == w_.shape and g.tobytes() == w_.tobytes(), f"{run.__name__}: ensemble != host merge of the plain outputs"
        for g, w_ in zip(_run_device(e, x[:1]), want):  # another batch size: frame 0 alone
            assert g.tobytes() == w_[:1].tobytes()
        # the identity scale: the plain maps again, up to the sign of a zero
        e.set_scale_ensemble([1.0])
        for g, p in zip(_run_device(e, x), plain):
            assert _canon(g) == _canon(p[:2])
        # with the flip ensemble as well: 8 images [frames, shrunk, their flips]; the flip merge over 4, then the scale merge over 2
        e.set_scale_ensemble([])
        plain8 = _run_device(e, np.concatenate([both, flipped]))
        e.set_scale_ensemble(HALF)
        e.set_flip_ensemble(True)
        for g, p8, (perm, sign) in zip(_run_device(e, x), plain8, _flip_tables(e)):
            assert g.tobytes() == frontend.scale_merge_host(frontend.flip_merge_host(p8, 4, perm, sign)[:4], 2, HALF)[:2].tobytes()
        with pytest.raises(HpError) as ex:  # 3 frames x 2 scales x 2 = 12 images > 8
            _run_device(e, np.concatenate([x, x[:1]]))
        assert ex.value.code == HP_ERR_CAPACITY and all(s in str(ex.value) for s in ("Yours@3", "K = 2", "flip", "12", f"Max@{MAX_BATCH}")), str(ex.value)
        e.set_flip_ensemble(False)
        if dtype == "i8":  # calibration runs the plain schedule whatever the setting
            before = e.int8_scales.copy()
            e.calibrate(np.concatenate([both, flipped]))
            assert e.scale_ensemble == 2 and np.array_equal(e.int8_scales, before)
        # the rules while on
        with pytest.raises(HpError) as ex:  # 5 frames x 2 scales = 10 images > 8
            _run_device(e, np.concatenate([x, x, x[:1]]))
        assert ex.value.code == HP_ERR_CAPACITY and all(s in str(ex.value) for s in ("Yours@5", "K = 2", "10", f"Max@{MAX_BATCH}")), str(ex.value)
        with pytest.raises(HpError) as ex:
            e.inference_f32(np.zeros((1, 3, NET_H, NET_W), np.float32))
        assert ex.value.code == HP_ERR_STATE and "scale ensemble" in str(ex.value)
        # off again: the plain engine, a fresh engine's outputs, and the setter dropped the captured graphs
        _run_device(e, x)
        if graph:
            assert e.cached_graphs >= 1
        e.set_scale_ensemble([])
        assert e.scale_ensemble == 1 and e.cached_graphs == 0
        again = _run_device(e, both)
        fresh = _engine(net, dtype, graph, parts, calib=np.concatenate([both, flipped]))
        try:
            for a, p, f in zip(again, plain, _run_device(fresh, both)):
                assert a.tobytes() == p.tobytes() == f.tobytes()
        finally:
            fresh.close()
    finally:
        e.close()


def test_fill_colour_and_three_scales(hp, net):
    """The general setter: a fill colour of its own and K = 4, against the host twins on the plain outputs."""
    scales, fill = [0.75, 0.5, 0.3], (9, 200, 77)
    x = synth.images_u8(synth.rng_for(2, salt=73), 2, NET_H, NET_W)
    staged = frontend.scale_stage_host(x, MAP_W, MAP_H, scales, fill)
    e = _engine(net, "f32")
    try:
        plain = _run_device(e, np.concatenate([x, staged]))
        e.set_scale_ensemble(scales, bgcolor=fill)
        assert e.scale_ensemble == 4
        for g, p in zip(_run_device(e, x), plain):
            assert g.tobytes() == frontend.scale_merge_host(p, 2, scales)[:2].tobytes()
        with pytest.raises(HpError) as ex:  # 3 frames x 4 = 12 > 8
            _run_device(e, np.concatenate([x, x[:1]]))
        assert ex.value.code == HP_ERR_CAPACITY and "Yours@3" in str(ex.value) and "12" in str(ex.value)
    finally:
        e.close()


def test_setter_refusals(hp, net):
    e = _engine(net, "f16")
    try:
        for what, args in [("scale 1.5", ([1.5],)), ("scale 0 ", ([0.0],)), ("scale nan", ([float("nan")],)), ("n_scales 4", ([0.5, 0.5, 0.5, 0.5],)),
                           ("fill (0, 256, 0)", ([0.5], (0, 256, 0)))]:
            with pytest.raises(HpError) as ex:
                e.set_scale_ensemble(*args)
            assert ex.value.code == HP_ERR_INVALID and what in str(ex.value), str(ex.value)
            assert e.scale_ensemble == 1
    finally:
        e.close()


def test_coco_form_refuses_a_pose_proposal_network(hp):
    m = E.Model("pose_proposal_resnet50", 96, 96)
    e = E.Engine.from_model(m, m.init_weights(3), max_batch=2, dtype="f16")
    try:
        with pytest.raises(HpError) as ex:
            e.set_scale_ensemble([0.5])
        assert ex.value.code == HP_ERR_INVALID and "hp_engine_set_scale_ensemble_coco" in str(ex.value) and e.scale_ensemble == 1
    finally:
        e.close()
