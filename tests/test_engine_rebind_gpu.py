"""GPU: running a batch leaves the engine's schedule alone.  Every launch binds a copy of its step's parameters to the frames of the call
(engine.cpp: bind / hp_engine::bound); nothing a call was bound to - its batch size, its frame offset, its input pointer - may stay behind in
the schedule.  So after calls on 3, 1, 2 and again 3 frames, eager and profiled, an engine must return the bits it returned the first time
and report the profile rows of an engine that never ran anything else.  max_batch = 3: with hp_engine_set_concurrency(2) the batch runs
as half-batches of 2 + 1 frames.  Run with captured graphs off (every call goes through hp_engine::run_step), then once more with them on.
"""
import functools

import numpy as np
import pytest

from hyperpose_amd import engine as E
from hyperpose_amd import synth

ARCHS = ["lw_openpose_mobilenet", "lw_openpose_vggtiny", "openpose_vgg19", "pose_proposal_resnet50", "pifpaf_resnet50"]
# (id, dtype, HP_NO_FUSE, concurrency)
ENGINES = [("f16", "f16", False, 1), ("f16-nofuse", "f16", True, 1), ("f32-c1", "f32", False, 1), ("f32-c2", "f32", False, 2),
           ("f32s", "f32s", False, 1), ("i8", "i8", False, 1)]
BATCH = 3


@functools.lru_cache(maxsize=None)
def _model(arch):
    # the small sizes of test_builtin_topologies_small / test_lw_openpose_small_end_to_end
    w, h = (97, 97) if arch.startswith("pifpaf") else (160, 128) if arch.startswith("pose_proposal") else (96, 80)
    m = E.Model(arch, w, h)
    return m, m.init_weights(3), synth.images_u8(synth.rng_for(8), BATCH, h, w)


def _engine(arch, dtype, parts):
    m, w, _ = _model(arch)
    eng = E.Engine.from_model(m, w, max_batch=BATCH, dtype=dtype)
    if dtype == "i8":
        eng.int8_scales = np.where(eng.int8_scales != 0, 1.0, 0.0).astype(np.float32)
    eng.set_concurrency(parts)
    return eng


def _rows(eng):
    return [(s["layer"], s["op"], s["tile"], s["flops"], s["bytes"]) for s in eng.profile(BATCH, iters=1)]


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("name,dtype,no_fuse,parts", ENGINES, ids=[e[0] for e in ENGINES])
def test_calls_on_other_batches_leave_no_trace(hp, monkeypatch, name, dtype, no_fuse, parts, arch):
    if no_fuse:
        monkeypatch.setenv("HP_NO_FUSE", "1")
    frames = _model(arch)[2]
    twin = _engine(arch, dtype, parts)
    fresh = _rows(twin)
    twin.close()
    eng = _engine(arch, dtype, parts)
    assert eng.concurrency == (parts if dtype in ("f32", "f32s") else 1)
    for graphs in (False, True):
        eng.set_graph(graphs)
        first = eng.inference(frames)
        eng.profile(1, iters=1)
        eng.inference(frames[:1])
        eng.profile(2, iters=1, in_sequence=True)
        again = eng.inference(frames)
        for b in range(BATCH):
            for (nm, x), (_, y) in zip(first[b], again[b]):
                assert np.array_equal(x, y), f"graphs {graphs}: output {nm} of frame {b} changed after calls on 1 and 2 frames"
        assert _rows(eng) == fresh, f"graphs {graphs}: profile({BATCH}) differs from a fresh engine's"
    eng.close()
