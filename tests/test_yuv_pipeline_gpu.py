"""GPU: Pipeline.submit_yuv against Pipeline.submit of the same frames converted on the CPU (tests/yuv_ref.py).  The network inputs are
byte-equal (tests/test_yuv_resize_gpu.py), so the humans must be bit-identical: no tolerance anywhere in this file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref  # noqa: E402

from hyperpose_amd import synth  # noqa: E402
from hyperpose_amd.engine import Model  # noqa: E402
from hyperpose_amd.pipeline import Pipeline  # noqa: E402

pytestmark = pytest.mark.gpu

# the network size of tests/test_pipeline_gpu.py: on its 20 x 16 feature map a part has at most 80 maxima, so the loose thresholds below cannot
# overflow the parser's candidate lists (8 388 per limb) whatever the random-weight maps look like
NET_W, NET_H = 160, 128


def _frames(n, w, h, fmt, seed):
    """n seeded YUV frames (uniform-noise BGR pictures through the input generator) + their CPU-converted BGR."""
    yuv = synth.bgr_to_yuv420(synth.images_u8(synth.rng_for(1, salt=seed), n, h, w), fmt)
    return [f for f in yuv], [yuv_ref.to_bgr(f, fmt) for f in yuv]


def _same(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert fa.tobytes() == fb.tobytes()


@pytest.fixture(scope="module")
def lw(hp):
    from hyperpose_amd import engine as E
    m = Model("lw_openpose_mobilenet", NET_W, NET_H)
    w = m.init_weights(11)
    for L in m.layers:  # blow up the two output convolutions: random weights then give O(1) maps, peaks, limbs and humans (tests/test_pipeline_gpu.py)
        if L.op == E.OP_CONV and L.cout in (19, 38) and L.out in [o.tensor for o in m.outputs]:
            w[L.w_off:L.w_off + L.cout * L.cin] *= 400.0
    return m, w


@pytest.mark.parametrize("keep_ratio", [False, True])
@pytest.mark.parametrize("w,h", [(1280, 720), (NET_W, NET_H)])
def test_submit_yuv_equals_submit_of_converted_frames(lw, w, h, keep_ratio):
    m, weights = lw
    pl = Pipeline(m, weights, max_batch=8, n_pipes=2, keep_ratio=keep_ratio, dtype="f32", conf_thresh=0.05, paf_thresh=-1e9, max_frame_wh=(1280, 720))
    try:
        for fmt in ("nv12", "i420"):
            yuv, bgr = _frames(8, w, h, fmt, seed=3 + keep_ratio)
            pl.submit_yuv(yuv, fmt)
            got = pl.collect()
            pl.submit(bgr)
            want = pl.collect()
            assert len(got) == 8
            print(f"{fmt} {w}x{h} keep_ratio={keep_ratio}: {sum(len(f) for f in want)} humans")
            _same(got, want)
            assert sum(len(f) for f in want) > 0  # the comparison is not vacuous
    finally:
        pl.close()


def test_submit_yuv_pose_proposal_parser(hp):
    """The shared tail of the two submits with another parser behind it."""
    m = Model("pose_proposal_resnet50", 192, 192)
    weights = m.init_weights(5)
    pl = Pipeline(m, weights, max_batch=8, n_pipes=2, keep_ratio=True, dtype="f32", parser="ppn", thresholds=(0.02, 0.01, 0.3), max_frame_wh=(1280, 720))
    try:
        yuv, bgr = _frames(8, 640, 480, "nv12", seed=11)
        pl.submit_yuv(yuv, "nv12")
        got = pl.collect()
        pl.submit(bgr)
        _same(got, pl.collect())
    finally:
        pl.close()


def test_mixed_bgr_and_yuv_submits_collect_in_submission_order(lw):
    m, weights = lw
    pl = Pipeline(m, weights, max_batch=8, n_pipes=4, keep_ratio=False, dtype="f32", conf_thresh=0.05, paf_thresh=-1e9, max_frame_wh=(1280, 720))
    try:
        batches = []
        for k, (kind, n, w, h) in enumerate([("nv12", 8, 1280, 720), ("bgr", 5, 640, 480), ("i420", 3, NET_W, NET_H), ("bgr", 8, 1280, 720),
                                              ("nv12", 1, 640, 480), ("i420", 8, 1280, 720), ("bgr", 2, NET_W, NET_H), ("nv12", 6, 320, 256)]):
            yuv, bgr = _frames(n, w, h, kind if kind != "bgr" else "nv12", seed=20 + k)
            batches.append((kind, yuv, bgr))
        # what each batch gives by itself, one at a time
        alone = []
        for kind, yuv, bgr in batches:
            pl.submit(bgr)
            alone.append(pl.collect())
        # the same batches, four in flight, BGR and YUV submits alternating
        got = []
        for start in (0, 4):
            for kind, yuv, bgr in batches[start:start + 4]:
                pl.submit(bgr) if kind == "bgr" else pl.submit_yuv(yuv, kind)
            assert pl.in_flight == 4
            got += [pl.collect() for _ in range(4)]
        assert [len(g) for g in got] == [len(b[1]) for b in batches]
        for g, a in zip(got, alone):
            _same(g, a)
        assert sum(len(f) for a in alone for f in a) > 0
    finally:
        pl.close()


def test_submit_yuv_refuses_bad_frames(lw):
    m, weights = lw
    from hyperpose_amd._lib import HpError, HP_ERR_CAPACITY, HP_ERR_INVALID
    pl = Pipeline(m, weights, max_batch=2, n_pipes=1, dtype="f32", max_frame_wh=(640, 480))
    try:
        with pytest.raises(HpError) as e:
            pl.submit_yuv([np.zeros((9, 5), np.uint8)])  # 5 x 6: odd width
        assert e.value.code == HP_ERR_INVALID
        with pytest.raises(HpError) as e:
            pl.submit_yuv([np.zeros((1080 * 3 // 2, 1920), np.uint8)])  # 3.1 MB > max_frame_bytes of 640 x 480 x 3
        assert e.value.code == HP_ERR_CAPACITY
        with pytest.raises(HpError) as e:
            pl.submit_yuv([np.zeros((72, 64), np.uint8)] * 3)  # batch 3 > max_batch 2
        assert e.value.code == HP_ERR_CAPACITY
        assert pl.in_flight == 0
        pl.submit_yuv([np.zeros((72, 64), np.uint8)], "i420")
        assert len(pl.collect()) == 1
    finally:
        pl.close()
