"""GPU: pixel index -> tensor offsets in the fp32 kernels, bit for bit against numpy on maps where the arithmetic can go wrong.

The fp32 GEMM kernels (conv32_t16_kernel, conv32_kernel in its row and lane = pixel forms, conv32_wk_kernel), the two-layer head and the
depthwise kernel turn a pixel (or thread) index into image, row and column with the layer's division constants (csrc/fastdiv.hpp: multiply-high,
add, shift - no `/`, no carry loop).  What can go wrong there is an offset, so the values are exact as in tests/test_conv32_drain_gpu.py (small
integers: every sum is an fp32 number whatever its order) and EVERY element of a tested tensor is compared bitwise with float64 numpy; halo,
separator rows and channels past Cout must still read zero, and frame 1 alone equals frame 1 of the batch.

Maps, three images each: 1, 3, 15, 16 and 17 pixels wide; OH * OW = 5, 21, 75, 119 are no multiple of 16 - image AND row change inside one
16-pixel MFMA tile, several times inside a t16 wavefront's five tiles on the narrow ones; 15, 63, 225, 240, 357 pixels end inside a tile of 64 and
of 160, and 3 x 7 x 17 is more than one block of either.  Per GEMM kernel: Cout 64 (quad path) and 19 (scalar path) x residual none | before |
after the activation x whole tensors | a slice at channel 3 of a wider buffer with a residual wider than Cout.
Depthwise: stride 1 | 2 and dilation 2 on odd widths, C = 32 and 512, one column per thread and column pairs.
"""
import numpy as np
import pytest

import footprint
from hyperpose_amd import engine as E
from test_conv32_drain_gpu import ExactNet, _bits, _expected, _run_case
from test_engine_footprint_gpu import _set_env, guarded, halo
from test_engine_gpu import Out

pytestmark = pytest.mark.gpu

MAPS = {"5x1": (3, 5, 1), "7x3": (3, 7, 3), "5x15": (3, 5, 15), "5x16": (3, 5, 16), "7x17": (3, 7, 17)}
# kernel: (environment, tile code of every tested layer, Cin)
KERNELS = {
    "t16-64x160": (dict(HP_C32_BN160="1", HP_C32_WK="0", HP_NO_ARENA="1"), 32064160, 16),
    "rows-64x64": (dict(HP_C32_WK="0", HP_NO_ARENA="1"), 32464064, 16),
    "lane-64x64": (dict(HP_C32_WK="0", HP_LANE_EPILOGUE="1", HP_NO_ARENA="1"), 32064064, 16),
    "whole-k-32": (dict(HP_C32_WK="1", HP_NO_ARENA="1"), 39032064, 32),
}


@pytest.mark.parametrize("size", list(MAPS))
@pytest.mark.parametrize("kernel", list(KERNELS))
@guarded
def test_gemm_kernels_place_every_pixel(hp, monkeypatch, kernel, size):
    env, code, cin = KERNELS[kernel]
    n, h, w = MAPS[size]
    _run_case(monkeypatch, env, code, n, h, w, cin, (64, 19))


def _same(size, k, stride, dil):
    out = -(-size // stride)
    total = max((out - 1) * stride + (k - 1) * dil + 1 - size, 0)
    return out, total // 2


def _expected_dw(L, blob, x):
    """Depthwise 3 x 3 layer L (TF SAME) on x [n, c, h, w] in float64: taps, + bias, activation."""
    n, c, h, w = x.shape
    oh, pt = _same(h, 3, L.stride, L.dil)
    ow, pl = _same(w, 3, L.stride, L.dil)
    wt = blob[L.w_off:L.w_off + c * 9].astype(np.float64).reshape(c, 3, 3)
    span = 2 * L.dil + 1
    xp = np.zeros((n, c, (oh - 1) * L.stride + span + pt, (ow - 1) * L.stride + span + pl))
    xp[:, :, pt:pt + h, pl:pl + w] = x
    v = np.zeros((n, c, oh, ow))
    for ky in range(3):
        for kx in range(3):
            y0, x0 = ky * L.dil, kx * L.dil
            v += wt[None, :, ky, kx, None, None] * xp[:, :, y0:y0 + (oh - 1) * L.stride + 1:L.stride, x0:x0 + (ow - 1) * L.stride + 1:L.stride]
    v = v + blob[L.b_off:L.b_off + c].astype(np.float64)[None, :, None, None]
    v = np.minimum(np.maximum(v, 0.0), 6.0) if L.act == E.ACT_RELU6 else np.where(v > 0, v, v * float(L.act_param))
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


@pytest.mark.parametrize("px", ["1", "2"])
@pytest.mark.parametrize("c,h,w", [(32, 9, 7), (512, 5, 3), (32, 35, 13)])
@guarded
def test_depthwise_threads_find_their_columns(hp, monkeypatch, c, h, w, px):
    """dwconv32_kernel<S, D, PX>: stride 1 | 2 and dilation 1 | 2 on odd widths (a ragged last column group, a pair's second column beyond the
    map), 4- and 8-row segments (OH = 35: run = 8, a ragged last segment), three images."""
    _set_env(monkeypatch, dict(HP_DW32_PX=px, HP_NO_FUSE32="1", HP_NO_ARENA="1"))
    n = 3
    net = ExactNet(5 + c)
    t0 = net.conv(0, 3, c, 3, 1, act=E.ACT_RELU6)
    tested = []
    for stride, dil, act in ((1, 1, E.ACT_RELU6), (2, 1, E.ACT_LEAKY), (1, 2, E.ACT_LEAKY)):
        t = net.conv(t0, c, c, 3, stride, dil, op=E.OP_DWCONV, act=act, act_param=0.25)
        tested.append((len(net.layers) - 1, t))
    outs = []
    for i, (_, t) in enumerate(tested):
        y, cy = halo(net, t, c)
        outs.append(Out(f"y{i}", y, 0, cy))
    blob = net.blob()
    eng = E.Engine(net.layers, [o.c() for o in outs], blob, w, h, n, factor=1.0, dtype="f32")
    frames = np.random.default_rng(h * 100 + w).integers(0, 4, (n, h, w, 3), dtype=np.uint8)
    eng.inference(frames)
    footprint.assert_zero_outside(eng, footprint.tensor_ids(net.layers), n, f"dw {c} {h}x{w}")
    x = eng.debug_tensor(t0, n).astype(np.float64)
    assert x.shape == (n, c, h, w) and x.min() >= 0 and x.max() <= 6 and np.array_equal(x, np.round(x))
    rows = {r["layer"]: r for r in eng.profile(n, 1)}
    for li, t in tested:
        assert rows[li]["op"] == E.OP_DWCONV and rows[li]["tile"] == 0, rows[li]   # (its own launch, not fused into the consumer)
        want, mine = _expected_dw(net.layers[li], blob, x), eng.debug_tensor(t, n)
        bad = _bits(mine) != _bits(want)
        assert not bad.any(), (li, int(bad.sum()), [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:6]], mine[bad][:6], want[bad][:6])
    eng.close()


@pytest.mark.parametrize("size", ["7x3", "7x17"])
@guarded
def test_two_layer_heads_place_every_pixel(hp, monkeypatch, size):
    """conv32_head_kernel / conv32_head_pair_kernel (1 x 1 128 -> 128 ReLU6 -> 1 x 1 128 -> 19 | 38): the NHWC slices of a concat buffer and the
    fp32 NCHW network output of a third head, 32-pixel tiles across image and row boundaries."""
    _set_env(monkeypatch, dict(HP_NO_ARENA="1"))
    n, h, w = MAPS[size]
    net = ExactNet(17)
    t0 = net.conv(0, 3, 128, 3, 1, act=E.ACT_RELU6)
    cat = net.new_tensor()
    net.conv(t0, 128, 3, 1, out=cat, out_coff=0, act=E.ACT_NONE)
    heads = []
    for cout, coff in ((19, 3), (38, 22)):
        a = net.conv(t0, 128, 128, 1, act=E.ACT_RELU6)
        net.conv(a, 128, cout, 1, out=cat, out_coff=coff, act=E.ACT_NONE)
        heads.append((len(net.layers) - 2, len(net.layers) - 1, coff))
    a = net.conv(t0, 128, 128, 1, act=E.ACT_RELU6)
    y = net.conv(a, 128, 19, 1, act=E.ACT_LEAKY, act_param=0.25)
    top = (len(net.layers) - 2, len(net.layers) - 1)
    z, cz = halo(net, cat, 60)
    blob = net.blob()
    eng = E.Engine(net.layers, [Out("y", y, 0, 19).c(), Out("z", z, 0, cz).c()], blob, w, h, n, factor=1.0, dtype="f32")
    frames = np.random.default_rng(h * 100 + w).integers(0, 4, (n, h, w, 3), dtype=np.uint8)
    got = eng.inference(frames)
    footprint.assert_zero_outside(eng, footprint.tensor_ids(net.layers), n, f"head32 {h}x{w}")
    assert sum(37000000 <= r["tile"] < 38000000 for r in eng.profile(n, 1)) == 3   # (a row per head; the first two share a grid when they run)
    x = eng.debug_tensor(t0, n).astype(np.float64)
    assert x.shape == (n, 128, h, w) and x.min() >= 0 and x.max() <= 6 and np.array_equal(x, np.round(x))

    def two(la, lb):
        return _expected(net.layers[lb], blob, _expected(net.layers[la], blob, x, None).astype(np.float64), None)
    whole = eng.debug_tensor(cat, n)
    for la, lb, coff in heads:
        want = two(la, lb)
        mine = whole[:, coff:coff + want.shape[1]]
        bad = _bits(mine) != _bits(want)
        assert not bad.any(), (coff, int(bad.sum()), [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:6]])
    want = two(*top)
    for b in range(n):
        mine = dict(got[b])["y"]
        assert np.array_equal(_bits(mine.reshape(want[b].shape)), _bits(want[b])), ("NCHW output", b)
    eng.close()
