"""GPU: the engines' arithmetic at the edges of its number range.  Every other engine test draws He-scaled weights and frames / 255 and gates on
max|got - ref| <= 1e-4 max|ref| over a tensor: an error confined to small operands or to low-magnitude channels passes.  Here

  1. the split engine's product (HP_DTYPE_F32S, csrc/conv32_direct.hip), one tap per output channel, operands with full 24-bit significands in
     four exponent windows from 2^-30 to 65504 and two mixed runs, element by element against tests/split_ref.py's layer_bound;
  2. its sums with positive, aligned remainders (a lost cross term adds up instead of cancelling): dense 1 x 1, dense 3 x 3, and the fused
     depthwise form, which splits a COMPUTED value on a second code path;
  3. the 65504 threshold: activations and weights exactly at it keep the fp16 pipe, 65505 / 65536 leave it;
  4. the fp32 engine (HP_DTYPE_F32): scaling a layer by powers of two scales its outputs bit for bit, in every kernel family.

All bounds are derived (split_ref.py) or exact; tests/test_split_contract_cpu.py shows on these very inputs that a dropped cross term, a dropped
lo, flushed fp16 subnormals or a wrong 2^-11 leave the bound on most outputs.  The layer's real input is read back (debug_tensor), so the
reference does not rest on the layer in front.
"""
import numpy as np
import pytest

import split_ref as S
from hyperpose_amd import engine as E
from test_engine_footprint_gpu import _set_env, guarded
from test_engine_gpu import Net, Out

pytestmark = pytest.mark.gpu

N, H, W = S.N, S.H, S.W


def _put(blob, L, w=None, b=None):
    if w is not None:
        w = np.asarray(w, np.float32).ravel()
        blob[L.w_off:L.w_off + w.size] = w
    if b is not None:
        blob[L.b_off:L.b_off + L.cout] = np.asarray(b, np.float32)


def _split_graph(des, out_act=E.ACT_NONE, consumer=False, bias=None):
    """first layer (1 x 1, 3 -> cin, power-of-two weights, no bias) [-> depthwise 3 x 3, RELU6] -> the layer under test [-> a 1 x 1 stride-2 reader].
    Without a reader the layer is a network output (the lane = pixel epilogue and its fused fp32 copy); with one it stores NHWC rows."""
    net = Net(0)
    t0 = net.conv(0, 3, des.cin, 1, 1, act=E.ACT_NONE)
    src = t0
    if getattr(des, "dw", False):
        src = net.conv(t0, des.cin, des.cin, 3, 1, 1, op=E.OP_DWCONV, act=E.ACT_RELU6)
    t = net.conv(src, des.cin, des.cout, des.k, act=out_act)
    # (the reader has stride 2: no split layer itself, so outputs beyond 65504 - the top window's products - raise no flag there)
    z = net.conv(t, des.cout, 8, 1, 2, act=E.ACT_NONE) if consumer else None
    blob = net.blob()
    blob[:] = 0
    _put(blob, net.layers[0], des.w_first)
    if getattr(des, "dw", False):
        _put(blob, net.layers[1], des.dw_w, des.dw_b)
    _put(blob, net.layers[-2 if consumer else -1], des.w, bias)
    if consumer:
        _put(blob, net.layers[-1], np.full(8 * des.cout, 2.0 ** -6))
    net.w = [blob]
    outs = [Out("z", z, 0, 8)] if consumer else [Out("y", t, 0, des.cout)]
    return net, t0, t, outs


def _tile_of(eng, *layers):
    """The tile codes of the profile rows of these layers (a fused pair has ONE row, under one of its two layers)."""
    return [r["tile"] for r in eng.profile(N, 1) if r["layer"] in layers]


def _within(got, A, Wt, bias, what):
    ref, bound = S.as_nchw(S.exact(A, Wt, bias), N, H, W), S.as_nchw(S.layer_bound(A, Wt, bias), N, H, W)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: worst |got - ref| / layer_bound = {worst:.4f}, elements beyond it {int((err > bound).sum())} of {err.size}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} of {err.size} elements beyond layer_bound, worst ratio {worst:.4g}"


# ---------------------------------------------------------------- 1. one tap per output channel
@pytest.mark.parametrize("act_win,w_win", S.RUNS, ids=[f"{a}-{w}" for a, w in S.RUNS])
@pytest.mark.parametrize("cin,cout,k", S.SHAPES, ids=[f"{a}-{b}-{k}x{k}" for a, b, k in S.SHAPES])
@guarded
def test_split_product_one_tap_per_channel(hp, monkeypatch, cin, cout, k, act_win, w_win):
    _set_env(monkeypatch, {})
    des = S.OneTap(cin, cout, k, act_win, w_win)
    rows = cout == 512      # this shape stores NHWC rows for a reader (conv32_store_rows); the other two are network outputs (lane = pixel epilogue)
    net, t0, t, outs = _split_graph(des, consumer=rows)
    eng = E.Engine(net.layers, [o.c() for o in outs], net.blob(), W, H, N, dtype="f32s")
    assert eng.split_fallbacks == 0
    got = eng.inference_f32(des.frames)
    got = eng.debug_tensor(t, N) if rows else np.stack([dict(g)["y"] for g in got])
    assert eng.split_fallbacks == 0
    x = eng.debug_tensor(t0, N)
    assert np.array_equal(x, des.act), "the first layer's power-of-two products are not exact"
    _within(got, S.patches(x, k), des.Wt, None, f"{cin}->{cout} {k}x{k} {act_win} x {w_win}")
    assert [tl // 1000 for tl in _tile_of(eng, 1)] == [33000 + k]
    eng.close()


# ---------------------------------------------------------------- 2. sums with aligned remainders
SUMS = [(64, 128, 1, False, 33001), (32, 64, 3, False, 33003), (64, 128, 1, True, 33101)]


@pytest.mark.parametrize("cin,cout,k,dw,code", SUMS, ids=["1x1-64", "3x3-32", "dw-1x1-64"])
@guarded
def test_split_sums_with_aligned_remainders(hp, monkeypatch, cin, cout, k, dw, code):
    _set_env(monkeypatch, {})
    des = S.Aligned(cin, cout, k, dw)
    net, t0, t, outs = _split_graph(des, out_act=E.ACT_RELU if dw else E.ACT_NONE, consumer=True, bias=des.bias)   # (RELU: g_sep32's graph; every sum is positive)
    eng = E.Engine(net.layers, [o.c() for o in outs], net.blob(), W, H, N, dtype="f32s")
    eng.inference_f32(des.frames)
    assert eng.split_fallbacks == 0
    x = eng.debug_tensor(t0, N)
    assert np.array_equal(x, des.act)
    if dw:
        x = des.depthwise(x)      # the depthwise result lives only inside the launch: float32, the kernel's own fmaf order
    got = eng.debug_tensor(t, N)
    _within(got, S.patches(x, k), des.Wt, des.bias, f"sum {cin}->{cout} {k}x{k}{' behind a depthwise layer' if dw else ''}")
    li = len(net.layers) - 2
    assert [tl // 1000 for tl in (_tile_of(eng, li - 1, li) if dw else _tile_of(eng, li))] == [code]
    eng.close()


# ---------------------------------------------------------------- 3. the 65504 threshold
class _Edge:
    """64 -> 19, 1 x 1 (after a fall-back the split engine and an HP_DTYPE_F32 engine both run conv32_direct_kernel's fp32 form on it: 34001).
    Dense weights with full significands in 2^-6 .. 2^2; activation c = plane c % 3 times 2^e_c."""

    def __init__(self, e_act, frames, seed=0):
        rng = np.random.default_rng([11, seed])
        self.cin, self.cout, self.k = 64, 19, 1
        self.frames = frames
        self.w_first = np.zeros((64, 3), np.float32)
        self.w_first[np.arange(64), np.arange(64) % 3] = np.float32(2.0) ** e_act
        self.act = frames[:, np.arange(64) % 3] * (np.float32(2.0) ** e_act)[None, :, None, None]
        self.w = np.ldexp(S.significands(rng, (19, 1, 1, 64)).astype(np.float64), rng.integers(-6, 3, (19, 1, 1, 64))).astype(np.float32)
        self.Wt = self.w.reshape(19, -1).T.copy()


def _engine(des, dtype):
    net, t0, t, outs = _split_graph(des)
    return net, t0, E.Engine(net.layers, [o.c() for o in outs], net.blob(), W, H, N, dtype=dtype)


@guarded
def test_activations_of_exactly_65504_stay_on_the_fp16_pipe(hp, monkeypatch):
    _set_env(monkeypatch, {})
    rng = np.random.default_rng(12)
    frames = (np.float32(S.F16_MAX / 2 ** 15) * rng.choice(np.float32([-1, 1]), (N, 3, H, W))).astype(np.float32)
    des = _Edge(np.full(64, 15), frames)
    assert (np.abs(des.act) == S.F16_MAX).all()
    net, t0, eng = _engine(des, "f32s")
    got = np.stack([dict(g)["y"] for g in eng.inference_f32(frames)])
    assert eng.split_fallbacks == 0
    x = eng.debug_tensor(t0, N)
    assert np.array_equal(x, des.act)
    _within(got, S.patches(x, 1), des.Wt, None, "activations +-65504")
    assert [tl // 1000 for tl in _tile_of(eng, 1)] == [33001]
    eng.close()


@guarded
def test_one_activation_of_65505_leaves_the_fp16_pipe(hp, monkeypatch):
    """65505 is the first float32 integer beyond fp16's range (it would still round to 65504).  ONE activation holds it: channel 0 (2^15, the only
    channel of plane 0 above 2^13) at one pixel.  The engine falls back once and returns the bytes of an HP_DTYPE_F32 engine of the same layers."""
    _set_env(monkeypatch, {})
    rng = np.random.default_rng(13)
    frames = np.clip(S.significands(rng, (N, 3, H, W)), -1.99, 1.99).astype(np.float32)
    e_act = rng.integers(-6, 14, 64)
    e_act[0] = 15
    frames[1, 0, 9, 10] = np.float32(65505.0 / 2 ** 15)
    des = _Edge(e_act, frames)
    assert int((np.abs(des.act) > S.F16_MAX).sum()) == 1 and des.act[1, 0, 9, 10] == 65505
    net, t0, eng = _engine(des, "f32s")
    got = np.stack([dict(g)["y"] for g in eng.inference_f32(frames)])
    assert eng.split_fallbacks == 1
    assert np.array_equal(eng.debug_tensor(t0, N), des.act)
    _, _, e32 = _engine(des, "f32")
    want = np.stack([dict(g)["y"] for g in e32.inference_f32(frames)])
    assert got.tobytes() == want.tobytes()
    again = np.stack([dict(g)["y"] for g in eng.inference_f32(frames)])
    assert eng.split_fallbacks == 1 and again.tobytes() == want.tobytes()
    tile = _tile_of(e32, 1)
    assert [tl // 1000 for tl in tile] == [34001] and _tile_of(eng, 1) == tile
    # the same frames with 65504 there: no fall-back
    frames[1, 0, 9, 10] = np.float32(S.F16_MAX / 2 ** 15)
    _, _, ok = _engine(_Edge(e_act, frames), "f32s")
    ok.inference_f32(frames)
    assert ok.split_fallbacks == 0
    for e in (eng, e32, ok):
        e.close()


@guarded
def test_weights_at_the_threshold(hp, monkeypatch):
    """A weight of 65504 has a split (hi = 65504, lo = 0) and keeps the fp16 pipe; 65536 has none (hi would be inf): the engine starts on the fp32 pipe."""
    _set_env(monkeypatch, {})
    rng = np.random.default_rng(14)
    frames = S.significands(rng, (N, 3, H, W))
    des = _Edge(rng.integers(-6, 3, 64), frames)
    des.w[3, 0, 0, 17], des.w[11, 0, 0, 40] = S.F16_MAX, -S.F16_MAX
    des.Wt = des.w.reshape(19, -1).T.copy()
    net, t0, eng = _engine(des, "f32s")
    assert eng.split_fallbacks == 0
    got = np.stack([dict(g)["y"] for g in eng.inference_f32(frames)])
    assert eng.split_fallbacks == 0
    _within(got, S.patches(eng.debug_tensor(t0, N), 1), des.Wt, None, "weights +-65504")
    assert [tl // 1000 for tl in _tile_of(eng, 1)] == [33001]
    eng.close()
    des.w[3, 0, 0, 17] = 65536.0
    _, _, big = _engine(des, "f32s")
    assert big.split_fallbacks == 1
    _, _, e32 = _engine(des, "f32")
    a = np.stack([dict(g)["y"] for g in big.inference_f32(frames)])
    b = np.stack([dict(g)["y"] for g in e32.inference_f32(frames)])
    assert big.split_fallbacks == 1 and a.tobytes() == b.tobytes()
    assert [tl // 1000 for tl in _tile_of(big, 1)] == [34001]
    big.close()
    e32.close()


# ---------------------------------------------------------------- 4. fp32 pipe: power-of-two homogeneity
# Every HP_DTYPE_F32 kernel is fmaf or the fp32 MFMA: with weights of output channel c times 2^e_c and input activations times 2^j (biases times
# 2^(e_c + j): a bias adds to a sum that carries both factors) every product, partial sum and rounding is the unscaled one times a power of
# two, so the outputs are the unscaled outputs times 2^(e_c + j), bit for bit - unless a path treats ranges differently.  One case per kernel
# family of test_engine_footprint_gpu.py, with its switches, map size, batch and tile code.  (family: environment, map, graph, tile test.)
HN = 3
is_ = lambda code: (lambda t: t == code)                 # noqa: E731
k_ = lambda code: (lambda t: t // 1000 == code)          # noqa: E731
FAMILIES = {
    "conv32-64x64": (dict(HP_C32_WK="0"), (9, 15), ("dense", 64, 128, 1), is_(32464064)),
    "conv32-64x160": (dict(HP_C32_BN160="1", HP_C32_WK="0"), (9, 15), ("dense", 64, 128, 1), is_(32064160)),
    "conv32-whole-k": (dict(HP_C32_WK="1"), (9, 15), ("dense", 64, 128, 1), k_(39064)),
    "direct-1x1": ({}, (9, 9), ("dense", 128, 38, 1), k_(34001)),
    "direct-3x3": (dict(HP_NO_WINOGRAD32="1"), (9, 9), ("dense", 64, 96, 3), k_(34003)),
    "winograd": ({}, (17, 9), ("dense", 48, 96, 3), is_(35003004)),
    "head": ({}, (9, 15), ("head", 128, 19), is_(37000000 + 12800 + 19)),
    "depthwise-px1": (dict(HP_DW32_PX="1"), (9, 9), ("dw", 32), is_(0)),
    "depthwise-px2": (dict(HP_DW32_PX="2"), (9, 9), ("dw", 32), is_(0)),
    "first": ({}, (17, 33), ("first", 32, 3), is_(0)),
}
ACTS = {"none": E.ACT_NONE, "relu": E.ACT_RELU, "leaky": E.ACT_LEAKY, "prelu": E.ACT_PRELU}
# (the first convolution and the depthwise kernels take no PRELU: the engine refuses such a layer)
HOMOG = [(f, a) for f in FAMILIES for a in ACTS if not (a == "prelu" and (f == "first" or f.startswith("depthwise")))]


def _homog_graph(kind, act):
    """Returns net, the tested tensor, its layer, the tensor in front (or None) and plan(j, e, g): layer -> (row exponents, column exponents, bias
    exponents) for the weights [cout][taps][cin] (depthwise: [c][9])."""
    net = Net(41)
    if kind[0] == "first":
        t = net.conv(0, 3, kind[1], kind[2], 1, act=act, act_param=0.125)
        net.conv(t, kind[1], 8, 1, act=E.ACT_NONE)
        return net, t, 0, None, lambda j, e, g: {0: (e, None, e + j)}
    if kind[0] == "dense":
        _, cin, cout, k = kind
        t0 = net.conv(0, 3, cin, 3, 1)
        t = net.conv(t0, cin, cout, k, act=act, act_param=0.125)
        net.conv(t, cout, 8, 1, act=E.ACT_NONE)
        return net, t, 1, t0, lambda j, e, g: {0: (j, None, j), 1: (e, None, e + j)}
    if kind[0] == "dw":
        c = kind[1]
        t0 = net.conv(0, 3, c, 3, 1)
        t = net.conv(t0, c, c, 3, 1, op=E.OP_DWCONV, act=act, act_param=0.125)
        net.conv(t, c, 8, 1, act=E.ACT_NONE)
        return net, t, 1, t0, lambda j, e, g: {0: (j, None, j), 1: (e, None, e + j)}
    _, hid, cout = kind   # the two-layer head: the hidden layer (in registers) scaled per channel by 2^g, undone in the second layer's columns
    t0 = net.conv(0, 3, 128, 3, 1)
    a = net.conv(t0, 128, hid, 1, act=E.ACT_LEAKY if act == E.ACT_PRELU else act, act_param=0.125)   # (a PRELU hidden layer is not fused)
    t = net.conv(a, hid, cout, 1, act=act, act_param=0.125)
    net.conv(t, cout, 8, 1, act=E.ACT_NONE)
    return net, t, 2, t0, lambda j, e, g: {0: (j, None, j), 1: (g, None, g + j), 2: (e, -g, e + j)}


def _scaled_blob(net, plan):
    blob = net.blob().copy()
    for li, (rows, cols, bexp) in plan.items():
        L = net.layers[li]
        rows_n = L.cin if L.op == E.OP_DWCONV else L.cout
        n = rows_n * L.kh * L.kw * (1 if L.op == E.OP_DWCONV else L.cin)
        w = blob[L.w_off:L.w_off + n].reshape(rows_n, L.kh * L.kw, -1)
        ex = np.broadcast_to(np.asarray(rows), (rows_n,))[:, None, None] + (0 if cols is None else np.asarray(cols)[None, None, :])
        w[:] = np.ldexp(w, ex)
        b = blob[L.b_off:L.b_off + L.cout]
        b[:] = np.ldexp(b, np.broadcast_to(np.asarray(bexp), (L.cout,)))
    return blob


def _in_range(x, what):
    nz = np.abs(x[x != 0])
    assert nz.size and nz.min() >= 2.0 ** -100 and nz.max() <= 2.0 ** 100, f"{what}: magnitudes {nz.min():.3g} .. {nz.max():.3g} leave [2^-100, 2^100]"


@pytest.mark.parametrize("family,act", HOMOG, ids=[f"{f}-{a}" for f, a in HOMOG])
@guarded
def test_fp32_pipe_is_homogeneous_in_powers_of_two(hp, monkeypatch, family, act):
    env, (h, w), kind, want = FAMILIES[family]
    _set_env(monkeypatch, env)
    net, t, li, t0, plan = _homog_graph(kind, ACTS[act])
    cout = net.layers[li].cout
    outs = [Out("z", net.layers[-1].out, 0, 8).c()]
    frames = np.random.default_rng(17).normal(0, 1, (HN, 3, h, w)).astype(np.float32)

    def run(blob, fr):
        eng = E.Engine(net.layers, outs, blob, w, h, HN, dtype="f32")
        eng.inference_f32(fr)
        tested, front = eng.debug_tensor(t, HN), (eng.debug_tensor(t0, HN) if t0 is not None else None)
        tiles = [r["tile"] for r in eng.profile(HN, 1) if r["layer"] == li or (kind[0] == "head" and r["layer"] == li - 1)]   # (a fused pair: ONE row)
        eng.close()
        return tested, front, tiles

    base, base_front, tiles = run(net.blob(), frames)
    assert len(tiles) == 1 and want(tiles[0]), (family, tiles)
    _in_range(base, "unscaled outputs")
    if act != "none":
        assert 0.2 <= float((base < 0).mean() if act != "relu" else (base == 0).mean()) <= 0.8     # both branches of the activation are taken
    rng = np.random.default_rng(19)
    for j in (-20, 12):
        e = rng.integers(-40, 41, cout)
        g = rng.integers(-10, 11, net.layers[1].cout) if kind[0] == "head" else None
        got, front, tiles_j = run(_scaled_blob(net, plan(j, e, g)), np.ldexp(frames, j) if kind[0] == "first" else frames)
        assert tiles_j == tiles
        _in_range(got, f"outputs scaled by 2^({j} + e_c)")
        if front is not None:
            _in_range(front, f"activations scaled by 2^{j}")
            assert np.array_equal(front, np.ldexp(base_front, j)), f"{family}: the layer in front is not homogeneous (2^{j})"
        expect = np.ldexp(base, (e + j)[None, :, None, None])
        diff = got != expect
        assert np.array_equal(got, expect), f"{family} {act}, activations x 2^{j}: {int(diff.sum())} of {diff.size} outputs are not the unscaled ones times 2^(e_c + j)"
