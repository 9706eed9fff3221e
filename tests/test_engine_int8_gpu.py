"""GPU: HP_DTYPE_I8 engines (data_type::kINT8) - the int8 matrix-pipe convolution (csrc/conv_i8.hip) against an exact emulation of
the quantization contract, MinMax calibration, the per-layer scale vector, serialization and whole networks against the fp32 oracle.

Numerics (include/hp_hip.h, HP_DTYPE_I8): s_w[c] = max |w| / 127, q_w = clamp(rint(w / s_w[c]), -127, 127); q_x = clamp(rint(x * (1 / s_a)),
-127, 127) of the stored fp16 input; exact int32 sums; v = (float)acc * (s_a * s_w[c]) + bias[c], then the fp16 engine's epilogue.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import footprint
from hyperpose_amd import _lib
from hyperpose_amd import engine as E
from oracle import ref_net

pytestmark = pytest.mark.gpu


class Out:
    def __init__(self, name, tensor, coff, channels, **kw):
        self.name, self.tensor, self.coff, self.channels, self.act = name.encode(), tensor, coff, channels, 0
        self.shuffle, self.group, self.sigmoid_mask, self.softplus_mask = 0, 0, 0, 0
        self.out_h, self.out_w, self.scale, self.grid = 0, 0, 0.0, 0
        for k, v in kw.items():
            setattr(self, k, v)

    def c(self):
        o = E.OutputDesc()
        for f, _ in E.OutputDesc._fields_:
            setattr(o, f, getattr(self, f))
        return o


class Net:
    def __init__(self, seed=0):
        self.layers, self.w, self.rng, self.nt = [], [], np.random.default_rng(seed), 1

    def _alloc(self, n, std):
        off = sum(len(x) for x in self.w)
        self.w.append((self.rng.normal(0, std, n)).astype(np.float32))
        return off

    def conv(self, in_, cin, cout, k=1, stride=1, dil=1, act=E.ACT_RELU, out=None, out_coff=0, in_coff=0, res=-1, res_before_act=0,
             act_param=0.0):
        if out is None:
            out = self.nt
            self.nt += 1
        w_off = self._alloc(cout * k * k * cin, np.sqrt(2.0 / (k * k * cin)))
        b_off = self._alloc(cout, 0.1)
        a_off = -1
        if act == E.ACT_PRELU:
            a_off = self._alloc(cout, 0.0)
            self.w[-1][:] = self.rng.uniform(0.1, 0.4, cout)
        self.layers.append(E.make_layer(E.OP_CONV, in_, out, cin, cout, k, stride, dil, act, in_coff, out_coff, res, res_before_act,
                                        w_off, b_off, a_off, act_param))
        return out

    def blob(self):
        return np.concatenate(self.w)


def _frames(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _same(size, k, s, d):
    out = (size + s - 1) // s
    total = max((out - 1) * s + (k - 1) * d + 1 - size, 0)
    return total // 2, total - total // 2


def _emulate(L, x, blob, s_a, res=None, return_acc=False):
    """The int8 layer L on fp32 NCHW input x (the stored fp16 values): returns v before the fp16 rounding (fp32); `return_acc`: and the
    exact integer sums (float64)."""
    k, cin, cout = L.kh, L.cin, L.cout
    w = blob[L.w_off:L.w_off + cout * k * k * cin].reshape(cout, k, k, cin).astype(np.float32)
    m = np.abs(w).reshape(cout, -1).max(axis=1)
    s_w = np.where(m > 0, m / np.float32(127), np.float32(1)).astype(np.float32)
    q_w = np.clip(np.rint(w / s_w[:, None, None, None]), -127, 127)
    inv_a = np.float32(1) / np.float32(s_a)
    q_x = np.clip(np.rint(x[:, L.in_coff:L.in_coff + cin].astype(np.float32) * inv_a), -127, 127)
    H, W = x.shape[2], x.shape[3]
    pt, pb = _same(H, k, L.stride, L.dil)
    pl, pr = _same(W, k, L.stride, L.dil)
    xt = F.pad(torch.from_numpy(q_x.astype(np.float64)), (pl, pr, pt, pb))
    acc = F.conv2d(xt, torch.from_numpy(q_w.transpose(0, 3, 1, 2).astype(np.float64)), stride=L.stride, dilation=L.dil).numpy()
    dq = (np.float32(s_a) * s_w).astype(np.float32)
    bias = blob[L.b_off:L.b_off + cout].astype(np.float32)
    v = acc.astype(np.float32) * dq[None, :, None, None] + bias[None, :, None, None]
    r = np.zeros_like(v) if res is None else res[:, :cout].astype(np.float32)
    if L.res_before_act:
        v = v + r
    if L.act == E.ACT_RELU:
        v = np.maximum(v, 0)
    elif L.act == E.ACT_RELU6:
        v = np.minimum(np.maximum(v, 0), 6)
    elif L.act in (E.ACT_LEAKY, E.ACT_PRELU):
        slope = np.float32(L.act_param) if L.act == E.ACT_LEAKY else blob[L.alpha_off:L.alpha_off + cout][None, :, None, None]
        v = np.where(v > 0, v, v * slope)
    if not L.res_before_act:
        v = v + r
    return (v.astype(np.float32), acc) if return_acc else v.astype(np.float32)


def _fp16_gate(got, want16):
    """<= 1 fp16 ulp of the value everywhere, >= 99.9 % bit-identical."""
    got16 = got.astype(np.float16)
    assert np.array_equal(got16.astype(np.float32), got), "stored tensor is not fp16"
    ulp = np.spacing(np.abs(want16)).astype(np.float32)
    diff = np.abs(got16.astype(np.float32) - want16.astype(np.float32))
    assert (diff <= ulp).all(), f"max diff {diff.max():.4g} beyond one fp16 ulp"
    same = float(np.mean(got16.view(np.uint16) == want16.view(np.uint16)))
    assert same >= 0.999, f"only {same:.5f} of the elements bit-identical"


# (cin, cout, k, stride, dil): the shapes of test_engine_gpu.py::test_mfma_conv_shapes whose geometry the int8 kernel covers
SHAPES = [(32, 64, 1, 1, 1), (64, 128, 1, 1, 1), (128, 128, 3, 1, 1), (128, 512, 1, 1, 1), (512, 19, 1, 1, 1), (512, 38, 1, 1, 1),
          (64, 64, 3, 2, 1), (96, 128, 3, 1, 2), (128, 128, 7, 1, 1), (256, 200, 3, 1, 1), (64, 256, 1, 2, 1), (64, 64, 3, 1, 1),
          (128, 64, 3, 1, 1), (256, 512, 1, 2, 1), (512, 256, 1, 1, 1), (256, 1024, 1, 1, 1), (185, 128, 7, 1, 1)]
CASES = [dict(cin=a, cout=b, k=k, stride=s, dil=d) for a, b, k, s, d in SHAPES] + [
    dict(cin=128, cout=128, k=3, res="before"), dict(cin=128, cout=128, k=3, res="after"), dict(cin=64, cout=38, k=1, concat=24),
    dict(cin=64, cout=64, k=1, concat=26), dict(cin=128, cout=128, k=3, concat=26),  # a writer whose channel offset is not 4-aligned
    dict(cin=128, cout=96, k=3, act=E.ACT_PRELU), dict(cin=64, cout=64, k=3, act=E.ACT_LEAKY), dict(cin=64, cout=64, k=1, act=E.ACT_RELU6)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_int8_layer_matches_the_quantization_contract(hp, case):
    cin, cout, k = case["cin"], case["cout"], case["k"]
    stride, dil, act = case.get("stride", 1), case.get("dil", 1), case.get("act", E.ACT_RELU)
    net = Net(cin * 7 + cout + k)
    h, w, n = 23, 29, 3
    t0 = net.conv(0, 3, cin, 3, 1)
    res, rba = -1, 0
    if "res" in case:
        res = net.conv(0, 3, cout, 3, 1)
        rba = 1 if case["res"] == "before" else 0
    out, out_coff = None, 0
    if case.get("concat"):
        out, out_coff = net.nt, case["concat"]
        net.nt += 1
        net.conv(t0, cin, out_coff, 1, out=out)  # channels [0, out_coff) of the concat buffer: an int8-eligible writer too
    t = net.conv(t0, cin, cout, k, stride, dil, act=act, act_param=0.1, out=out, out_coff=out_coff, res=res, res_before_act=rba)
    z = net.conv(t, out_coff + cout, 8, 1)      # a reader: the layer's fp16 tensor is materialised next to its fused fp32 copy
    blob = net.blob()
    # a concat writer's output is read through the conversion kernel (scale 2): the layer then stores through the vector epilogue
    fused = not case.get("concat")
    outs = [Out("y", t, out_coff, cout, **({} if fused else dict(scale=2.0))), Out("z", z, 0, 8)]
    eng = E.Engine(net.layers, [o.c() for o in outs], blob, w, h, n, dtype="i8")
    L = net.layers[-2]
    li = len(net.layers) - 2
    fr = _frames(n, h, w, seed=cout + k)
    eng.calibrate(_frames(4, h, w, seed=99))
    s = eng.int8_scales
    assert s[0] == 0 and s[li] > 0
    got = eng.inference(fr)
    footprint.assert_zero_outside(eng, footprint.tensor_ids(net.layers), n)
    x = eng.debug_tensor(t0, n)
    r = eng.debug_tensor(res, n) if res >= 0 else None
    v = _emulate(L, x, blob, s[li], r)
    stored = eng.debug_tensor(t, n)[:, out_coff:out_coff + cout]
    _fp16_gate(stored, v.astype(np.float16))
    y = np.stack([dict(g)["y"] for g in got])
    if fused:
        scale = float(np.abs(v).max()) + 1e-6
        assert np.abs(y - v).max() <= 2e-6 * scale + 1e-6, "fused fp32 output copy vs the unrounded emulation"
    else:
        assert np.array_equal(y, 2 * stored)
    tiles = {q["layer"]: q["tile"] for q in eng.profile(n, 1)}
    direct = k in (3, 7) and stride == 1 and dil == 1 and -(-cin // 32) * 32 % 64 == 0 and (cout > 64 and -(-cout // 128) * 128 % 128 == 0)
    assert tiles[li] == (8900000 + k if direct else tiles[li]) and 8000000 <= tiles[li] < 9000000, tiles[li]   # conv_i8_direct / conv_i8_kernel


# Signed, tying, saturating inputs.  The cases above quantize relu outputs with a calibrated scale: q_x is never negative, x / s_a never
# lands on a .5 and never passes 127.  Here the layer in front has no activation and the scale is set by hand to a power of two below the
# calibrated one, 2^floor(log2(max|x| / 127)): x / s_a is then exact in fp32 (no rounding before the rint), a few per cent of the fp16 inputs sit
# exactly between two integers (half of them above an even one: half-up, half-away and half-even all differ) and about 1 % lie beyond each
# end of [-127, 127] - the sign handling, the round-half-even and the clamp of quant1, in the generic kernel's loader and in the direct
# kernel's halo loader, at the bit level.  (cin, cout, k, stride): two shapes of conv_i8_kernel, two of conv_i8_direct_kernel.
SIGNED_CASES = [dict(cin=64, cout=128, k=1), dict(cin=64, cout=64, k=3, stride=2), dict(cin=128, cout=128, k=3), dict(cin=128, cout=128, k=7)]
SIGNED_H, SIGNED_W, SIGNED_N = 23, 29, 3


def signed_case(case):
    """The graph (first layer without activation -> the layer under test -> a reader), its frames and its calibration frames."""
    net = Net(case["cin"] * 7 + 128 + 3)
    t0 = net.conv(0, 3, case["cin"], 3, 1, act=E.ACT_NONE)
    t = net.conv(t0, case["cin"], case["cout"], case["k"], case.get("stride", 1))
    z = net.conv(t, case["cout"], 8, 1)
    return net, t0, t, z, _frames(SIGNED_N, SIGNED_H, SIGNED_W, seed=131), _frames(4, SIGNED_H, SIGNED_W, seed=99)


def dyadic_scale(s_calibrated):
    """The largest power of two <= the calibrated scale max|x| / 127."""
    return np.float32(2.0 ** np.floor(np.log2(float(s_calibrated))))


def assert_input_shares(x, s_a):
    """Conditions on the INPUT of the layer under test (x = the stored fp16 values, s_a a power of two), not on the kernel: enough negative
    values, values beyond both clamps and exact ties that a wrong sign, clamp or rounding mode cannot hide below _fp16_gate's 0.1 %."""
    v = x.astype(np.float32) * (np.float32(1) / np.float32(s_a))
    assert np.array_equal(v.astype(np.float64), x.astype(np.float64) / float(s_a)), "x / s_a is not exact: s_a is no power of two"
    tie = np.abs(v - np.floor(v) - 0.5) == 0
    shares = dict(negative=float((v < 0).mean()), low=float((v <= -127.5).mean()), high=float((v >= 127.5).mean()), ties=float(tie.mean()),
                  ties_even_floor=float((tie & (np.floor(v) % 2 == 0)).mean()))
    print("input shares:", {k: round(s, 5) for k, s in shares.items()})
    assert shares["negative"] >= 0.30 and shares["low"] >= 0.003 and shares["high"] >= 0.003 and shares["ties"] >= 0.01, shares
    return shares


@pytest.mark.parametrize("case", SIGNED_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_int8_layer_on_signed_tying_saturating_inputs(hp, case):
    cin, cout, k, stride = case["cin"], case["cout"], case["k"], case.get("stride", 1)
    net, t0, t, z, fr, calib = signed_case(case)
    n, blob, li = SIGNED_N, net.blob(), 1
    L = net.layers[li]
    eng = E.Engine(net.layers, [Out("y", t, 0, cout).c(), Out("z", z, 0, 8).c()], blob, SIGNED_W, SIGNED_H, n, dtype="i8")
    eng.calibrate(calib)
    s = eng.int8_scales
    assert s[0] == 0 and s[li] > 0
    s[li] = dyadic_scale(s[li])
    eng.int8_scales = s
    assert eng.int8_scales[li] == s[li]
    got = eng.inference(fr)
    footprint.assert_zero_outside(eng, footprint.tensor_ids(net.layers), n)
    x = eng.debug_tensor(t0, n)
    assert_input_shares(x, s[li])
    v = _emulate(L, x, blob, s[li])
    _fp16_gate(eng.debug_tensor(t, n), v.astype(np.float16))
    y = np.stack([dict(g)["y"] for g in got])
    scale = float(np.abs(v).max()) + 1e-6
    assert np.abs(y - v).max() <= 2e-6 * scale + 1e-6, "fused fp32 output copy vs the unrounded emulation"
    tiles = {q["layer"]: q["tile"] for q in eng.profile(n, 1)}
    assert tiles[li] == (8900000 + k if (k in (3, 7) and stride == 1 and cout > 64) else tiles[li]) and 8000000 <= tiles[li] < 9000000, tiles[li]


# Sums beyond 2^24.  With random data |acc| stays far below 2^24, where every integer is a float32: a kernel that carried partial sums in fp32
# would pass every case above.  Here the first layer's outputs are all positive (positive weights, bias 1.3), the scale is set by hand to 2^-6 so
# that most inputs saturate at 127 and the rest land on 100 .. 126, and the first third of the output channels has the constant weight
# 127 * 2^-11 in every tap (q_w = 127 everywhere, s_w = 2^-11) and no bias: their acc = 127 * sum q_x, odd as often as not - no float32 above 2^24.
# dq = 2^-17 is a power of two, so for those channels the contract's v = (float)acc * dq is ONE rounding, the int -> float conversion of the exact
# sum, and the fused fp32 copy must equal it bit for bit; an fp32 partial sum rounds somewhere else.  (The fp16 store keeps 11 bits and cannot
# see this: the fp32 copy is the witness.  The other channels keep random weights and the gates above.)
# (cin, cout, k).  127 * 127 * K must pass 2^24: K >= 1041.  A 1 x 1 layer on 512 channels tops out at 8 258 048 and the first layer cannot feed more than
# ~600 channels, so the generic kernel's case is 3 x 3 with 64 outputs (K = 1152, conv_i8_kernel: the direct kernel wants more than 64); the direct
# kernel runs 3 x 3 (18 580 608 at most, reached away from the border) and 7 x 7 on 128 -> 128.
BIG_SUM_CASES = [(128, 128, 3), (128, 128, 7), (128, 64, 3)]
BIG_H, BIG_W, BIG_N = 9, 11, 2


@pytest.mark.parametrize("cin,cout,k", BIG_SUM_CASES, ids=[f"{a}-{b}-{k}x{k}" for a, b, k in BIG_SUM_CASES])
def test_int8_sums_beyond_2_to_the_24_are_exact(hp, cin, cout, k):
    net = Net(cin + k)
    t0 = net.conv(0, 3, cin, 3, 1)
    t = net.conv(t0, cin, cout, k, act=E.ACT_NONE)
    z = net.conv(t, cout, 8, 1)
    blob = net.blob()
    L0, L = net.layers[0], net.layers[1]
    blob[L0.w_off:L0.w_off + cin * 27] = net.rng.uniform(0, 0.12, cin * 27)
    blob[L0.b_off:L0.b_off + cin] = 1.3
    third = cout // 3
    blob[L.w_off:L.w_off + third * k * k * cin] = 127 * 2.0 ** -11
    blob[L.b_off:L.b_off + third] = 0
    net.w = [blob]
    eng = E.Engine(net.layers, [Out("y", t, 0, cout).c(), Out("z", z, 0, 8).c()], blob, BIG_W, BIG_H, BIG_N, dtype="i8")
    eng.calibrate(_frames(4, BIG_H, BIG_W, seed=99))
    s = eng.int8_scales
    assert s[1] > 0
    s[1] = np.float32(2.0 ** -6)
    eng.int8_scales = s
    got = eng.inference(_frames(BIG_N, BIG_H, BIG_W, seed=k))
    x = eng.debug_tensor(t0, BIG_N)
    v, acc = _emulate(L, x, blob, s[1], return_acc=True)
    # conditions on the inputs: saturation with variety, sums beyond 2^24 that are no float32, magnitudes that survive fp16
    q = x / 2.0 ** -6
    assert (x > 0).all() and float((q >= 127.5).mean()) >= 0.4 and float((q < 126.5).mean()) >= 0.05, (float((q >= 127.5).mean()), float((q < 126.5).mean()))
    a3 = acc[:, :third]
    beyond = (np.abs(a3) > 2 ** 24) & (a3.astype(np.float32).astype(np.float64) != a3)
    print(f"{cin}->{cout} {k}x{k}: max |acc| {np.abs(a3).max():.0f}, beyond 2^24 and no float32: {float(beyond.mean()):.3f} of the constant channels' elements")
    assert float(beyond.mean()) >= 0.10
    assert float(np.abs(v).max()) < 65504
    _fp16_gate(eng.debug_tensor(t, BIG_N), v.astype(np.float16))
    y = np.stack([dict(g)["y"] for g in got])
    scale = float(np.abs(v).max()) + 1e-6
    assert np.abs(y - v).max() <= 2e-6 * scale + 1e-6, "fused fp32 output copy vs the unrounded emulation"
    exact = a3.astype(np.float32) * np.float32(2.0 ** -17)
    assert np.array_equal(v[:, :third], exact)
    wrong = y[:, :third] != exact
    assert not wrong.any(), f"{int(wrong.sum())} of {wrong.size} sums are not the exact integer rounded once ({int((wrong & beyond).sum())} of them beyond 2^24)"
    tiles = {r["layer"]: r["tile"] for r in eng.profile(BIG_N, 1)}
    assert (tiles[1] == 8900000 + k) if cout > 64 else (8000000 <= tiles[1] < 8900000), tiles[1]


@pytest.mark.parametrize("cin,cout,k", [(64, 128, 1), (128, 128, 3), (96, 38, 3)], ids=["1x1", "direct-3x3", "generic-3x3-38ch"])
def test_int8_channel_of_zero_weights_is_its_bias(hp, cin, cout, k):
    """max |w| == 0 -> s_w = 1 (no division by zero), q_w = 0, acc = 0: v = 0 * dq + bias, exactly."""
    net = Net(cin + k)
    t0 = net.conv(0, 3, cin, 3, 1)
    t = net.conv(t0, cin, cout, k, act=E.ACT_NONE)
    z = net.conv(t, cout, 8, 1)
    blob = net.blob()
    L = net.layers[1]
    dead = [0, 5, cout - 1]
    for c in dead:
        blob[L.w_off + c * k * k * cin:L.w_off + (c + 1) * k * k * cin] = 0
    net.w = [blob]
    eng = E.Engine(net.layers, [Out("y", t, 0, cout).c(), Out("z", z, 0, 8).c()], blob, 29, 23, 2, dtype="i8")
    eng.calibrate(_frames(4, 23, 29, seed=99))
    s = eng.int8_scales
    assert s[1] > 0
    got = eng.inference(_frames(2, 23, 29, seed=3))
    bias = blob[L.b_off:L.b_off + cout]
    y = np.stack([dict(g)["y"] for g in got])
    stored = eng.debug_tensor(t, 2)
    for c in dead:
        assert bias[c] != 0 and (y[:, c] == bias[c]).all() and (stored[:, c] == np.float32(np.float16(bias[c]))).all(), c
    _fp16_gate(stored, _emulate(L, eng.debug_tensor(t0, 2), blob, s[1]).astype(np.float16))


def test_int8_all_zero_calibration_gives_scale_one(hp):
    """max |x| == 0 -> s_a = 1: all-zero frames through a first layer without bias; the layer's outputs are then exactly its biases."""
    net = Net(9)
    t0 = net.conv(0, 3, 64, 3, 1)
    t = net.conv(t0, 64, 128, 1, act=E.ACT_NONE)
    z = net.conv(t, 128, 8, 1)
    blob = net.blob()
    L0, L = net.layers[0], net.layers[1]
    blob[L0.b_off:L0.b_off + 64] = 0
    net.w = [blob]
    eng = E.Engine(net.layers, [Out("y", t, 0, 128).c(), Out("z", z, 0, 8).c()], blob, 29, 23, 2, dtype="i8")
    zeros = np.zeros((2, 23, 29, 3), np.uint8)
    eng.calibrate(zeros)
    assert eng.int8_scales[1] == 1.0
    got = eng.inference(zeros)
    assert not eng.debug_tensor(t0, 2).any()
    bias = blob[L.b_off:L.b_off + 128]
    y = np.stack([dict(g)["y"] for g in got])
    assert np.array_equal(y, np.broadcast_to(bias[None, :, None, None], y.shape))
    assert np.array_equal(eng.debug_tensor(t, 2), np.broadcast_to(bias.astype(np.float16).astype(np.float32)[None, :, None, None], y.shape))


def test_uncovered_geometry_stays_fp16(hp):
    """A 1 x 1 stride-3 layer has no int8 kernel: scale 0 after calibration, a scale > 0 for it is refused."""
    net = Net(3)
    t0 = net.conv(0, 3, 64, 3, 1)
    t = net.conv(t0, 64, 64, 1, 3)
    eng = E.Engine(net.layers, [Out("y", t, 0, 64).c()], net.blob(), 29, 23, 2, dtype="i8")
    assert list(eng.int8_scales) == [0, 0]
    eng.calibrate(_frames(2, 23, 29))
    assert list(eng.int8_scales) == [0, 0]
    with pytest.raises(_lib.HpError):
        eng.int8_scales = [0, 0.5]


def _no_fuse_f16(monkeypatch, m, w, max_batch):
    monkeypatch.setenv("HP_NO_FUSE", "1")
    e = E.Engine.from_model(m, w, max_batch=max_batch, dtype="f16")
    monkeypatch.delenv("HP_NO_FUSE")
    return e


def _absmax_rule(m, f16, frames):
    """s_a of every eligible layer from the fp16 per-layer engine's tensors: f32(max |x|) / 127 (1 for 0)."""
    want = {}
    for b0 in range(0, len(frames), f16.max_batch):
        f16.inference(frames[b0:b0 + f16.max_batch])
        cnt = len(frames[b0:b0 + f16.max_batch])
        for i, L in enumerate(m.layers):
            if L.op == E.OP_CONV and L.in_ != 0:
                x = f16.debug_tensor(L.in_, cnt)[:, L.in_coff:L.in_coff + L.cin]
                want[i] = max(want.get(i, 0.0), float(np.abs(x).max()))
    return {i: (np.float32(a) / np.float32(127) if a > 0 else np.float32(1)) for i, a in want.items()}


def test_calibration_is_minmax_and_chunk_invariant(hp, monkeypatch):
    m = E.Model("lw_openpose_vggtiny", 64, 48)
    w = m.init_weights(3)
    frames = _frames(5, 48, 64, seed=11)
    e2 = E.Engine.from_model(m, w, max_batch=2, dtype="i8")
    e2.calibrate(frames)                     # 2 * max_batch + 1 frames in chunks
    e5 = E.Engine.from_model(m, w, max_batch=5, dtype="i8")
    e5.calibrate(frames[::-1].copy())        # one chunk, other order
    s2, s5 = e2.int8_scales, e5.int8_scales
    assert np.array_equal(s2, s5)
    want = _absmax_rule(m, _no_fuse_f16(monkeypatch, m, w, 2), frames)
    for i, L in enumerate(m.layers):
        if i in want:
            assert s2[i] == want[i], (i, s2[i], want[i])
        else:
            assert s2[i] == 0, i
    assert (s2 > 0).sum() >= len(m.layers) // 2


def test_scale_zero_is_the_fp16_per_layer_schedule(hp, monkeypatch):
    m = E.Model("lw_openpose_mobilenet", 96, 80)
    w = m.init_weights(1)
    fr = _frames(2, 80, 96, seed=4)
    e8 = E.Engine.from_model(m, w, max_batch=2, dtype="i8")
    e8.int8_scales = np.zeros(len(m.layers), np.float32)
    ref = _no_fuse_f16(monkeypatch, m, w, 2).inference(fr)
    got = e8.inference(fr)
    for b in range(2):
        for (n0, a), (n1, r) in zip(got[b], ref[b]):
            assert n0 == n1 and np.array_equal(a, r), n0


def test_scales_reach_the_kernels_and_state_checks(hp):
    m = E.Model("lw_openpose_vggtiny", 64, 48)
    w = m.init_weights(2)
    fr = _frames(3, 48, 64, seed=5)
    e = E.Engine.from_model(m, w, max_batch=3, dtype="i8")
    with pytest.raises(_lib.HpError) as ex:                  # uncalibrated: HP_ERR_STATE naming calibration
        e.inference(fr)
    assert "calibrat" in str(ex.value)
    assert (e.int8_scales == -1).sum() > 0
    e.calibrate(_frames(4, 48, 64, seed=6))
    a = e.int8_scales
    b = np.where(a > 0, a * 1.7, 0).astype(np.float32)
    e.inference(fr)                                          # captures a graph with scales A
    e.int8_scales = b
    got = e.inference(fr)
    fresh = E.Engine.from_model(m, w, max_batch=3, dtype="i8")
    fresh.int8_scales = b
    ref = fresh.inference(fr)
    for k in range(3):
        for (n0, x), (_, y) in zip(got[k], ref[k]):
            assert np.array_equal(x, y), f"{n0}: a stale graph replayed the old scales"
    alone = e.inference(fr[1:2])[0]                          # batch invariance, bit for bit
    for (n0, x), (_, y) in zip(alone, got[1]):
        assert np.array_equal(x, y), n0
    n = len(m.layers)
    ineligible = int(np.flatnonzero(a == 0)[0])
    for bad in (np.full(n - 1, 0.1, np.float32), np.where(np.arange(n) == ineligible, 0.5, a), np.where(a > 0, -a, 0),
                np.where(a > 0, np.nan, 0), np.where(a > 0, np.inf, 0)):
        with pytest.raises(_lib.HpError):
            e.int8_scales = bad.astype(np.float32)
    assert np.array_equal(e.int8_scales, b)                  # a refused vector changes nothing


def test_save_load_keeps_the_calibration(hp, tmp_path):
    m = E.Model("lw_openpose_vggtiny", 64, 48)
    w = m.init_weights(4)
    fr = _frames(2, 48, 64, seed=7)
    e = E.Engine.from_model(m, w, max_batch=2, dtype="i8")
    e.calibrate(_frames(3, 48, 64, seed=8))
    got = e.inference(fr)
    path = str(tmp_path / "i8.hpeng")
    e.save(path)
    assert open(path, "rb").read(8) == b"HPENG003"
    back = E.Engine.load(path)
    assert back.dtype == E.DTYPE_I8 and np.array_equal(back.int8_scales, e.int8_scales)
    again = back.inference(fr)
    for b in range(2):
        for (n0, x), (_, y) in zip(got[b], again[b]):
            assert np.array_equal(x, y), n0
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-4])                         # a truncated scale vector is an error
    with pytest.raises(_lib.HpError):
        E.Engine.load(path)


class _QuantConv:
    """Stands in for torch.nn.functional inside oracle/ref_net.py: every convolution of a layer whose scale is > 0 is evaluated as the int8
    contract (q_x, q_w, exact integer sums, * dq + bias); everything else - fp16 storage between layers, the fp16 layers, activations,
    residuals, outputs - is ref_net's own fp16-matched evaluation.  The result is the whole-network int8 emulation, independent of the kernels."""

    def __init__(self, layers, blob, scales):
        self.layers, self.blob, self.scales = layers, blob, scales
        self.order = [i for i, L in enumerate(layers) if L.op in (E.OP_CONV, E.OP_DWCONV)]
        self.k = 0

    def __getattr__(self, name):
        return getattr(F, name)

    def conv2d(self, xp, wt, b=None, stride=1, dilation=1, groups=1):
        i = self.order[self.k]
        self.k += 1
        s_a = self.scales[i]
        if s_a <= 0:
            return F.conv2d(xp, wt, b, stride=stride, dilation=dilation, groups=groups)
        L = self.layers[i]
        k, cin, cout = L.kh, L.cin, L.cout
        w = self.blob[L.w_off:L.w_off + cout * k * k * cin].reshape(cout, k, k, cin).astype(np.float32)
        m = np.abs(w).reshape(cout, -1).max(axis=1)
        s_w = np.where(m > 0, m / np.float32(127), np.float32(1)).astype(np.float32)
        q_w = np.clip(np.rint(w / s_w[:, None, None, None]), -127, 127).transpose(0, 3, 1, 2)
        inv_a = np.float32(1) / np.float32(s_a)
        q_x = np.clip(np.rint(xp.numpy().astype(np.float32) * inv_a), -127, 127)
        acc = F.conv2d(torch.from_numpy(q_x.astype(np.float64)), torch.from_numpy(q_w.astype(np.float64)), stride=stride, dilation=dilation).numpy()
        dq = (np.float32(s_a) * s_w).astype(np.float32)
        bias = self.blob[L.b_off:L.b_off + cout].astype(np.float32) if L.b_off >= 0 else np.zeros(cout, np.float32)
        return torch.from_numpy(acc.astype(np.float32) * dq[None, :, None, None] + bias[None, :, None, None])


def _emulate_network(m, w, frames, scales, monkeypatch):
    with monkeypatch.context() as mp:
        mp.setattr(ref_net, "F", _QuantConv(m.layers, w, scales))
        return ref_net.run(m.layers, m.outputs, w, frames_u8=frames, match_fp16=True, mean=m.mean, inv_std=m.inv_std)


def _rel(a, ref):
    return max(float(np.abs(a[n] - ref[n]).max()) / (float(np.abs(ref[n]).max()) + 1e-6) for n in ref)


@pytest.mark.parametrize("arch,w_,h_", [("lw_openpose_mobilenet", 96, 80), ("lw_openpose_vggtiny", 64, 48), ("openpose_vgg19", 64, 48),
                                        ("pose_proposal_resnet50", 160, 128), ("pifpaf_resnet50", 97, 97)])
def test_whole_network_against_the_fp32_oracle(hp, arch, w_, h_, monkeypatch):
    m = E.Model(arch, w_, h_)
    w = m.init_weights(1)
    e = E.Engine.from_model(m, w, max_batch=2, dtype="i8")
    e.calibrate(_frames(4, h_, w_, seed=21))
    scales = e.int8_scales
    assert (scales > 0).sum() >= 3
    fr = _frames(2, h_, w_, seed=22)
    got = e.inference(fr)
    got = {name: np.stack([dict(g)[name] for g in got]) for name, _ in got[0]}
    ref = ref_net.run(m.layers, m.outputs, w, frames_u8=fr, match_fp16=False, mean=m.mean, inv_std=m.inv_std)
    emu = _emulate_network(m, w, fr, scales, monkeypatch)
    engine_vs_fp32, contract_vs_fp32, engine_vs_contract = _rel(got, ref), _rel(emu, ref), _rel(got, emu)
    print(f"{arch}: engine vs fp32 {engine_vs_fp32:.4f}, int8 emulation vs fp32 {contract_vs_fp32:.4f}, engine vs emulation {engine_vs_contract:.4f}")
    # Measured (engine | torch emulation of the int8 contract, no libhp_hip.so kernel involved | engine vs emulation), of max|ref|:
    #   lw_openpose_mobilenet 0.080 | 0.080 | 0.062     lw_openpose_vggtiny 0.046 | 0.052 | 0.039     openpose_vgg19 0.060 | 0.060 | 0.000
    #   pose_proposal_resnet50 0.059 | 0.077 | 0.083    pifpaf_resnet50 0.024 | 0.022 | 0.024
    # The contract itself misses the issue's 5e-2 estimate on three topologies, so no implementation of it can meet that bound.  Where the
    # fp16 layers sum in another order than torch (depthwise, residual networks), single fp16 rounding flips move q_x across a rounding
    # boundary and the two evaluations part by the contract's own noise level; on openpose_vgg19 (no such layers) they agree exactly.
    # The gate: the engine no further from fp32 than the contract (1.5 x + 1e-2); a wrong scale or lane map gives errors of order 1.
    assert engine_vs_fp32 <= 1.5 * contract_vs_fp32 + 1e-2


def test_int8_error_per_layer(hp, monkeypatch):
    """Where the whole-network error of lw_openpose_mobilenet comes from: the int8 emulation with ONE layer quantized at a time (all others
    fp16) against the all-fp16 evaluation.  No single layer may account for the whole error - a badly calibrated layer would."""
    m = E.Model("lw_openpose_mobilenet", 96, 80)
    w = m.init_weights(1)
    e = E.Engine.from_model(m, w, max_batch=2, dtype="i8")
    e.calibrate(_frames(4, 80, 96, seed=21))
    scales = e.int8_scales
    fr = _frames(2, 80, 96, seed=22)
    base = ref_net.run(m.layers, m.outputs, w, frames_u8=fr, match_fp16=True, mean=m.mean, inv_std=m.inv_std)
    whole = _rel(_emulate_network(m, w, fr, scales, monkeypatch), base)
    per = {}
    for i in np.flatnonzero(scales > 0):
        one = np.where(np.arange(len(scales)) == i, scales, 0).astype(np.float32)
        per[int(i)] = _rel(_emulate_network(m, w, fr, one, monkeypatch), base)
    top = sorted(per.items(), key=lambda kv: -kv[1])[:5]
    print(f"int8 layers {len(per)}, whole-network error vs fp16 {whole:.4f}; largest single-layer errors: "
          + ", ".join(f"layer {i} ({m.layers[i].cin}->{m.layers[i].cout} {m.layers[i].kh}x{m.layers[i].kw}) {v:.4f}" for i, v in top))
    assert top[0][1] < 0.5 * whole, top


def test_keypoint_drift_configs1(hp):
    """Test 7, configs[1] at full size (8 x 368 x 432), the weights and frames of test_pipeline_gpu.py's kHALF drift measurement, the kINT8
    engine calibrated on other synthetic frames: heat-map error against the pure fp32 oracle.  (The peak comparison of that measurement
    cannot run here: on these random-weight maps, blown up x 400 at the outputs, the int8 noise raises more candidates per limb than the PAF
    parser's hard list holds (> 8388 on frame 4) - measured)"""
    from oracle import ref_net as rn
    in_w, in_h, B = 432, 368, 8
    m = E.Model("lw_openpose_mobilenet", in_w, in_h)
    w = m.init_weights(11)
    for L in m.layers:
        if L.op == E.OP_CONV and L.cout in (19, 38) and L.out in [o.tensor for o in m.outputs]:
            w[L.w_off:L.w_off + L.cout * L.cin] *= 400.0
    frames = np.random.default_rng(21).integers(0, 256, (B, in_h, in_w, 3), dtype=np.uint8)
    eng = E.Engine.from_model(m, w, max_batch=B, dtype="i8")
    eng.calibrate(np.random.default_rng(5).integers(0, 256, (B, in_h, in_w, 3), dtype=np.uint8))
    got = eng.inference(frames)
    ref = rn.run(m.layers, m.outputs, w, frames_u8=frames, match_fp16=False, device="cuda" if torch.cuda.is_available() else "cpu")
    map_err = max(float(np.abs(got[b][k][1] - ref[n][b]).max() / np.abs(ref[n][b]).max()) for b in range(B) for k, n in enumerate(("conf", "paf")))
    print(f"kINT8 configs[1] @ {in_h}x{in_w} x {B}: heat-map max rel err {map_err:.4f}")
    # Measured 0.103 (kHALF: < 2e-2).  The issue's 5e-2 estimate is missed here as on the reduced-size networks, where the torch emulation of
    # the int8 contract shows the same error as the engine (test_whole_network_against_the_fp32_oracle: lw_openpose_mobilenet 0.080 | 0.080,
    # spread over its 42 int8 layers, test_int8_error_per_layer).  The bound below only separates that from a broken scale (order 1).
    assert map_err < 0.15, map_err


def test_pipeline_over_a_calibrated_engine(hp):
    """A stream of I8 engines created from one engine's calibrated scales == that engine + the PAF parser called by hand."""
    from hyperpose_amd.parser import Paf
    from hyperpose_amd.pipeline import Pipeline
    m = E.Model("lw_openpose_vggtiny", 64, 48)
    w = m.init_weights(5)
    e = E.Engine.from_model(m, w, max_batch=2, dtype="i8")
    with pytest.raises(_lib.HpError):                        # no scales: HP_ERR_STATE
        Pipeline(m, w, max_batch=2, n_pipes=1, dtype="i8", max_frame_wh=(64, 48))
    e.calibrate(_frames(3, 48, 64, seed=9))
    fr = _frames(2, 48, 64, seed=10)
    pl = Pipeline(m, w, max_batch=2, n_pipes=2, dtype="i8", max_frame_wh=(64, 48), conf_thresh=0.05, paf_thresh=-1e9,
                  int8_scales=e.int8_scales)
    pl.submit(list(fr))
    got = pl.collect()
    pl.close()
    maps = e.inference(fr)
    want = Paf(conf_thresh=0.05, paf_thresh=-1e9, max_batch=2).process_batch(np.stack([mp[0][1] for mp in maps]),
                                                                           np.stack([mp[1][1] for mp in maps]))
    assert len(got) == 2
    for g, r in zip(got, want):
        assert g.tobytes() == r.tobytes()


def test_cpp_mirror_int8_flow_runs(hp, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "operator_api_int8")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "operator_api_int8.cpp"),
                           "-L" + os.path.join(root, "hyperpose_amd"), "-lhp_hip", "-lpthread", "-Wl,-rpath," + os.path.join(root, "hyperpose_amd"),
                           "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "e.hpeng")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    tag, humans, frames = out.stdout.split()[-3:]
    assert tag == "OK" and int(frames) == 4


def test_cli_int8_calibrates_on_the_first_batch(hp, tmp_path):
    import subprocess
    import test_cli
    test_cli._build()
    r = subprocess.run([test_cli.BIN, "--model", "builtin:lw_openpose_mobilenet", "--post=paf", "--w", "160", "--h=128", "--max_batch_size", "3",
                        "--source=synthetic:5:200x150", "--int8", "--saving_prefix", str(tmp_path / "o"), "--noimshow"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "--int8: calibrated the kINT8 engine on the first 3 frame(s)" in r.stderr
    assert "5 images got processed" in r.stdout
