"""GPU: the epilogues ("drains") of the fp32 GEMM kernels, bit for bit against values that do not depend on the order of summation.

conv32_t16_kernel's drain and conv32_drain_rows (conv32_kernel's row form, conv32_direct_kernel) compute a lane's
pixel offsets with one division pair and carries, request bias, slopes and residual from clamped addresses, and choose the quad or the
scalar path per launch.  What can go wrong there is an offset, a guard or an operand - not a rounding - so the expected
values are made exact: weights, biases and the network input are small integers, act_hi = 6, the leaky slope 0.25, PReLU slopes powers of
two.  With Cin <= 64 every product, partial sum and epilogue result is then an fp32 number, the layer has ONE result whatever its kernel, and
EVERY element of the tested tensor is compared bitwise (no tolerance) with float64 numpy in the documented order: sum, + bias, + residual
before the activation, clamp or slope, + residual after.  The layer's actual input and residual are read with the debug tensor tap.

One engine per (kernel, map, Cin) holds eighteen tested 1 x 1 layers: Cout 64 (whole quads) | 70 (a ragged quad, a second channel group
that is mostly padding) | 19 (no quad path) x residual none | before | after the activation x whole tensors | an output that is a slice of
a wider buffer at channel 3 with a residual tensor wider than Cout (the network's concat at channel 147: the scalar path; a layer
description has no residual channel offset, so the residual's own slice starts at channel 0).  Maps: 1 x 1 at batch 1 (one valid pixel) and
7 x 11 at batch 3 (231 pixels: two image boundaries inside the first 160-pixel tile, a ragged last tile, rows and images changing inside
one 16-pixel MFMA tile - the carries).  Cin 16 (one K-step: the loop's clamped re-load) and 48 (three; a slice of a 64-channel tensor).
Every tested tensor has a halo (a 3 x 3 dilation-2 consumer); halo, separator rows and channels past Cout must still read zero
(raw-buffer tap), and frame 1 alone equals frame 1 of the batch.  The tile code of every tested layer is asserted from profile().

The kernel that only shares the drain, conv32_direct_kernel, gets one case.
"""
import numpy as np
import pytest

import footprint
from hyperpose_amd import engine as E
from test_engine_footprint_gpu import _set_env, guarded, halo
from test_engine_gpu import Net, Out

pytestmark = pytest.mark.gpu

ACTS = [(E.ACT_RELU6, 0.0), (E.ACT_LEAKY, 0.25), (E.ACT_PRELU, 0.0), (E.ACT_NONE, 0.0)]
MAPS = {"1x1-batch1": (1, 1, 1), "7x11-batch3": (3, 7, 11)}
KERNELS = {
    "t16-64x160": (dict(HP_C32_BN160="1", HP_C32_WK="0", HP_NO_ARENA="1"), 32064160),
    "rows-64x64": (dict(HP_C32_WK="0", HP_NO_ARENA="1"), 32464064),
}
SLICE_AT = 3   # the sliced output's channel offset: no multiple of four


class ExactNet(Net):
    """Net with small-integer weights and biases and power-of-two PReLU slopes."""

    def _alloc(self, n, std):
        off = sum(len(x) for x in self.w)
        self.w.append(self.rng.integers(-2, 3, n).astype(np.float32))
        return off

    def conv(self, *a, **kw):
        t = super().conv(*a, **kw)
        if kw.get("act", E.ACT_RELU) == E.ACT_PRELU:
            self.w[-1][:] = self.rng.choice(np.array([0.5, 0.25, 0.125], np.float32), len(self.w[-1]))
        return t


def _expected(L, blob, x, res):
    """Layer L (any square kernel, stride 1, SAME) on x [n, cin, h, w] in float64, in the epilogue's order; res [n, >= cout, h, w] or None."""
    n, cin, h, w = x.shape
    k, pad = L.kh, (L.kh - 1) // 2
    wt = blob[L.w_off:L.w_off + L.cout * k * k * cin].astype(np.float64).reshape(L.cout, k, k, cin)
    xp = np.zeros((n, cin, h + 2 * pad, w + 2 * pad))
    xp[:, :, pad:pad + h, pad:pad + w] = x
    v = np.zeros((n, L.cout, h, w))
    for ky in range(k):
        for kx in range(k):
            v += np.einsum("oc,nchw->nohw", wt[:, ky, kx, :], xp[:, :, ky:ky + h, kx:kx + w])
    v = v + blob[L.b_off:L.b_off + L.cout].astype(np.float64)[None, :, None, None]
    if res is not None and L.res_before_act:
        v = v + res[:, :L.cout]
    if L.act == E.ACT_RELU6:
        slope, hi = 0.0, 6.0
    elif L.act == E.ACT_LEAKY:
        slope, hi = float(L.act_param), np.inf
    elif L.act == E.ACT_PRELU:
        slope, hi = blob[L.alpha_off:L.alpha_off + L.cout].astype(np.float64)[None, :, None, None], np.inf
    else:
        slope, hi = 1.0, np.inf
    v = np.where(v > 0, np.minimum(v, hi), v * slope)     # y = v > 0 ? min(v, act_hi) : v * slope
    if res is not None and not L.res_before_act:
        v = v + res[:, :L.cout]
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v), "the expected values are not fp32 numbers: the case is not exact"
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _graph(cin, couts, k=1, sliced=(False, True), in_coff=0):
    """stem (integers 0 .. 6; the tested layers read its channels in_coff ..) and two residual sources, then per (Cout, residual, layout) a
    tested layer and its halo consumer.
    Returns the net, the outputs and [(layer index, tensor, channel offset, residual tensor or -1)]."""
    net = ExactNet(11)
    t0 = net.conv(0, 3, in_coff + cin, 3, 1, act=E.ACT_RELU6)
    tested, outs, a = [], [], 0
    for cout in couts:
        r_whole = net.conv(0, 3, cout, 3, 1, act=E.ACT_RELU6)
        r_wide = net.conv(0, 3, cout + 13, 3, 1, act=E.ACT_RELU6)
        for res in (None, "before", "after"):
            for sl in sliced:
                act, param = ACTS[a % len(ACTS)]
                a += 1
                kw = dict(act=act, act_param=param, in_coff=in_coff)
                r = -1 if res is None else r_wide if sl else r_whole
                if res is not None:
                    kw.update(res=r, res_before_act=1 if res == "before" else 0)
                if sl:
                    t = net.new_tensor()
                    net.conv(t0, cin, SLICE_AT, 1, out=t, out_coff=0, act=E.ACT_NONE, in_coff=in_coff)
                    net.conv(t0, cin, cout, k, out=t, out_coff=SLICE_AT, **kw)
                    width = SLICE_AT + cout
                else:
                    t = net.conv(t0, cin, cout, k, **kw)
                    width = cout
                li = len(net.layers) - 1
                tested.append((li, t, SLICE_AT if sl else 0, r))
                y, c = halo(net, t, width)
                outs.append(Out(f"y{len(outs)}", y, 0, c))
    return net, t0, outs, tested


def _run_case(monkeypatch, env, code, n, h, w, cin, couts, **graph_kw):
    _set_env(monkeypatch, env)
    in_coff = graph_kw.get("in_coff", 0)
    net, t0, outs, tested = _graph(cin, couts, **graph_kw)
    blob = net.blob()
    eng = E.Engine(net.layers, [o.c() for o in outs], blob, w, h, n, factor=1.0, dtype="f32")
    frames = np.random.default_rng(h * 100 + w).integers(0, 4, (n, h, w, 3), dtype=np.uint8)
    eng.inference(frames)
    ids = footprint.tensor_ids(net.layers)
    assert footprint.assert_zero_outside(eng, ids, n, f"{code} {n}x{h}x{w}") >= len(tested)   # halo, separator rows, channels past Cout
    x = eng.debug_tensor(t0, n).astype(np.float64)[:, in_coff:]
    assert x.shape == (n, cin, h, w) and x.min() >= 0 and x.max() <= 6 and np.array_equal(x, np.round(x))
    got = {}
    for li, t, coff, r in tested:
        L = net.layers[li]
        assert eng.debug_raw(t)[1]["P"] >= 2
        res = eng.debug_tensor(r, n).astype(np.float64) if r >= 0 else None
        want = _expected(L, blob, x, res)
        mine = eng.debug_tensor(t, n)[:, coff:coff + L.cout]
        got[li] = mine
        bad = _bits(mine) != _bits(want)
        assert not bad.any(), (code, (n, h, w), cin, L.cout, L.act, r >= 0 and (L.res_before_act, r), coff, int(bad.sum()),
                               [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:6]], mine[bad][:6], want[bad][:6])
    rows = {r_["layer"]: r_["tile"] for r_ in eng.profile(n, 1)}
    assert all(rows.get(li) == code for li, _, _, _ in tested), (code, [(li, rows.get(li)) for li, _, _, _ in tested])
    if n > 1:   # batch invariance: frame 1 alone
        eng.inference(frames[1:2])
        for li, t, coff, _ in tested:
            alone = eng.debug_tensor(t, 1)[0, coff:coff + net.layers[li].cout]
            assert np.array_equal(_bits(alone), _bits(got[li][1])), (code, li, "frame 1 alone differs from frame 1 of the batch")
    eng.close()


@pytest.mark.parametrize("cin", [16, 48])
@pytest.mark.parametrize("size", list(MAPS))
@pytest.mark.parametrize("kernel", list(KERNELS))
@guarded
def test_gemm_drains_are_exact(hp, monkeypatch, kernel, size, cin):
    env, code = KERNELS[kernel]
    n, h, w = MAPS[size]
    # (a 1 x 1 layer of <= 64 padded outputs whose input buffer holds a whole 64-channel chunk from the slice's first channel goes to
    # conv32_direct_kernel: the 48-channel input is therefore channels 16 .. 63 of the stem's 64)
    _run_case(monkeypatch, env, code, n, h, w, cin, (64, 70, 19), in_coff=16 if cin == 48 else 0)


@guarded
def test_direct_kernel_shares_the_drain(hp, monkeypatch):
    """conv32_direct_kernel (1 x 1 on whole 64-channel chunks, narrow outputs): 38 channels, whole and sliced, every residual form."""
    _run_case(monkeypatch, dict(HP_NO_ARENA="1"), 34001001, 3, 7, 11, 64, (38,))
