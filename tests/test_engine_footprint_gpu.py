"""GPU: what the convolution kernels write OUTSIDE their outputs (tests/footprint.py over Engine.debug_raw).

The engine zero-fills every activation buffer once and never again: the halo (P pixels around each image), the separator rows of fp32
buffers and the pad channels C .. cs - 1 must stay zero whatever runs, frames n .. max_batch - 1 must not be touched by a batch of n, and
a producer of a concat slice must not spill into its neighbour.  The kernel-level tests elsewhere look at network outputs (P = 0); here

  (a) every activation-writing kernel family writes a tensor that HAS a halo (a 3 x 3 dilation-2 consumer: P = 2; 7 x 7: P = 3) on maps one
      pixel larger and one pixel smaller than its tile, batch 3, odd H for the fp32 engines; the profile's tile code is asserted, so a
      routing change cannot empty a case;
  (b) unaligned concat slices [32 | 19 | 38 | 39] are written right to left, so that a spill into the right neighbour stays visible;
  (c) partial batches on a max_batch = 4 engine leave frames n .. bitwise alone;
  (d) the five built-in topologies, small, in all four precisions: everything the tap shows - every arena buffer included - is zero outside.

Values: the tested tensor (test tap) and the consumer's output against the oracle at the tolerance the family's own test uses (_close /
_close32, unchanged).  The tested tensor is read through hp_engine_debug_tensor and not exported: the fused families refuse a tensor that
is a network output, and a plain export moves a layer to the epilogue with the fused fp32 copy - either would empty the case.
int8 layers are compared with the quantization contract's emulation (test_engine_int8_gpu._emulate / _fp16_gate).
"""
import functools

import numpy as np
import pytest

import footprint
from hyperpose_amd import engine as E
from hyperpose_amd import synth
from oracle import ref_net
from test_engine_fp32_gpu import _close32
from test_engine_gpu import Net, Out, _close, _frames
from test_engine_graphs_gpu import _guarded
from test_engine_int8_gpu import _emulate, _fp16_gate

pytestmark = pytest.mark.gpu

N = 3
ENV_KEYS = ("HP_NO_FUSE", "HP_FUSE32", "HP_NO_FUSE32", "HP_NO_HEAD32", "HP_HEAD_PAIR", "HP_NO_WINOGRAD32", "HP_WINO_NC", "HP_WINO_TALL",
            "HP_C32_BN160", "HP_C32_WK", "HP_LANE_EPILOGUE", "HP_DW32_PX", "HP_NO_SPLITK", "HP_NO_CHAIN", "HP_NO_BNECK", "HP_NO_SEPPAIR", "HP_NO_ARENA", "HP_NO_PAIR_HEADS")


def guarded(fn):
    """A failed HIP call ends the session (test_engine_graphs_gpu._guarded): nothing more is started on a device that faulted."""
    @functools.wraps(fn)
    def run(*a, **kw):
        return _guarded(lambda: fn(*a, **kw))
    return run


class Case:
    """One graph: `build(net)` returns (tested tensors, consumer outputs [(tensor, channels)]); `want(rows)` is true when the profile rows
    (dicts layer / op / tile) show the kernel the case is about; `sizes` = frame sizes (h, w); `tol` = the family's own _close arguments."""

    def __init__(self, name, dtype, build, want, sizes, env=None, tol=None, seed=3, differs_from=None):
        self.name, self.dtype, self.build, self.want, self.sizes, self.env, self.tol, self.seed = name, dtype, build, want, sizes, env or {}, tol or {}, seed
        self.differs_from = differs_from   # environment of a second engine whose tested tensor must differ somewhere: proves a form no tile code shows


def _around(th, tw):
    """Maps one pixel larger and one pixel smaller than a th x tw tile (th even: both heights are odd, what the fp32 engines need)."""
    return [(th + 1, tw + 1), (th - 1, tw - 1)]


def halo(net, t, c, p=2):
    """The consumer that gives `t` a halo of p pixels: 3 x 3 dilation 2 (p = 2) or 7 x 7 (p = 3); a network output."""
    return (net.conv(t, c, 8, 3, dil=2, act=E.ACT_NONE) if p == 2 else net.conv(t, c, 8, 7, act=E.ACT_NONE)), 8


def tile_at(layer, pred):
    return lambda rows: any(r["layer"] == layer and pred(r) for r in rows)


def has_tile(pred, count=None):
    return lambda rows: (sum(bool(pred(r["tile"])) for r in rows) >= 1) if count is None else (sum(bool(pred(r["tile"])) for r in rows) == count)


def op_at(layer, op):
    return tile_at(layer, lambda r: r["op"] == op and r["tile"] == 0)


# ---------------------------------------------------------------- (a) graphs: one per kernel family
def g_first(cout, k, stride=1, act=E.ACT_RELU, p=2):
    def build(net):
        t = net.conv(0, 3, cout, k, stride, act=act, act_param=0.1)
        return [t], [halo(net, t, cout, p)]
    return build


def g_dense(cin, cout, k, stride=1, dil=1, act=E.ACT_RELU, res=None, p=2, stem_act=E.ACT_RELU, res_c=0):
    """stem -> the layer under test (layer 1, or 2 with a residual) -> consumer.  `res_c`: channels of the residual's tensor where it has more
    than the layer writes (the residual of pad channel Cout is then NOT zero: an epilogue that forgets the channel guard writes a value there)."""
    def build(net):
        t0 = net.conv(0, 3, cin, 3, 1, act=stem_act)
        r = net.conv(0, 3, res_c or cout, 3, stride) if res else -1
        t = net.conv(t0, cin, cout, k, stride, dil, act=act, act_param=0.1, res=r, res_before_act=1 if res == "before" else 0)
        return [t], [halo(net, t, cout, p)]
    return build


def g_simple(op, c, k, stride=1, dil=1, act=E.ACT_NONE, kind=None):
    """stem -> depthwise / pool / upsample (layer 1) -> consumer."""
    def build(net):
        t0 = net.conv(0, 3, c, 3, 1, act=E.ACT_LEAKY, act_param=0.5)
        if op == E.OP_UPSAMPLE:
            t = net.new_tensor()
            up = E.make_layer(E.OP_UPSAMPLE, t0, t, c, c, 1, stride, 1, E.ACT_NONE)
            up.kh = kind
            net.layers.append(up)
        else:
            t = net.conv(t0, c, c, k, stride, dil, op=op, act=act, act_param=0.1)
        return [t], [halo(net, t, c)]
    return build


def g_sep(c, cout, stride=1, dil=1, act=E.ACT_RELU):
    def build(net):
        a = net.conv(0, 3, c, 3, 1)
        d = net.conv(a, c, c, 3, stride, dil, op=E.OP_DWCONV, act=E.ACT_RELU6)
        y = net.conv(d, c, cout, 1, act=act, act_param=0.1)
        return [y], [halo(net, y, cout)]
    return build


def g_seppair(net):
    a = net.conv(0, 3, 32, 3, 1)
    d1 = net.conv(a, 32, 32, 3, 1, op=E.OP_DWCONV)
    p1 = net.conv(d1, 32, 64, 1)
    d2 = net.conv(p1, 64, 64, 3, 2, op=E.OP_DWCONV)
    p2 = net.conv(d2, 64, 128, 1)
    return [p2], [halo(net, p2, 128)]


def g_chain(variant, act=E.ACT_RELU):
    def build(net):
        t = net.conv(0, 3, 128, 3, 1)
        if variant.startswith("block"):
            u = net.conv(t, 128, 128, 1, act=act)
            v = net.conv(u, 128, 128, 3, act=act)
            y = net.conv(v, 128, 128, 3, act=act, res=u if variant == "block" else -1)
        else:
            v = net.conv(t, 128, 128, 3, act=act, res=t if variant == "pair_res1" else -1)
            y = net.conv(v, 128, 128, 3, act=act, res=t if variant == "pair_res2" else -1)
        return [y], [halo(net, y, 128)]
    return build


def g_bneck(m, mr, front):
    def build(net):
        x = net.conv(0, 3, 4 * m, 3, 1)
        if front:
            r = net.conv(x, 4 * m, m, 1)
            v = net.conv(r, m, m, 3)
        else:
            v = net.conv(x, 4 * m, m, 3, 1)
        y = net.conv(v, m, 4 * m, 1, res=x, res_before_act=1)
        tested, outs = [y], []
        if mr:
            z = net.conv(y, 4 * m, mr, 1)
            tested.append(z)
            outs.append(halo(net, z, mr))
        outs.append(halo(net, y, 4 * m))
        return tested, outs
    return build


def g_bneck_proj(mr, own):
    def build(net):
        x = net.conv(0, 3, 64, 3, 1)
        pj = net.conv(x, 64, 256, 1, act=E.ACT_NONE)
        if own is None:
            r = net.conv(x, 64, 96, 1)
            v = net.conv(r, 96, 64, 3)
        else:
            r = net.conv(x, 64, 64, 1)
            v = net.conv(r, 64, 64, 3)
        y = net.conv(v, 64, 256, 1, res=pj, res_before_act=1)
        tested, outs = [y], []
        if mr:
            z = net.conv(y, 256, mr, 1)
            tested.append(z)
            outs.append(halo(net, z, mr))
        outs.append(halo(net, y, 256))
        if not own:
            outs.append((net.conv(r, 64, 32, 1, act=E.ACT_NONE), 32))
        return tested, outs
    return build


def g_head16(k1, cout2):
    """mlp_head_kernel writing an unaligned slice of a concat buffer that has a halo."""
    def build(net):
        a = net.conv(0, 3, k1, 3, 1)
        cat = net.new_tensor()
        net.conv(a, k1, 32, 1, out=cat, out_coff=0)
        hid = net.conv(a, k1, 512, 1, act=E.ACT_RELU)
        net.conv(hid, 512, cout2, 1, act=E.ACT_NONE, out=cat, out_coff=32)
        return [cat], [halo(net, cat, 32 + cout2)]
    return build


def g_sep32(c, cout, dil):
    def build(net):
        t0 = net.conv(0, 3, c, 3, 1)
        d = net.conv(t0, c, c, 3, 1, dil, op=E.OP_DWCONV, act=E.ACT_RELU6)
        y = net.conv(d, c, cout, 1, act=E.ACT_RELU)
        return [y], [halo(net, y, cout)]
    return build


def g_head32(hid, paired):
    """LW-OpenPose's stage layout (test_fused_two_layer_heads): both heads write slices of a concat buffer, the second at channel 147."""
    def build(net):
        cat = net.new_tensor()
        t0 = net.conv(0, 3, 32, 3, 1)
        net.conv(t0, 32, 128, 3, 1, out=cat, out_coff=0)
        trunk = net.conv(cat, 128, 128, 1, 1, in_coff=0)
        a = net.conv(trunk, 128, hid, 1, 1, act=E.ACT_RELU)
        net.conv(a, hid, 19, 1, 1, out=cat, out_coff=128, act=E.ACT_NONE)
        if paired:
            b = net.conv(trunk, 128, hid, 1, 1, act=E.ACT_RELU)
            net.conv(b, hid, 38, 1, 1, out=cat, out_coff=147, act=E.ACT_NONE)
        return [cat], [halo(net, cat, 185 if paired else 147)]
    return build


def g_i8(cin, cout, k):
    def build(net):
        t0 = net.conv(0, 3, cin, 3, 1)
        t = net.conv(t0, cin, cout, k)
        return [t], [halo(net, t, cout)]
    return build


GEMM16 = [(9, 15), (7, 9)]        # kernels whose tile is a run of 64 / 128 pixels of the whole batch: 405 and 189 pixels, no multiple of either
GEMM32 = [(9, 15), (7, 9)]        # (odd heights: fp32 buffers then carry a separator row)
T16x12, T8x12, T4x8, T8x8 = _around(16, 12), _around(8, 12), _around(4, 8), _around(8, 8)
generic16 = lambda t: 0 < t < 1000000                                           # conv_mfma_kernel: BM * 1000 + BN
CASES = [
    # ---- fp16
    # (first-layer rows carry tile 0 whichever kernel runs: that "f16form" cases run first_conv_f16_kernel - 3 x 3 | 7 x 7, Cout % 8 == 0,
    # Cout <= 64 - and "plain" ones first_conv_kernel rests on reading launch_first_conv, not on an assertion; op and layer are asserted)
    Case("f16-first-f16form-3x3", "f16", g_first(32, 3), op_at(0, E.OP_CONV), _around(16, 32)),
    Case("f16-first-f16form-7x7-leaky", "f16", g_first(64, 7, act=E.ACT_LEAKY, p=3), op_at(0, E.OP_CONV), _around(16, 32)),
    Case("f16-first-f16form-stride2", "f16", g_first(24, 3, 2), op_at(0, E.OP_CONV), [(33, 65), (31, 63)]),
    Case("f16-first-plain-20ch", "f16", g_first(20, 3), op_at(0, E.OP_CONV), _around(16, 32)),
    Case("f16-first-plain-5x5", "f16", g_first(32, 5), op_at(0, E.OP_CONV), _around(16, 32)),
    Case("f16-mfma-fast-dil2", "f16", g_dense(96, 128, 3, dil=2), tile_at(1, lambda r: generic16(r["tile"])), GEMM16),
    Case("f16-mfma-fast-stride2", "f16", g_dense(64, 64, 3, stride=2), tile_at(1, lambda r: generic16(r["tile"])), [(17, 29), (13, 17)]),
    Case("f16-mfma-slow-19ch", "f16", g_dense(96, 19, 1, act=E.ACT_NONE), tile_at(1, lambda r: generic16(r["tile"])), GEMM16),
    Case("f16-mfma-slow-38ch-3x3", "f16", g_dense(128, 38, 3, act=E.ACT_NONE), tile_at(1, lambda r: generic16(r["tile"])), GEMM16),
    Case("f16-small1x1-64", "f16", g_dense(64, 128, 1), tile_at(1, lambda r: r["tile"] == 5100064), GEMM16),
    Case("f16-small1x1-128-512", "f16", g_dense(128, 512, 1), tile_at(1, lambda r: r["tile"] == 5100128), GEMM16),
    Case("f16-big1x1", "f16", g_dense(256, 256, 1), tile_at(1, lambda r: r["tile"] == 5201002), GEMM16),
    Case("f16-big1x1-residual", "f16", g_dense(256, 512, 1, res="before"), tile_at(2, lambda r: r["tile"] == 5201002), GEMM16),
    # The channel configurations of test_pixel_block_gemm_through_the_fast_epilogue, whose ResNet-sized maps are beyond footprint.RAW_LIMIT.
    # Small maps run conv1x1_big_kernel<1, 2> (5201002); those tests run <2, 2> (5202002: >= 320 blocks of 64 pixels x 256 channels), reached
    # here with 1024 outputs on 3 x 41 x 43 pixels; <1, 4> (5201004) takes padded outputs that are no multiple of 256 with >= 1024 blocks
    Case("f16-big1x1-1024-residual", "f16", g_dense(256, 1024, 1, res="before"), tile_at(2, lambda r: r["tile"] == 5201002), GEMM16),
    Case("f16-big1x1-256-residual", "f16", g_dense(256, 256, 1, res="before"), tile_at(2, lambda r: r["tile"] == 5201002), GEMM16),
    Case("f16-big1x1-1024-residual-2x2", "f16", g_dense(256, 1024, 1, res="before"), tile_at(2, lambda r: r["tile"] == 5202002), [(41, 43)]),
    Case("f16-big1x1-640-1x4", "f16", g_dense(256, 640, 1), tile_at(1, lambda r: r["tile"] == 5201004), [(95, 95)]),
    Case("f16-small1x1-256-residual", "f16", g_dense(256, 128, 1, res="after"), tile_at(2, lambda r: r["tile"] == 5100256), GEMM16),
    Case("f16-big1x1-stride2-odd-map", "f16", g_dense(256, 512, 1, stride=2), tile_at(1, lambda r: r["tile"] == 5201002), [(17, 29), (13, 17)]),
    Case("f16-conv3x3-direct-128", "f16", g_dense(128, 128, 3), tile_at(1, lambda r: r["tile"] == 5064192), T16x12),
    Case("f16-conv3x3-direct-64-prelu", "f16", g_dense(64, 64, 3, act=E.ACT_PRELU), tile_at(1, lambda r: r["tile"] == 5064192), T16x12),
    Case("f16-direct-5x5", "f16", g_dense(256, 128, 5), tile_at(1, lambda r: r["tile"] == 6256025), T16x12),
    Case("f16-direct-7x7-residual", "f16", g_dense(256, 128, 7, res="after", p=3), tile_at(2, lambda r: r["tile"] == 6256049), T16x12),
    # (3 x 3 layers take conv_direct_kernel only on maps its tiles cover well: one pixel smaller than one / two tiles; few blocks: split-K)
    Case("f16-direct-3x3-splitk", "f16", g_dense(256, 128, 3, act=E.ACT_PRELU), tile_at(1, lambda r: r["tile"] == 6256009), [(15, 11), (31, 23)],
         differs_from=dict(HP_NO_SPLITK="1")),   # (the tile code is the unsplit launch's too: the split shows as another fp32 summation order)
    Case("f16-direct-3x3-splitk4", "f16", g_dense(512, 128, 3), tile_at(1, lambda r: r["tile"] == 6512009), [(15, 11), (31, 23)],
         differs_from=dict(HP_NO_SPLITK="1")),
    Case("f16-depthwise", "f16", g_simple(E.OP_DWCONV, 32, 3, act=E.ACT_LEAKY), op_at(1, E.OP_DWCONV), _around(8, 8)),
    Case("f16-depthwise-stride2", "f16", g_simple(E.OP_DWCONV, 32, 3, stride=2, act=E.ACT_RELU6), op_at(1, E.OP_DWCONV), [(17, 17), (14, 14)]),
    Case("f16-depthwise-dil2", "f16", g_simple(E.OP_DWCONV, 40, 3, dil=2, act=E.ACT_RELU), op_at(1, E.OP_DWCONV), _around(8, 8)),
    Case("f16-maxpool-3-2", "f16", g_simple(E.OP_MAXPOOL, 32, 3, stride=2), op_at(1, E.OP_MAXPOOL), [(17, 17), (14, 14)]),
    Case("f16-maxpool-2-2", "f16", g_simple(E.OP_MAXPOOL, 24, 2, stride=2), op_at(1, E.OP_MAXPOOL), [(17, 17), (14, 14)]),
    Case("f16-upsample-nearest", "f16", g_simple(E.OP_UPSAMPLE, 32, 1, stride=2, kind=0), op_at(1, E.OP_UPSAMPLE), [(9, 5), (4, 7)]),
    Case("f16-upsample-bilinear", "f16", g_simple(E.OP_UPSAMPLE, 24, 1, stride=3, kind=1), op_at(1, E.OP_UPSAMPLE), [(9, 5), (4, 7)]),
    Case("f16-sep-v1", "f16", g_sep(128, 128), has_tile(lambda t: t == 4000001, 1), T4x8),
    Case("f16-sep-v2", "f16", g_sep(64, 128, 2), has_tile(lambda t: t == 4000002, 1), [(9, 17), (6, 14)]),
    Case("f16-sep-v3", "f16", g_sep(128, 256, 2), has_tile(lambda t: t == 4000003, 1), [(9, 17), (6, 14)]),
    Case("f16-sep-v4", "f16", g_sep(256, 256), has_tile(lambda t: t == 4000004, 1), T4x8),
    Case("f16-sep-v5", "f16", g_sep(256, 512), has_tile(lambda t: t == 4000005, 1), T4x8),
    Case("f16-sep-v6-dil2", "f16", g_sep(512, 512, 1, 2), has_tile(lambda t: t == 4000006, 1), T4x8),
    Case("f16-sep-v7", "f16", g_sep(32, 64), has_tile(lambda t: t == 4000007, 1), T4x8),
    Case("f16-sep-v7-40ch", "f16", g_sep(32, 40), has_tile(lambda t: t == 4000007, 1), T4x8),
    Case("f16-sep-pair", "f16", g_seppair, has_tile(lambda t: t == 4000020, 1), [(9, 17), (6, 14)]),
    Case("f16-sep-512-tail-leaky", "f16", g_sep(512, 512, act=E.ACT_LEAKY), has_tile(lambda t: t in (4000005, 4000006), 1), T4x8),
    Case("f16-sep-512-tail-relu6", "f16", g_sep(384, 512, act=E.ACT_RELU6), has_tile(lambda t: t in (4000005, 4000006), 1), T4x8),
    Case("f16-sep-512-tail-prelu", "f16", g_sep(256, 512, act=E.ACT_PRELU), has_tile(lambda t: t in (4000005, 4000006), 1), T4x8),
] + [
    Case(f"f16-chain-{v}", "f16", g_chain(v, E.ACT_RELU6 if v == "pair_res2" else E.ACT_RELU), has_tile(lambda t: 7000000 <= t < 8000000, 1), T8x12)
    for v in ("pair", "pair_res1", "pair_res2", "block", "block_nores")
] + [
    Case(f"f16-bneck-{m}-{mr}-{'front' if front else 'nofront'}", "f16", g_bneck(m, mr, front),
         has_tile(lambda t, code=9000000 + 1000 * (m // 64) + 10 * (mr // 64) + int(front): t == code, 1), T8x12, tol=dict(rel=3e-3))
    for m, mr, front in ((64, 64, True), (64, 0, True), (64, 64, False), (128, 128, True), (128, 128, False))
] + [
    Case(f"f16-bneck-proj-{mr}-{own}", "f16", g_bneck_proj(mr, own),
         has_tile(lambda t, code=9000000 + 1000 + (300 if own else 100) + 10 * (mr // 64) + (0 if own is None else 1): t == code, 1), T8x12,
         tol=dict(rel=4e-3, abs_=2e-3))
    for mr, own in ((64, True), (0, True), (128, False), (64, None))
] + [
    Case("f16-head-19", "f16", g_head16(128, 19), has_tile(lambda t: t == 6000128, 1), GEMM16),
    Case("f16-head-38", "f16", g_head16(128, 38), has_tile(lambda t: t == 6000128, 1), GEMM16),
    Case("f16-head-k64-64", "f16", g_head16(64, 64), has_tile(lambda t: t == 6000064, 1), GEMM16),
    # ---- fp32 / split fp32 (odd H: the separator row exists)
    Case("f32-first", "f32", g_first(32, 3), op_at(0, E.OP_CONV), _around(16, 32)),
    Case("f32-first-7x7-20ch", "f32", g_first(20, 7, 2, act=E.ACT_LEAKY, p=3), op_at(0, E.OP_CONV), [(33, 65), (29, 61)]),
    Case("f32s-first", "f32s", g_first(24, 3), op_at(0, E.OP_CONV), _around(16, 32)),
    Case("f32-conv32-64x64-rows", "f32", g_dense(64, 128, 1), tile_at(1, lambda r: r["tile"] == 32464064), GEMM32, env=dict(HP_C32_WK="0")),
    Case("f32-conv32-strided-3x3", "f32", g_dense(64, 96, 3, stride=2), tile_at(1, lambda r: 32000000 <= r["tile"] < 33000000), [(17, 29), (13, 17)]),
    Case("f32-conv32-19ch-unaligned-k", "f32", g_dense(96, 19, 5, act=E.ACT_NONE), tile_at(1, lambda r: 32000000 <= r["tile"] < 33000000), GEMM32),
    Case("f32-conv32-19ch-residual-of-32", "f32", g_dense(96, 19, 5, act=E.ACT_NONE, res="after", res_c=32), tile_at(2, lambda r: r["tile"] == 32464064), GEMM32),
    Case("f32-conv32-lane-epilogue", "f32", g_dense(64, 70, 1, act=E.ACT_PRELU), tile_at(1, lambda r: r["tile"] == 32064064), GEMM32,
         env=dict(HP_C32_WK="0", HP_LANE_EPILOGUE="1")),
    Case("f32-conv32-64x160", "f32", g_dense(64, 128, 1, res="before"), tile_at(2, lambda r: r["tile"] == 32064160), GEMM32, env=dict(HP_C32_BN160="1", HP_C32_WK="0")),
    Case("f32-conv32-whole-k-64", "f32", g_dense(64, 128, 1, res="before", act=E.ACT_RELU6), tile_at(2, lambda r: r["tile"] // 1000 == 39064), GEMM32, env=dict(HP_C32_WK="1")),
    Case("f32-conv32-whole-k-32-70ch", "f32", g_dense(32, 70, 1, act=E.ACT_LEAKY), tile_at(1, lambda r: r["tile"] // 1000 == 39032), GEMM32, env=dict(HP_C32_WK="1")),
    Case("f32-direct-3x3", "f32", g_dense(64, 96, 3), tile_at(1, lambda r: r["tile"] // 1000 == 34003), T8x8, env=dict(HP_NO_WINOGRAD32="1")),
    Case("f32-direct-1x1-38ch", "f32", g_dense(128, 38, 1, act=E.ACT_NONE), tile_at(1, lambda r: r["tile"] // 1000 == 34001), T8x8),
    Case("f32s-split-3x3", "f32s", g_dense(64, 128, 3), tile_at(1, lambda r: r["tile"] // 1000 == 33003), T8x8),
    Case("f32s-split-1x1-512", "f32s", g_dense(128, 512, 1), tile_at(1, lambda r: r["tile"] // 1000 == 33001), T8x8),
    Case("f32s-split-1x1-19ch", "f32s", g_dense(64, 19, 1, act=E.ACT_NONE), tile_at(1, lambda r: r["tile"] // 1000 == 33001), T8x8),
    Case("f32-dwfused-dil1", "f32", g_sep32(64, 128, 1), has_tile(lambda t: t // 1000 == 34101, 1), T8x8, env=dict(HP_FUSE32="1")),
    Case("f32-dwfused-dil2", "f32", g_sep32(128, 64, 2), has_tile(lambda t: t // 1000 == 34201, 1), T8x8, env=dict(HP_FUSE32="1")),
    Case("f32s-dwfused-dil1", "f32s", g_sep32(64, 128, 1), has_tile(lambda t: t // 1000 == 33101, 1), T8x8),
    Case("f32s-dwfused-dil2-512", "f32s", g_sep32(128, 512, 2), has_tile(lambda t: t // 1000 == 33201, 1), T8x8),
    # Winograd F(2 x 2): 17 rows -> the rows form, 15 -> per image, 7 -> the tall form, HP_WINO_NC=1 -> 8 x 8 blocks.  Every form reports tile
    # 35003004: which form a size takes rests on reading launch_conv32_winograd (T >= 4 nc, rows_y, tall_y), not on an assertion
    Case("f32-winograd", "f32", g_dense(48, 96, 3, act=E.ACT_LEAKY), tile_at(1, lambda r: r["tile"] == 35003004), [(17, 9), (15, 7), (7, 9)]),
    Case("f32-winograd-residual-70ch", "f32", g_dense(64, 70, 3, res="before"), tile_at(2, lambda r: r["tile"] == 35003004), [(17, 9), (15, 7), (7, 9)]),
    Case("f32-winograd-small-blocks", "f32", g_dense(48, 96, 3), tile_at(1, lambda r: r["tile"] == 35003004), [(17, 9), (9, 7), (7, 9)], env=dict(HP_WINO_NC="1")),
    Case("f32-winograd-per-image", "f32", g_dense(48, 96, 3), tile_at(1, lambda r: r["tile"] == 35003004), [(17, 9), (7, 7)], env=dict(HP_WINO_TALL="0")),
    Case("f32-depthwise-px1", "f32", g_simple(E.OP_DWCONV, 32, 3, act=E.ACT_RELU6), op_at(1, E.OP_DWCONV), _around(8, 8), env=dict(HP_DW32_PX="1")),
    Case("f32-depthwise-px2", "f32", g_simple(E.OP_DWCONV, 32, 3, act=E.ACT_LEAKY), op_at(1, E.OP_DWCONV), _around(8, 8), env=dict(HP_DW32_PX="2")),
    Case("f32-depthwise-px2-dil2", "f32", g_simple(E.OP_DWCONV, 40, 3, dil=2, act=E.ACT_RELU), op_at(1, E.OP_DWCONV), _around(8, 8), env=dict(HP_DW32_PX="2")),
    Case("f32-depthwise-stride2", "f32", g_simple(E.OP_DWCONV, 32, 3, stride=2, act=E.ACT_RELU6), op_at(1, E.OP_DWCONV), [(17, 17), (13, 14)]),
    Case("f32-maxpool-3-2", "f32", g_simple(E.OP_MAXPOOL, 32, 3, stride=2), op_at(1, E.OP_MAXPOOL), [(17, 17), (13, 14)]),
    Case("f32-maxpool-2-2", "f32", g_simple(E.OP_MAXPOOL, 24, 2, stride=2), op_at(1, E.OP_MAXPOOL), [(18, 17), (14, 14)]),
    Case("f32-upsample-nearest", "f32", g_simple(E.OP_UPSAMPLE, 32, 1, stride=3, kind=0), op_at(1, E.OP_UPSAMPLE), [(3, 5), (5, 7)]),
    Case("f32-upsample-bilinear", "f32", g_simple(E.OP_UPSAMPLE, 24, 1, stride=3, kind=1), op_at(1, E.OP_UPSAMPLE), [(3, 5), (5, 7)]),
    Case("f32-head32-single", "f32", g_head32(128, False), has_tile(lambda t: t == 37000000 + 12800 + 19, 1), GEMM32),
    Case("f32-head32-pair", "f32", g_head32(512, True), has_tile(lambda t: t // 1000000 == 37, 2), GEMM32),
    Case("f32-head32-two-launches", "f32", g_head32(256, True), has_tile(lambda t: t // 1000000 == 37, 2), GEMM32, env=dict(HP_HEAD_PAIR="0")),
    # ---- int8
    Case("i8-conv-1x1", "i8", g_i8(64, 128, 1), tile_at(1, lambda r: 8000000 <= r["tile"] < 8900000), GEMM16),
    Case("i8-conv-3x3-38ch", "i8", g_i8(96, 38, 3), tile_at(1, lambda r: 8000000 <= r["tile"] < 8900000), GEMM16),
    Case("i8-direct-3x3", "i8", g_i8(128, 128, 3), tile_at(1, lambda r: r["tile"] == 8900003), T16x12),
    Case("i8-direct-7x7", "i8", g_i8(128, 128, 7), tile_at(1, lambda r: r["tile"] == 8900007), T16x12),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _make(case, h, w, max_batch=N):
    net = Net(case.seed)
    tested, consumers = case.build(net)
    outs = [Out(f"y{i}", t, 0, c) for i, (t, c) in enumerate(consumers)]
    eng = E.Engine(net.layers, [o.c() for o in outs], net.blob(), w, h, max_batch, dtype=case.dtype)
    if case.dtype == "i8":
        eng.calibrate(_frames(4, h, w, seed=99))
    return net, tested, outs, eng


def _values(case, net, tested, outs, eng, got, frames, n):
    """Outputs and tested tensors against the oracle (int8: the tested layer against the quantization contract's emulation)."""
    if case.dtype == "i8":
        li = next(i for i, L in enumerate(net.layers) if L.out == tested[0])
        s = eng.int8_scales
        assert s[li] > 0
        v = _emulate(net.layers[li], eng.debug_tensor(net.layers[li].in_, n), net.blob(), s[li])
        _fp16_gate(eng.debug_tensor(tested[0], n), v.astype(np.float16))
        return
    f16 = case.dtype == "f16"
    ref, tens = ref_net.run(net.layers, outs, net.blob(), frames_u8=frames, match_fp16=f16, return_tensors=True)
    for b in range(n):
        for nm, arr in got[b]:
            if f16:
                _close(arr, ref[nm][b], **case.tol)
            else:
                _close32(arr, ref[nm][b], nm)
    for t in tested:
        mine = eng.debug_tensor(t, n)      # (must not be refused: a tested tensor is materialised and shares no arena buffer in these graphs)
        if f16:
            _close(mine, tens[t][:n], **case.tol)
        else:
            _close32(mine, tens[t][:n], f"tensor {t}")


@pytest.mark.parametrize("name", list(BY_NAME))
@guarded
def test_family_output_with_a_halo(hp, monkeypatch, name):
    """(a): the family's kernel ran (tile code), its tensor has a halo of >= 2 pixels, values match the oracle, and everything outside the
    interior of every tensor of the graph is zero - on every map size of the case."""
    case = BY_NAME[name]
    _set_env(monkeypatch, case.env)
    for h, w in case.sizes:
        net, tested, outs, eng = _make(case, h, w)
        frames = _frames(N, h, w, seed=h * 100 + w)
        got = eng.inference(frames)
        ids = footprint.tensor_ids(net.layers)
        for t in tested:
            g = eng.debug_raw(t)[1]
            assert g["P"] >= 2 and g["max_batch"] == N, g
            if case.dtype in ("f32", "f32s"):
                assert g["H"] % 2 == 1 and g["rows"] == g["H"] + 2 * g["P"] + 1, g      # the separator row exists
        assert footprint.assert_zero_outside(eng, ids, N, f"{name} {h}x{w}") >= len(tested)
        _values(case, net, tested, outs, eng, got, frames, N)
        rows = eng.profile(N, 1)
        assert case.want(rows), (name, h, w, [(r["layer"], r["op"], r["tile"]) for r in rows])
        assert footprint.assert_zero_outside(eng, ids, None, f"{name} {h}x{w} after profile") >= len(tested)   # (the profiler runs every step again)
        if case.differs_from:
            eng.inference(frames)
            mid = eng.debug_tensor(tested[0], N)
            _set_env(monkeypatch, {**case.env, **case.differs_from})
            eng2 = _make(case, h, w)[3]
            eng2.inference(frames)
            mid2 = eng2.debug_tensor(tested[0], N)
            _set_env(monkeypatch, case.env)
            assert case.want(eng2.profile(N, 1))
            _close(mid, mid2, **case.tol)
            assert (mid != mid2).any(), (name, h, w, case.differs_from, "the two engines ran the same arithmetic")
            eng2.close()
        eng.close()


# ---------------------------------------------------------------- (b) unaligned concat slices, written right to left
SLICES = [(0, 32), (32, 19), (51, 38), (89, 39)]


def _concat_graph(kind, residual):
    """cat = [32 | 19 | 38 | 39], every slice written AFTER its right neighbour: 39 at 89 (a plain 1 x 1), then the producers under test - 38
    channels at 51, then 19 at 32 - then 32 at 0 (a plain 1 x 1).  Whatever a producer spills to the right lands in a slice that nobody
    writes again and that is compared with the oracle.  `residual`: the producers under test add a residual before the activation (a
    layer's residual is read from channel 0 of its tensor: the layer description has no residual channel offset, so the residual's own
    slice cannot be unaligned - the output slice it is added into is).  Returns the net, cat, the outputs and the tested layers' range."""
    net = Net(23)
    cin = 128 if kind in ("head16", "head32") else 96 if kind == "k5" else 64
    t0 = net.conv(0, 3, cin, 3, 1)
    cat = net.new_tensor()
    other = net.new_tensor()
    if residual:
        net.conv(t0, cin, 38, 1, out=other, out_coff=0, act=E.ACT_NONE)
    net.conv(t0, cin, 39, 1, out=cat, out_coff=89, act=E.ACT_LEAKY, act_param=0.1)
    first_tested = len(net.layers)
    for cout, coff in ((38, 51), (19, 32)):
        res = dict(res=other, res_before_act=1) if residual else {}
        if kind in ("head16", "head32"):
            hid = net.conv(t0, cin, 512, 1, act=E.ACT_RELU)
            net.conv(hid, 512, cout, 1, act=E.ACT_NONE, out=cat, out_coff=coff)
        else:
            net.conv(t0, cin, cout, int(kind[1]), act=E.ACT_NONE, out=cat, out_coff=coff, **res)
    end_tested = len(net.layers)
    net.conv(t0, cin, 32, 1, out=cat, out_coff=0)
    y = net.conv(cat, 128, 8, 3, dil=2, act=E.ACT_NONE)
    outs = [Out(f"s{coff}", cat, coff, c, scale=2.0) for coff, c in SLICES] + [Out("y", y, 0, 8)]
    return net, cat, outs, (first_tested, end_tested)


# (dtype, producer, environment, with a residual, the exact tile code of the producers under test, profile rows they take).  The two fp16
# heads read the same tensor and share ONE launch (mlp_head_kernel's paired form) unless HP_NO_PAIR_HEADS=1.  fp32, at 3 x 9 x 11 pixels and 64
# padded outputs: 5 x 5 on 96 channels -> conv32_kernel<64, 64> with the row epilogue (32464064), 1 x 1 on 64 channels -> conv32_direct_kernel
# with one wavefront group (34001001; HP_NO_WINOGRAD32=1: 3 x 3 -> 34003001), 3 x 3 -> Winograd (35003004); the split engine: 33003001 / 33001001
is_ = lambda code: (lambda t: t == code)
CONCAT = [
    ("f16", "k3", {}, False, generic16, 2), ("f16", "k1", {}, False, generic16, 2), ("f16", "k3", {}, True, generic16, 2),
    ("f16", "head16", {}, False, is_(6000128), 1), ("f16", "head16", dict(HP_NO_PAIR_HEADS="1"), False, is_(6000128), 2),
    ("f32", "k5", {}, False, is_(32464064), 2), ("f32", "k5", {}, True, is_(32464064), 2),
    ("f32", "k1", {}, False, is_(34001001), 2), ("f32", "k1", {}, True, is_(34001001), 2),
    ("f32", "k3", dict(HP_NO_WINOGRAD32="1"), False, is_(34003001), 2), ("f32", "k3", dict(HP_NO_WINOGRAD32="1"), True, is_(34003001), 2),
    ("f32", "k3", {}, False, is_(35003004), 2), ("f32", "k3", {}, True, is_(35003004), 2),
    ("f32", "head32", {}, False, lambda t: t in (37051219, 37051238), 2),
    ("f32s", "k3", {}, True, is_(33003001), 2), ("f32s", "k1", {}, False, is_(33001001), 2),
    ("i8", "k3", {}, False, lambda t: 8000000 <= t < 8900000, 2), ("i8", "k1", {}, False, lambda t: 8000000 <= t < 8900000, 2),
]


@pytest.mark.parametrize("dtype,kind,env,residual,pred,launches", CONCAT, ids=[f"{c[0]}-{c[1]}{'-res' if c[3] else ''}{'-' + '-'.join(c[2]) if c[2] else ''}" for c in CONCAT])
@guarded
def test_unaligned_concat_slices_written_right_to_left(hp, monkeypatch, dtype, kind, env, residual, pred, launches):
    _set_env(monkeypatch, env)
    h, w = 9, 11
    net, cat, outs, (first_tested, end_tested) = _concat_graph(kind, residual)
    eng = E.Engine(net.layers, [o.c() for o in outs], net.blob(), w, h, N, dtype=dtype)
    frames = _frames(N, h, w, seed=5)
    f16 = dtype in ("f16", "i8")
    if dtype == "i8":
        eng.calibrate(_frames(4, h, w, seed=99))
    got = eng.inference(frames)
    footprint.assert_zero_outside(eng, footprint.tensor_ids(net.layers), N, f"concat {dtype} {kind}")
    g = eng.debug_raw(cat)[1]
    assert (g["C"], g["cs"], g["P"]) == (128, 128, 2)
    raw = eng.debug_raw(cat)[0]
    stored = raw[:, 2:2 + h, 2:2 + w, :].transpose(0, 3, 1, 2).astype(np.float32)
    if dtype == "i8":
        # every slice's stored values against the emulation of its LAST writer (the quantization contract), slice by slice
        s = eng.int8_scales
        x = eng.debug_tensor(net.layers[0].out, N)
        last = {L.out_coff: i for i, L in enumerate(net.layers) if L.out == cat}
        for coff, c in SLICES:
            li = last[coff]
            assert s[li] > 0
            _fp16_gate(stored[:, coff:coff + c], _emulate(net.layers[li], x, net.blob(), s[li]).astype(np.float16))
    else:
        ref = ref_net.run(net.layers, outs, net.blob(), frames_u8=frames, match_fp16=f16)
        for b in range(N):
            for nm, arr in got[b]:
                (_close if f16 else _close32)(arr, ref[nm][b])
        for coff, c in SLICES:   # the exported slices are the buffer's own channels (x 2)
            exported = np.stack([dict(gb)[f"s{coff}"] for gb in got])
            assert np.array_equal(exported, 2 * stored[:, coff:coff + c]), coff
    rows = eng.profile(N, 1)
    mine = [r["tile"] for r in rows if first_tested <= r["layer"] < end_tested]
    assert sum(bool(pred(t)) for t in mine) == launches and len(mine) == launches, [(r["layer"], r["tile"]) for r in rows]


# ---------------------------------------------------------------- (c) partial batches leave the other frames alone
PARTIAL = [("f32-winograd", (7, 9), 1), ("f32-winograd", (7, 9), 2), ("f32-winograd", (17, 9), 1), ("f32-winograd", (17, 9), 2),
           ("f32-winograd-small-blocks", (7, 9), 1), ("f32-winograd-small-blocks", (7, 9), 2),
           ("f32-conv32-64x160", (9, 15), 1), ("f32-conv32-64x160", (9, 15), 2), ("f32-direct-3x3", (9, 9), 1), ("f32-direct-3x3", (9, 9), 2),
           ("f32-head32-pair", (9, 15), 1), ("f32-head32-pair", (9, 15), 2), ("f32s-dwfused-dil1", (9, 9), 1), ("f32s-dwfused-dil1", (9, 9), 2),
           ("f32s-split-3x3", (9, 9), 1), ("f32s-split-3x3", (9, 9), 2),
           ("f16-sep-v1", (5, 9), 1), ("f16-sep-pair", (9, 17), 1), ("f16-chain-block", (9, 13), 1), ("f16-bneck-64-64-front", (9, 13), 1),
           ("f16-head-19", (9, 15), 1), ("f16-sep-v5", (5, 9), 1), ("i8-conv-1x1", (9, 15), 1), ("i8-direct-3x3", (17, 13), 1)]


@pytest.mark.parametrize("name,size,conc", PARTIAL, ids=[f"{n}-{s[0]}x{s[1]}-conc{c}" for n, s, c in PARTIAL])
@guarded
def test_partial_batches_leave_other_frames_alone(hp, monkeypatch, name, size, conc):
    case = BY_NAME[name]
    _set_env(monkeypatch, case.env)
    h, w = size
    net, tested, outs, eng = _make(case, h, w, max_batch=4)
    if conc == 2:
        eng.set_concurrency(2)
        assert eng.concurrency == 2
    ids = footprint.tensor_ids(net.layers)
    A, B = _frames(4, h, w, seed=1), _frames(4, h, w, seed=2)
    first = eng.inference(A)
    assert case.want(eng.profile(4, 1))
    first = eng.inference(A)                      # (the profiler ran the steps on its own input)
    snap = footprint.snapshot_frames(eng, ids, 1)
    assert set(tested) <= set(snap[1])
    for n in (1, 3):                              # (after n = 3 only frame 3 is still A's: the snapshot's last frame)
        eng.inference(B[:n])
        footprint.assert_frames_unchanged(eng, snap, n, f"{name} n={n}")
        footprint.assert_zero_outside(eng, ids, n, f"{name} n={n}")
    again = eng.inference(A)
    for b in range(4):
        for (nm, x), (_, y) in zip(first[b], again[b]):
            assert np.array_equal(x, y), (nm, b)


# ---------------------------------------------------------------- (d) whole small networks, arena included
ARCHS = ["lw_openpose_mobilenet", "lw_openpose_vggtiny", "openpose_vgg19", "pose_proposal_resnet50", "pifpaf_resnet50"]


@pytest.mark.parametrize("dtype", ["f16", "f32", "f32s", "i8"])
@pytest.mark.parametrize("arch", ARCHS)
@guarded
def test_whole_small_networks_stay_zero_outside(hp, monkeypatch, arch, dtype):
    _set_env(monkeypatch, {})
    w_, h_ = (97, 97) if arch.startswith("pifpaf") else (160, 128) if arch.startswith("pose_proposal") else (96, 80)
    m = E.Model(arch, w_, h_)
    eng = E.Engine.from_model(m, m.init_weights(3), max_batch=3, dtype=dtype)
    fr = synth.images_u8(synth.rng_for(8), 3, h_, w_)
    if dtype == "i8":
        eng.calibrate(fr)
    assert not footprint.too_large(eng)
    ids = footprint.tensor_ids(m.layers)
    first = eng.inference(fr[:2])
    seen = footprint.assert_zero_outside(eng, ids, 2, f"{arch} {dtype} n=2")
    assert seen >= 3
    snap = footprint.snapshot_frames(eng, ids, 1)
    eng.inference(fr[2:3])
    footprint.assert_frames_unchanged(eng, snap, 1, f"{arch} {dtype}")
    footprint.assert_zero_outside(eng, ids, 1, f"{arch} {dtype} n=1")
    eng.inference(fr)
    footprint.assert_zero_outside(eng, ids, 3, f"{arch} {dtype} n=3")
    if dtype in ("f32", "f32s"):
        info = eng.arena_info
        assert info["tensors"] > info["buffers"] >= 1     # buffers are shared: the raw tap shows them through every tenant
    third = eng.inference(fr[:2])
    for b in range(2):
        for (nm, x), (_, y) in zip(first[b], third[b]):
            assert np.array_equal(x, y), (nm, b)
