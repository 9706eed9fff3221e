// conv_pick.hpp — which kernel serves a dense fp16 convolution, decided ONCE, as pure host code: no device code and no HIP runtime
// call, so the decision runs in a plain host program (tests/cpp/conv_pick.cpp).  The engine packs the weights by conv_weight_layout,
// labels profile rows by conv_mfma_tile, sizes the split-K scratch by conv_splitk and launches through launch_conv_mfma
// (conv_kernels.hpp, defined in conv_kernels.hip): all four read the one conv_choice that pick_conv returns.
#pragma once
#include "conv_kernels.hpp"

namespace hp {

enum conv_form : int {
    CONV_GEMM,     // conv_mfma_kernel<BM, BN, BK, EPI>: any geometry, weights in rows (w_layout 0)
    CONV_HALO,     // conv3x3_direct_kernel<CIN, 16>: 3x3 / stride 1 with 64 or 128 input channels
    CONV_DIRECT,   // conv_direct_kernel<KS, CK, NBUF> (+ conv_direct_finish_kernel<KS, CK> when split): square 3 / 5 / 7, chunked Cin
    CONV_SMALL1X1, // conv1x1_small_kernel<KP>
    CONV_BIG1X1,   // conv1x1_big_kernel<TM, NTP>
};

struct conv_choice {
    conv_form form;
    // false: fragment-ordered weights (w_layout 1) were asked for a geometry that has no fragment-order form; `form` is then where the
    // cascade ended and the launcher returns hipErrorInvalidValue
    bool ok;
    int BM, BN, BK, EPI;       // CONV_GEMM (EPI 0: the fast epilogue, 1: the generic one)
    int CIN;                   // CONV_HALO
    int KS, CK, NBUF, nchunks; // CONV_DIRECT (nchunks = Cin / CK)
    int KP;                    // CONV_SMALL1X1
    int TM, NTP;               // CONV_BIG1X1 (0, 0: not a pixel-block GEMM; never ok)
    int ksplit;                // CONV_DIRECT <3, 64, 2> on maps whose tiles leave CUs idle: 2 or 4 blocks share a tile's chunks; else 1
    size_t scratch_bytes;      // the fp32 partial sums of that split (0 when ksplit == 1)

    // the profile rows' code: BM*1000+BN for the generic implicit GEMM, 5064192 conv3x3_direct_kernel, 51xxxxx conv1x1_small_kernel,
    // 52xxxxx conv1x1_big_kernel<TM, NTP>, 6xxxxxx conv_direct_kernel
    int tile;
};

// fast epilogue (aligned fp16 NHWC vectors) when every 8-channel chunk is whole and 16-byte aligned
inline bool fast_epilogue(const conv_params& p)
{
    return p.out.p && !p.out_f32 && p.Cout % 8 == 0 && p.out.coff % 8 == 0 && p.out.cs % 8 == 0
        && (!p.res.p || (p.res.coff % 8 == 0 && p.res.cs % 8 == 0));
}

// conv_direct_kernel (8 wavefronts, 128 output channels x 16x12 pixels per block, any square kernel / chunked Cin) serves this layer:
// 0 = no, otherwise the channel chunk CK (128 or 64).
inline int use_gdirect(const conv_params& p)
{
    if (p.KH != p.KW || (p.KH != 3 && p.KH != 5 && p.KH != 7) || p.stride != 1 || p.dil != 1 || p.pad_t != p.KH / 2
        || p.pad_l != p.KH / 2 || p.OH != p.H || p.OW != p.W || p.Cin % 64 || p.Cout_pad % 128 || p.in.coff % 8 || !fast_epilogue(p))
        return 0;
    if (p.KH == 3 && p.Cin <= 128)
        return 0; // (these stay with conv3x3_direct_kernel, whose half-size blocks share a CU at batch 8)
    // maps smaller than two tiles: the generic implicit GEMM packs pixels of several images into one tile - worth more than the halo
    // re-use unless K is long (measured at 12 x 12: 512 -> 512 57 -> 45 us, 2048 -> 512 212 -> 163 us on this kernel)
    if ((long)p.OH * p.OW < 256 && p.Cin < 256)
        return 0;
    // 3x3 on maps the 16 x 12 tiles cover badly (49 x 49: 20 tiles for 12.5 tiles of pixels, 25 x 25: 6 for 3.3): the generic kernel has no
    // tiles to round up to (measured at batch 64: 256 channels at 49 x 49 253 -> 223 us, 512 channels at 25 x 25 276 -> 220 us)
    if (p.KH == 3 && (double)p.OH * p.OW < 0.68 * ((p.OH + 15) / 16 * 16) * ((p.OW + 11) / 12 * 12))
        return 0;
    // 128-channel chunks only where ONE chunk is the whole input (7x7 / 5x5 x 128: a 101 / 82 KB tile, single-buffered); everything
    // else runs on double-buffered 64-channel chunks (the 128-channel form of that pipeline needs more than 256 registers)
    // (measured: 7x7 x 128 as two pipelined 64-channel chunks is 10 % slower than as one 128-channel chunk - the chunk barrier waits for
    // the wavefronts that lose the matrix-pipe arbitration)
    return p.Cin == 128 ? 128 : 64;
}

inline bool use_halo(const conv_params& p)
{
    return p.KH == 3 && p.KW == 3 && p.stride == 1 && p.dil == 1 && p.pad_t == 1 && p.pad_l == 1 && (p.Cin == 128 || p.Cin == 64)
        && p.Cout_pad % 64 == 0 && p.in.coff % 8 == 0;
}

// which (TM, NTP) the pixel-block GEMM runs a layer with: TM * 1000 + NTP, or 0 when the layer is not its kind
inline int big1x1_variant(const conv_params& p)
{
    // (any stride: a strided 1x1 is the same GEMM over every stride-th pixel - the producers gather them; ResNet's projection shortcuts)
    if (p.KH != 1 || p.KW != 1 || p.stride < 1 || p.pad_t || p.pad_l || p.OH != (p.H + p.stride - 1) / p.stride
        || p.OW != (p.W + p.stride - 1) / p.stride || p.Cin % 256 /* four-chunk ring */ || p.Cout_pad % 128 || p.Cout % 8 || p.in.coff % 8
        || p.in.cs - p.in.coff < p.Cin)
        return 0;
    // (TM, NTP) by a small cost model: blocks are dealt to the 256 CUs in rounds (two blocks share a CU when each needs <= 256
    // registers); a round costs its MFMAs at ~80 % pipe efficiency plus ~6 k cycles of prologue / epilogue; 64-pixel blocks (NTP = 2)
    // pull twice the weights per MFMA through the texture path
    // (TM, NTP): measured over the ResNet-50 bottlenecks at 193^2 .. 12^2 pixels and LW-OpenPose's pointwise layers (sweep of all
    // instances, tools/profile_layers.py): 64 pixels x 256 output channels wins or ties almost everywhere - 118 registers and 72 KB
    // of LDS let TWO blocks share a CU, so one block's prologue (first chunk from HBM) and epilogue (stores) sit under the other's
    // MFMAs; wider or taller blocks run alone on their CU and pay both phases in full.  128-row blocks where the output has no
    // 256-row groups.
    // ... except where that grid is barely more than one block per CU (ResNet's reductions on 24 x 24 / 12 x 12 maps at batch 32: 288 / 144
    // blocks): 128-row blocks halve the last, nearly empty round (25.5 -> 21.4 us, 22.8 -> 19.2 us; a higher threshold loses with two streams)
    if (p.Cout_pad % 256 == 0 && (long)((p.npix + 63) / 64) * (p.Cout_pad / 256) < 320)
        return 1002;
    if (p.Cout_pad % 256 == 0)
        return 2002;
    const long blocks4 = (long)((p.npix + 127) / 128) * (p.Cout_pad / 128);
    return blocks4 >= 1024 ? 1004 : 1002;
}

inline bool use_small1x1(const conv_params& p)
{
    return p.KH == 1 && p.KW == 1 && p.stride == 1 && p.Cout_pad % 128 == 0 && p.Cout_pad <= 512
        && (p.Cout_pad == 128 || p.Cin <= 128) // (wider outputs only where the layer is HBM-bound: K <= 128)
        && (p.Cin == 64 || p.Cin == 128 || p.Cin == 192 || p.Cin == 256)
        && p.in.coff % 8 == 0 && p.in.cs - p.in.coff >= p.Cin && p.OH == p.H && p.OW == p.W;
}

// The cascade: small 1x1, big 1x1, chunked direct, 3x3 halo for fragment-ordered weights (w_layout 1), the generic GEMM for rows
// (w_layout 0 - also how tests and tools force it).  Every field of p but w_layout, ksplit and splitk is read.
inline conv_choice pick_conv(const conv_params& p, int w_layout)
{
    conv_choice c{};
    c.ksplit = 1;
    if (w_layout != 1) {
        c.form = CONV_GEMM, c.ok = true;
        c.BM = (p.Cout_pad % 128 == 0) ? 128 : 64;
        // prefer the 128-pixel tile only when it still fills the 256 CUs at least once
        const long blocks128 = (long)((p.npix + 127) / 128) * (p.Cout_pad / c.BM);
        c.BN = blocks128 >= 256 ? 128 : 64;
        c.BK = p.Cin % 64 == 0 ? 64 : 32;
        c.EPI = fast_epilogue(p) ? 0 : 1;
        c.tile = c.BM * 1000 + c.BN;
    } else if (p.KH == 1 && use_small1x1(p)) {
        c.form = CONV_SMALL1X1, c.ok = fast_epilogue(p);
        c.KP = p.Cin, c.tile = 5100000 + c.KP;
    } else if (p.KH == 1) {
        const int v = big1x1_variant(p);
        c.form = CONV_BIG1X1, c.ok = v && fast_epilogue(p);
        c.TM = v / 1000, c.NTP = v % 1000, c.tile = 5200000 + v;
    } else if (const int ck = use_gdirect(p)) {
        c.form = CONV_DIRECT, c.ok = true;
        c.KS = p.KH, c.CK = ck, c.nchunks = p.Cin / ck;
        c.NBUF = ck == 128 || (p.KH == 3 && c.nchunks == 1) ? 1 : 2;
        c.tile = 6000000 + p.Cin * 1000 + p.KH * p.KW;
        // split-K for the chunk-pipelined 3x3 instance when its tiles leave CUs idle (configs[3]: 12 x 12 maps at batch 32 = 32 tiles x 4
        // output-channel groups = 128 blocks; the 2048 -> 512 head convolution alone is 8 % of that network's conv time)
        if (p.KH == 3 && ck == 64) {
            const long blocks = (long)((p.OW + 11) / 12) * ((p.OH + 15) / 16) * p.B * (p.Cout_pad / 128);
            if (blocks <= 64 && c.nchunks >= 8 && c.nchunks % 4 == 0)
                c.ksplit = 4;
            else if (blocks <= 160 && c.nchunks >= 4 && c.nchunks % 2 == 0)
                c.ksplit = 2;
            if (c.ksplit > 1)
                c.scratch_bytes = (size_t)c.ksplit * blocks * 8 * 3 * 4 * 64 * sizeof(float4); // [z][slot][wave][K0 = 3][4][64 lanes] float4
        }
    } else {
        c.form = CONV_HALO, c.ok = use_halo(p) && fast_epilogue(p);
        c.CIN = p.Cin == 128 ? 128 : 64, c.tile = 5000000 + 64 * 1000 + 192;
    }
    return c;
}

// What conv_weight_layout / conv_mfma_tile / conv_splitk (conv_kernels.hpp) answer: conv_kernels.hip forwards to these, so that the host
// program runs the text the engine runs.
namespace pick {
inline int weight_layout(const conv_params& p) { return pick_conv(p, 1).ok ? 1 : 0; } // 1: the geometry has a fragment-order form
inline int tile(const conv_params& p) { return pick_conv(p, p.w_layout).tile; }
inline int splitk(const conv_params& p, size_t* scratch_bytes)
{
    const conv_choice c = pick_conv(p, p.w_layout);
    if (scratch_bytes)
        *scratch_bytes = c.scratch_bytes;
    return c.ksplit;
}
} // namespace pick

} // namespace hp
