// conv32_pick.hpp — which kernel, which template instance and which grid a dense fp32 layer gets, decided ONCE, as pure host code: no device
// code, no HIP runtime call, no allocation, so the decision runs in a plain host program (tests/cpp/conv32_pick.cpp).  The engine asks
// conv32_layer_forms at build time (which weight forms a layer gets), the launchers of conv_fp32.hip / conv32_direct.hip / conv32_winograd.hip /
// conv32_head.hip carry out the conv32_choice that pick_conv32 / pick_head32 return, and the profile rows print its `tile`.
// (The first layer and the depthwise kernels keep their arithmetic in their launchers, conv_fp32.hip: it is used once.)
#pragma once
#include "conv_fp32.hpp"

namespace hp {

// ---- geometry the picker and the kernels share
constexpr int WCK = 16;                             // conv32_winograd_kernel: input channels per chunk
constexpr int WINO_BW = 8;                          // ... its block: 8 NC rows x 8 columns of pixels, NC = 2 | 1
constexpr int WINO_MW = 4;                          // ... four wavefronts (16-channel MFMA tiles) per block, the pipelined form
constexpr int WINO_LDS[3] = { 0, 40960, 77824 };    // ... dynamic LDS by NC (wino_geom<4, NC>::PLDS_BYTES: conv32_winograd.hip asserts it)
constexpr int DIRECT_T = 8;                         // conv32_direct_kernel: a block's 8 x 8 pixel tile
constexpr int HK1 = 128;                            // conv32_head_kernel: input channels
constexpr int HEAD_PX = 32;                         // ... pixels per block

template <bool SPLIT, int KS, int CK, int MW, int DWD = 0>
struct direct32_geom {
    static constexpr int HP = DIRECT_T + KS - 1;                   // halo tile is HP x HP pixels
    static constexpr int PBU = CK / 4 + 1;                         // 16-byte units per halo pixel: CK elements of 4 bytes + one unit of padding (odd)
    static constexpr int PB = PBU * 16;
    static constexpr int RP = ((HP * PBU + 7) / 16 * 16 + 8) * 16; // pixel-row pitch in bytes: >= HP pixels, = 8 mod 16 units
    static constexpr int LDS_BYTES = HP * RP;
    static constexpr int QPP = CK / 4;                             // float4 quads per pixel
    // DWD > 0 (a depthwise 3 x 3 of dilation DWD fused in front of the 1 x 1, KS = 1): the chunk's DEPTHWISE input - (8 + 2 DWD)^2 pixels x CK
    // fp32 channels in pixel rows of PB bytes - is what arrives from HBM, into a second LDS tile behind the first; the depthwise outputs are
    // computed from it into the first tile, which the MFMAs read as before.  The depthwise weights and biases of ALL chunks ([9][C] + [C]
    // floats) sit behind that, loaded once per block.
    static constexpr int XP = DWD ? DIRECT_T + 2 * DWD : HP;       // staged tile is XP x XP pixels
    static constexpr int XT_BYTES = DWD ? XP * XP * PB : 0;
    static constexpr int QUADS = XP * XP * QPP;                    // float4 quads staged per chunk
    static constexpr int TM = SPLIT ? 2 : 1, TN = SPLIT ? 2 : 1, NWN = 2 / TN; // MFMA tiles per wavefront; wavefronts side by side over the pixels
    static constexpr int SLABS = MW * NWN * (32 * (TM * 32 + 4) * 4); // the epilogue's transposition slabs (rows_geom<TM>::SLAB_BYTES per wavefront) lie over the dead tiles
    static constexpr int TILES_BYTES = LDS_BYTES + XT_BYTES;
    static constexpr int DWW_OFF = TILES_BYTES > SLABS ? TILES_BYTES : SLABS; // dynamic LDS: this + 40 bytes per depthwise channel (DWD)
    static constexpr int KQ = SPLIT ? CK / 16 : CK / 8;            // steps per tap: 32 bytes of a pixel row each
    static constexpr int SPC = KS * KS * KQ;                       // steps per chunk
    static constexpr int RING = SPC % 3 == 0 ? 3 : (SPLIT ? 2 : 4); // A-fragment ring: the step in use + one or two in flight
    static constexpr int AHEAD = RING - 1;                         // steps between an A fragment's request and its use
    // chunks in flight between HBM and LDS (registers): a 1 x 1 layer's chunk is only KQ steps of MFMAs - far shorter than an HBM round trip
    // under load - and Little's law asks for ~40 KB in flight per CU to stream at the rate the layer needs; a 3 x 3 chunk covers its successor
    static constexpr int DEPTH = KS != 1 ? 1 : DWD ? (SPLIT && MW == 8 ? 1 : 2) : (SPLIT && (MW < 4 || MW == 8) ? 2 : 3); // (fewer threads share a tile's staging when MW < 4: 16 quads per thread and chunk at MW = 1)
    static_assert(SPC % RING == 0 && SPC % 2 == 0, "ring / double buffer periods");
};

// ---- the compiled instances, as data: the launchers expand these into their dispatch, the host test asks them "does this choice exist?"
// conv32_kernel<BM, BN, WM, WN, ROWS> (both epilogues of each), conv32_t16_kernel<BN, WN>, conv32_wk_kernel<KT, BN>
#define HP_CONV32_INSTANCES(X) X(128, 128, 2, 2) X(64, 128, 1, 4) X(64, 64, 2, 2)
#define HP_CONV32_T16_INSTANCES(X) X(160, 2)
#define HP_CONV32_WK_INSTANCES(X) X(32, 64) X(64, 64)
// conv32_winograd_kernel<MW, PIPE, NC>
#define HP_CONV32_WINO_INSTANCES(X) X(4, true, 2) X(4, true, 1)
// conv32_direct_kernel<SPLIT, KS, CK, MW, DWD>.  Eight wavefront groups: the split 1 x 1 layers only, and not behind a depthwise layer of
// dilation 2 (68 spilled registers); behind a depthwise layer: 2 / 4 (split, dilation 1: 8) groups
#define HP_CONV32_DIRECT_INSTANCES(X)                                                                                     \
    X(true, 1, 64, 1, 0) X(true, 1, 64, 2, 0) X(true, 1, 64, 4, 0) X(true, 1, 64, 8, 0)                                   \
    X(true, 3, 32, 1, 0) X(true, 3, 32, 2, 0) X(true, 3, 32, 4, 0)                                                        \
    X(false, 1, 64, 1, 0) X(false, 1, 64, 2, 0) X(false, 1, 64, 4, 0)                                                     \
    X(false, 3, 32, 1, 0) X(false, 3, 32, 2, 0) X(false, 3, 32, 4, 0)                                                     \
    X(true, 1, 64, 2, 1) X(true, 1, 64, 4, 1) X(true, 1, 64, 8, 1) X(true, 1, 64, 2, 2) X(true, 1, 64, 4, 2)              \
    X(false, 1, 64, 2, 1) X(false, 1, 64, 4, 1) X(false, 1, 64, 2, 2) X(false, 1, 64, 4, 2)
// conv32_head_kernel<TM2>, conv32_head_pair_kernel<TMA, TMB>
#define HP_CONV32_HEAD_INSTANCES(X) X(1) X(2)
#define HP_CONV32_HEAD_PAIR_INSTANCES(X) X(1, 1) X(1, 2) X(2, 1) X(2, 2)

enum conv32_form : int { C32_GEMM, C32_WINO2, C32_DIRECT }; // what a dense layer can be launched as (engine.cpp: launch_kind)
enum conv32_kern : int { K32_CONV, K32_T16, K32_WK, K32_WINO2, K32_DIRECT, K32_HEAD, K32_HEAD_PAIR };

struct conv32_choice {
    bool ok; // false: the form does not take this layer, or no compiled instance does - the launcher returns hipErrorInvalidValue
    conv32_kern kernel;
    // the kernel's template arguments, in its parameter list's order: conv32_kernel BM BN WM WN ROWS; conv32_t16_kernel BN WN; conv32_wk_kernel KT BN;
    // conv32_winograd_kernel MW PIPE NC; conv32_direct_kernel SPLIT KS CK MW DWD; conv32_head_kernel TM2; conv32_head_pair_kernel TMA TMB
    int targ[5];
    unsigned grid_x, grid_y;
    int threads;
    size_t lds;                    // dynamic LDS bytes
    int tiles_x, tiles_y, vh, rows; // the kernel arguments behind the parameter struct (Winograd and direct kernels)
    // the profile rows' code: 32000000 + 400000 (row-major epilogue) + BM * 1000 + BN conv32_kernel / conv32_t16_kernel; 39000000 + Cin * 1000 +
    // pixels per block conv32_wk_kernel; 33000000 (split) / 34000000 (fp32) + 100000 * fused depthwise dilation + KS * 1000 + wavefront groups per
    // block conv32_direct_kernel; 35003004 the Winograd F(2 x 2) kernel; 37000000 + 100 * HID + C2 the two-layer heads
    int tile;
};

namespace pick32 {

// 3 x 3, stride 1, dilation 1, SAME padding, input slice readable in whole WCK-channel chunks, NHWC output only (a network head
// keeps the direct kernel's lane = pixel epilogue for its NCHW copy)
inline bool winograd_ok(const conv32_params& p)
{
    return p.KH == 3 && p.KW == 3 && p.stride == 1 && p.dil == 1 && p.Cin % WCK == 0 && p.Cout_pad % 64 == 0 && p.OH == p.H && p.OW == p.W && p.pad_t == 1
        && p.pad_l == 1 && !p.out_f32 && p.out.p;
}

// the direct kernels' channel chunk: 64 channels at 1 x 1, 32 at 3 x 3 (what conv32_split_pack / conv32_frag_pack lay the weights out in)
inline int direct_chunk(int taps) { return taps == 1 ? 64 : 32; }

// Which layers the direct kernels take: square 1 x 1 / 3 x 3, stride 1, dilation 1, SAME padding, channel slice readable in whole chunks
// (32 channels at 3 x 3, 64 at 1 x 1).
inline bool direct_ok(const conv32_params& p)
{
    return p.KH == p.KW && (p.KH == 1 || p.KH == 3) && p.Cin % direct_chunk(p.KH * p.KW) == 0 && p.stride == 1 && p.dil == 1 && p.Cout_pad % 64 == 0
        && p.OH == p.H && p.OW == p.W && p.pad_t == (p.KH - 1) / 2 && p.pad_l == (p.KW - 1) / 2;
}

// Wavefront groups per block.  All wavefronts of a block share one 8 x 8 pixel tile, so more of them amortise the tile's staging over more
// output channels - but a layer needs enough blocks for 256 CUs.  SPLIT: MW wavefronts of 64 channels; fp32: MW x 2 wavefronts, 32 MW channels.
// dwd = dilation of a depthwise 3 x 3 fused in front (0: none).  The fused forms exist for 2 / 4 (and, split at dilation 1, 8) groups only: a
// fused layer takes the largest of those that still leaves enough blocks, 2 at least; 0 = no fused form fits (odd group count).
inline int direct_mw(const conv32_params& p, bool split, int dwd)
{
    const int groups = p.Cout_pad / (split ? 64 : 32);
    const long tiles = (long)p.B * ((p.OH + DIRECT_T - 1) / DIRECT_T) * ((p.OW + DIRECT_T - 1) / DIRECT_T);
    for (int mw : { 8, 4, 2, 1 }) {
        if (mw == 8 && (!split || p.KH != 1 || dwd == 2))
            continue; // (8 wavefronts of 64 channels: the split 1 x 1 layers with 512 outputs read their input tile once; behind a depthwise layer of dilation 2: 68 spilled registers - not compiled)
        if (dwd && mw == 1)
            break;
        if (groups % mw == 0 && (mw == 1 || (dwd && mw == 2) || tiles * (groups / mw) >= (split ? 256 : 640)))
            return mw;
    }
    return dwd ? 0 : 1;
}

// DWW_OFF of the compiled instance <split, ks, direct_chunk, mw, dwd>, or -1: there is none
inline long direct_lds(bool split, int ks, int mw, int dwd)
{
#define HP_X(SPLIT_, KS_, CK_, MW_, DWD_)                        \
    if (split == SPLIT_ && ks == KS_ && mw == MW_ && dwd == DWD_) \
        return direct32_geom<SPLIT_, KS_, CK_, MW_, DWD_>::DWW_OFF;
    HP_CONV32_DIRECT_INSTANCES(HP_X)
#undef HP_X
    return -1;
}

// The depthwise-fused forms that are compiled: dilation 1 | 2; split: 2 / 4 / 8 wavefronts of 64 channels, fp32: 2 / 4 wavefront pairs of 32.
// Whether the 1 x 1 layer p can take a depthwise 3 x 3 of dilation `dil` in front of it in the same launch (p.dw_w etc. not yet set).
inline bool dw_fusable(const conv32_params& p, bool split, int dil)
{
    return direct_ok(p) && p.KH == 1 && (dil == 1 || dil == 2) && direct_mw(p, split, dil) != 0;
}

// The pairs conv32_head_kernel takes: 1 x 1 / stride 1 / no padding on both layers, 128 input channels (a 4-aligned slice), a hidden width that is a
// multiple of 128 (32 rows x four wavefronts), at most 64 outputs, no residual on either layer
inline bool head_ok(int k1, int hid, int c2) { return k1 == HK1 && hid >= 128 && hid % 128 == 0 && c2 >= 1 && c2 <= 64; }
inline int head_tm2(int c2) { return c2 <= 32 ? 1 : 2; } // 32-row output tiles of the second layer
inline int head_tile(int hid, int c2) { return 37000000 + hid * 100 + c2; }

// whether two head launches may share one grid: the same input view and map
inline bool same_input(const conv32_params& a, const conv32_params& b)
{
    return a.in.p == b.in.p && a.in.cs == b.in.cs && a.in.coff == b.in.coff && a.in.wp == b.in.wp && a.in.img == b.in.img && a.OH == b.OH && a.OW == b.OW
        && a.npix == b.npix;
}
inline bool head_pair_ok(const conv32_params& a, const conv32_params& b, const engine_switches& sw) { return sw.head_pair32 && same_input(a, b); }

constexpr int wk_lds(int kt, int bn) { return kt / 16 * ((64 * 16 + 16) + (bn * 16 + 16)) * 4 + 4 * 16 * 36 * 4 + 3 * bn * 8; }

// Which layers take conv32_wk_kernel: 1 x 1 (any stride), exactly 32 / 64 input channels, an NHWC output only, and enough pixel tiles that
// two blocks per CU stay busy (HP_C32_WK=0: none, the A/B switch; =1: every layer of that shape).  Looks at pick_npix like gemm_tile.
inline int wk_bn(const conv32_params& p, const engine_switches& sw)
{
    const int wk = sw.c32_wk;
    if (wk == 0 || p.KH != 1 || p.KW != 1 || p.dil != 1 || p.out_f32 || !p.out.p || (p.Cin != 32 && p.Cin != 64))
        return 0;
    // (K = 128, 77 KB and two blocks per CU, won nothing: ResNet's 128 -> 512 at 32 x 48 x 48 140 -> 135 us, MobileNet's 128 -> 128 at 8 x 92 x 108
    // 38.6 -> 41.6, profiles/r06_ab_layers_f32_whole_k.txt: not built)
    const int bn = 64; // (LDS: 27 / 44 KB per block at K = 32 / 64: five / three blocks per CU)
    const long np = p.pick_npix > 0 ? p.pick_npix : p.npix, blocks = (np + bn - 1) / bn * (p.Cout_pad / 64);
    return wk == 1 || blocks >= 768 ? bn : 0;
}

// Block tile (BM output channels x BN pixels) of a layer.  The fp32 matrix pipe is slow enough (64 cycles per MFMA) that small tiles cost
// little per MFMA, and a layer that is one wave of 128 x 128 tiles leaves CUs idle: LW-OpenPose's 3 x 3 128 -> 128 layers at 8 x 46 x 54 pixels
// are 156 such tiles on 256 CUs (0.38 of the fp32 MFMA peak) - as 64 x 64 tiles they are 622 blocks, several per CU.
inline void gemm_tile(const conv32_params& p, const engine_switches& sw, int& BM, int& BN)
{
    BM = p.Cout_pad % 128 == 0 ? 128 : 64, BN = 128;
    const long blocks = (long)(((p.pick_npix > 0 ? p.pick_npix : p.npix) + 127) / 128) * (p.Cout_pad / BM);
    if (blocks < 448) // fewer than ~1.75 blocks per CU: quarter the tile
        BM = 64, BN = 64;
    else if (blocks < 1024 && BM == 128) // up to four blocks per CU: halve the tile (512 -> 512 at 8 x 46 x 54: 115 -> 100 us alone, same machine time)
        BM = 64;
    // Round quantisation: 64 x 128 tiles have 1024 slots (four blocks per CU); a layer that is "one round and a bit" of them but ONE round of
    // 64 x 160 tiles takes conv32_t16_kernel<160> (see there).  HP_C32_BN160=0: the A/B switch back; =1: every layer (tests).
    const int bn160 = sw.c32_bn160;
    if (bn160 == 1) { // (tests: every layer on the 64 x 160 tile)
        BM = 64, BN = 160;
        return;
    }
    if (BM == 64 && BN == 128 && bn160 != 0) {
        const long np = p.pick_npix > 0 ? p.pick_npix : p.npix; // (the engine's max_batch geometry: see conv32_params::pick_npix)
        const long g = p.Cout_pad / 64, b128 = (long)((np + 127) / 128) * g, b160 = (long)((np + 159) / 160) * g;
        if (b128 > 1024 && b160 <= 1024)
            BN = 160;
        // (a 64 x 176 tile for b160 a few blocks over the 1 024 slots: 1 272 -> 1 172 us alone, 1 039 -> 1 053 with a second stream - not built)
    }
    // ResNet's 1 x 1 expansions with few input channels (64 -> 256 at 96 x 96, 128 -> 512 at 48 x 48, batch 32): four to eight K-steps, then 300 MB
    // of output + residual - the layer is its epilogue.  conv32_t16_kernel's stores cover 16 pixels x 64 contiguous bytes per instruction where
    // the 32 x 32 accumulator layout covers 64 pixels x 16 bytes: 259 -> 205 us alone, 218 -> 188 with a second stream for 64 -> 256, 146 -> 142 | 130 -> 126
    // for 128 -> 512; every wider-K layer is slower on it (profiles/r06_ab_layers_f32_config3_t16.txt)
    if (bn160 != 0 && p.KH == 1 && p.KW == 1 && p.stride == 1 && p.Cin <= 128 && p.Cout_pad >= 256 && !p.out_f32 && (BN == 128))
        BM = 64, BN = 160;
}

inline bool gemm_rows(const conv32_params& p, int BN)
{
    if (BN == 160)
        return false; // conv32_t16_kernel has the one epilogue (16 pixels x 64 contiguous bytes per store instruction)
    // The row-major epilogue pays on the 64-pixel tile only.  Measured per layer of LW-OpenPose @ 8 x 46 x 54 (us alone | with a second
    // stream; rows -> lane = pixel): <64, 64> 256 -> 256 33.2 | 26.9 -> 33.8 | 29.2, 128 -> 256 21.3 | 15.8 -> 21.7 | 19.0;  <64, 128> (two
    // channel tiles per wavefront: eight pixel rows of 256 B in flight per lane group) 128 -> 512 61.5 | 40.3 -> 35.1 | 27.4, 32 -> 64 at
    // 184 x 216 59.2 | 46.6 -> 36.0 | 29.6, 512 -> 512 129 | 93 -> 106 | 94 (profiles/r05_ab_layers_f32_*_epilogue.txt).
    // HP_LANE_EPILOGUE=1: lane form everywhere, HP_LANE_EPILOGUE=-1: row form everywhere.
    return !p.out_f32 && (p.lane_epilogue < 0 || (p.lane_epilogue == 0 && BN == 64));
}

// Column tiles per block: 2 (16 x 8 pixels) or 1 (8 x 8 pixels: twice the blocks, half the accumulators, three blocks per CU - and twice the U
// bytes per MFMA).  A 128 -> 128 layer at 8 x 46 x 54 is 336 blocks of the first form for 256 CUs x 2: 176 CUs run one block, 80 run two and
// set the launch's time (45.0 us); as 672 blocks of the second it takes 35.9 us alone and the same 27 us next to a second stream's launch -
// but four pipes lose 1.4 % (5 113 -> 5 042 frames/s, three runs each: the U stream).  So: the small form for a caller with ONE batch in flight
// (conv32_params::latency, i.e. hp_engine_set_concurrency(e, 2)) when the large form would not fill the chip's 512 slots twice; the same
// tiles, the same arithmetic: the same bits (tests/test_engine_fp32_gpu.py).  HP_WINO_NC=1 | 2 forces one.
inline int winograd_nc(const conv32_params& p, const engine_switches& sw, int blocks_nc2)
{
    const int force = sw.wino_nc;
    if (force == 1 || force == 2)
        return force;
    return p.latency && blocks_nc2 <= 512 ? 1 : 2;
}

// Rows per image of the tall form, or 0 where it does not apply: the input's images must lie vh = even rows apart with at least one (zero) halo
// row above and below each.  HP_WINO_TALL=0: the A/B switch.
inline int winograd_tall(const conv32_params& p, const engine_switches& sw)
{
    if (!sw.wino_tall)
        return 0;
    if (p.B < 2 || p.in.wp <= 0 || p.in.img % p.in.wp)
        return 0;
    const int vh = p.in.img / p.in.wp;
    return (vh & 1) == 0 && vh >= p.H + 2 ? vh : 0;
}

inline void set_targ(conv32_choice& c, int a0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0) { c.targ[0] = a0, c.targ[1] = a1, c.targ[2] = a2, c.targ[3] = a3, c.targ[4] = a4; }

} // namespace pick32

// The launch of dense layer p as `form` (split: the direct kernel's products on the fp16 pipe).  Every field of p that the launch depends on is
// read here and nowhere else; the pointers w_frag / w_split / w_wino are the launcher's argument check.
inline conv32_choice pick_conv32(const conv32_params& p, const engine_switches& sw, conv32_form form, bool split)
{
    using namespace pick32;
    conv32_choice c{};
    c.grid_y = 1, c.threads = 256;
    switch (form) {
    case C32_GEMM:
        c.ok = true; // (any geometry)
        if (const int bn = wk_bn(p, sw)) {
            c.kernel = K32_WK, set_targ(c, p.Cin, bn);
            c.grid_x = ((p.npix + bn - 1) / bn + 7) / 8 * 8 * (p.Cout_pad / 64);
            c.lds = wk_lds(p.Cin, bn);
            c.tile = 39000000 + p.Cin * 1000 + bn;
        } else {
            int BM, BN, WM = 0, WN = 0;
            gemm_tile(p, sw, BM, BN);
            const bool rows = gemm_rows(p, BN);
#define HP_X(BM_, BN_, WM_, WN_) \
    if (BM == BM_ && BN == BN_)  \
        WM = WM_, WN = WN_;
            HP_CONV32_INSTANCES(HP_X)
#undef HP_X
            if (BN == 160)
                c.kernel = K32_T16, set_targ(c, BN, 2);
            else
                c.kernel = K32_CONV, set_targ(c, BM, BN, WM, WN, rows);
            c.grid_x = ((p.npix + BN - 1) / BN + 7) / 8 * 8 * (p.Cout_pad / BM); // XCD-aware 1-D order: see conv32_kernel
            c.tile = 32000000 + (rows ? 400000 : 0) + BM * 1000 + BN;
        }
        break;
    case C32_WINO2: {
        c.ok = winograd_ok(p);
        c.tiles_x = (p.OW + WINO_BW - 1) / WINO_BW;
        const int nc = winograd_nc(p, sw, c.tiles_x * ((p.OH + 15) / 16) * p.B * (p.Cout_pad / 64)), bh = 8 * nc;
        int tiles_y = (p.OH + bh - 1) / bh, vh = winograd_tall(p, sw), images = p.B, rows = 0;
        // the rows form (tile rows numbered per image: see the kernel) where an image has at least a block's tile rows and the batch's tile rows
        // are fewer blocks than the images' own; it reads what the per-image form reads, whatever lies between two images
        const int T = (p.OH + 1) / 2, rows_y = (p.B * T + 4 * nc - 1) / (4 * nc);
        if (sw.wino_tall && p.B > 1 && T >= 4 * nc && rows_y < tiles_y * p.B)
            tiles_y = rows_y, images = 1, rows = T, vh = 0;
        else if (vh) { // fewer tile rows per image: the tall form
            const int tall_y = ((p.B - 1) * vh + p.H + bh - 1) / bh;
            if (tall_y < tiles_y * p.B)
                tiles_y = tall_y, images = 1;
            else
                vh = 0; // (a map that is whole 16-row blocks already: 48 rows + 2 halo rows would only add separator rows)
        }
        c.kernel = K32_WINO2, set_targ(c, WINO_MW, true, nc);
        c.tiles_y = tiles_y, c.vh = vh, c.rows = rows;
        c.grid_x = (c.tiles_x * tiles_y * images + 7) / 8 * 8 * (p.Cout_pad / (16 * WINO_MW)); // XCD-aware 1-D order: see the kernel
        c.threads = 64 * WINO_MW, c.lds = WINO_LDS[nc];
        c.tile = 35000000 + 3000 + 4; // four wavefronts (16-channel MFMA tiles) per block, the pipelined form: see "Kernel shape"
        break;
    }
    case C32_DIRECT: {
        const int dwd = p.dw_w ? p.dw_dil : 0, mw = direct_mw(p, split, dwd);
        const long lds = direct_lds(split, p.KH, mw, dwd);
        c.kernel = K32_DIRECT, set_targ(c, split, p.KH, direct_chunk(p.KH * p.KW), mw, dwd);
        c.tile = (split ? 33000000 : 34000000) + (p.dw_w ? 100000 * p.dw_dil : 0) + p.KH * 1000 + mw;
        c.lds = lds < 0 ? 0 : (size_t)lds + (dwd ? (size_t)40 * p.Cin : 0);
        c.ok = direct_ok(p) && lds >= 0 && c.lds <= 160 * 1024;
        if (!c.ok)
            break;
        c.tiles_x = (p.OW + DIRECT_T - 1) / DIRECT_T, c.tiles_y = (p.OH + DIRECT_T - 1) / DIRECT_T;
        c.grid_x = c.tiles_x * c.tiles_y * p.B, c.grid_y = p.Cout_pad / ((split ? 64 : 32) * mw);
        c.threads = (split ? 64 : 128) * mw;
        break;
    }
    }
    return c;
}

// The two-layer heads: q = the second layer's parameters, hid = the hidden width; qb / hidb: the sibling head that shares the grid (pair kernel)
inline conv32_choice pick_head32(const conv32_params& q, int hid, const conv32_params* qb = nullptr, int hidb = 0)
{
    using namespace pick32;
    conv32_choice c{};
    c.ok = head_ok(HK1, hid, q.Cout) && q.npix > 0 && (!qb || (head_ok(HK1, hidb, qb->Cout) && qb->npix > 0 && same_input(q, *qb)));
    c.kernel = qb ? K32_HEAD_PAIR : K32_HEAD, set_targ(c, head_tm2(q.Cout), qb ? head_tm2(qb->Cout) : 0);
    const unsigned blocks = (q.npix + HEAD_PX - 1) / HEAD_PX;
    c.grid_x = qb ? (blocks + 7) / 8 * 8 * 2 : blocks, c.grid_y = 1, c.threads = 256; // (a pair: whole groups of eight tiles, the two heads of a tile eight ids apart)
    c.tile = head_tile(hid, q.Cout);
    return c;
}

// Build time: which weight forms dense layer p gets (p filled but for the forms' pointers; Cin = the layer's channels padded to 16), what it is
// launched as and, for the direct kernel, the channel count the launch reads (whole chunks).  dw_in_front: a depthwise layer is fused in front;
// room: the channels the input buffer has from the slice's first one; layer_cin: the layer's own input channels.
struct conv32_forms {
    bool w_wino, w_frag, w_split;
    conv32_form kind;
    int cin_split;
};
inline conv32_forms conv32_layer_forms(const conv32_params& p, int dtype, const engine_switches& sw, bool dw_in_front, int room, int layer_cin)
{
    using namespace pick32;
    conv32_forms f{};
    f.kind = C32_GEMM;
    // HP_DTYPE_F32: 3 x 3 stride-1 layers in Winograd's F(2 x 2, 3 x 3) form (HP_NO_WINOGRAD32=1 is the A/B switch back to the direct kernel).
    // (Never a layer with a depthwise or hidden layer fused in front: those are 1 x 1.)
    if (dtype == HP_DTYPE_F32 && !sw.no_winograd32 && winograd_ok(p))
        f.w_wino = true, f.kind = C32_WINO2;
    // a 3 x 3 layer the Winograd kernel has taken needs no direct-form fragments (they doubled its weight bytes in HBM); 1 x 1 layers wider than
    // 64 padded outputs stay on conv32_kernel - unless HP_DTYPE_F32S (every direct layer) or a depthwise layer is fused in front
    const int taps = p.KH * p.KW;
    if (dtype != HP_DTYPE_F32S && !dw_in_front && (f.w_wino || (taps == 1 && p.Cout_pad > 64)))
        return f;
    const int ck = direct_chunk(taps), cin_s = (layer_cin + ck - 1) / ck * ck;
    conv32_params q = p;
    q.Cin = cin_s;
    if (cin_s <= room && direct_ok(q))
        f.w_frag = true, f.w_split = dtype == HP_DTYPE_F32S, f.kind = C32_DIRECT, f.cin_split = cin_s;
    return f;
}

} // namespace hp
