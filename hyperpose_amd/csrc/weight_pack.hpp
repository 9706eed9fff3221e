// weight_pack.hpp — the weight layouts the engine uploads (engine.cpp), as pure host functions: blob floats in, the packed buffer out.
// No HIP runtime call and nothing of hp_engine, so every layout runs in a plain host program (tests/cpp/weight_pack.cpp).  Sources are
// pointers into the weight blob as the exported graph stores them: dense [cout][taps][cin], depthwise [C][9].  The layouts that belong to
// one fp32 kernel family stay next to it and are only called from the engine: conv32_frag_pack, conv32_split_pack, conv32_winograd_pack,
// conv32_head_pack (conv_fp32.hpp).
#pragma once
#include "conv_i8.hpp" // conv_i8_direct_index; __half / __float2half through conv_kernels.hpp

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace hp {
namespace wpack {

// n floats zero-padded to n_pad (biases, PReLU slopes); src == nullptr: all zeros
inline std::vector<float> padded(const float* src, size_t n, size_t n_pad)
{
    std::vector<float> v(n_pad, 0.f);
    if (src)
        std::copy(src, src + n, v.begin());
    return v;
}

// ---- depthwise 3 x 3: [C][9] -> [9][C]
inline std::vector<float> dw_taps32(const float* w, int C)
{
    std::vector<float> packed((size_t)9 * C);
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < 9; ++t)
            packed[(size_t)t * C + c] = w[(size_t)c * 9 + t];
    return packed;
}
inline std::vector<__half> dw_taps16(const float* w, int C)
{
    std::vector<__half> packed((size_t)9 * C);
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < 9; ++t)
            packed[(size_t)t * C + c] = __float2half(w[(size_t)c * 9 + t]);
    return packed;
}
// conv32_direct_kernel's fused form: [9][C] + the bias as row 9
inline std::vector<float> dw_taps32_bias(const float* w, const float* bias, int C)
{
    std::vector<float> dpack = dw_taps32(w, C);
    dpack.insert(dpack.end(), bias, bias + C);
    return dpack;
}

// ---- dense fp32: rows [taps][cout_pad][cin_pad] ...
inline std::vector<float> dense32_rows(const float* w, int cout, int taps, int cin, int cout_pad, int cin_pad)
{
    std::vector<float> packed((size_t)taps * cout_pad * cin_pad, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int t = 0; t < taps; ++t)
            std::copy(w + ((size_t)co * taps + t) * cin, w + ((size_t)co * taps + t + 1) * cin, packed.begin() + ((size_t)t * cout_pad + co) * cin_pad);
    return packed;
}
// ... and the same rows at the stride conv32_direct_kernel reads them with (whole 32- / 64-channel chunks: cin_s >= cin_pad)
inline std::vector<float> restride32(const std::vector<float>& packed, int taps, int cout_pad, int cin_pad, int cin_s)
{
    std::vector<float> wide((size_t)taps * cout_pad * cin_s, 0.f);
    for (int t = 0; t < taps; ++t)
        for (int co = 0; co < cout_pad; ++co)
            std::copy(packed.begin() + ((size_t)t * cout_pad + co) * cin_pad, packed.begin() + ((size_t)t * cout_pad + co) * cin_pad + cin_pad,
                wide.begin() + ((size_t)t * cout_pad + co) * cin_s);
    return wide;
}

// ---- fp16
// element (m, k) of a K-wide fp16 matrix in MFMA fragment order: [32-row tile][16-wide k step][lane = (k % 16 / 8) * 32 + m % 32][k % 8],
// KQ = K / 16 steps; tile0 = 32-row tiles in front of the matrix (a convolution's earlier taps)
inline size_t frag16(size_t m, size_t k, size_t KQ, size_t tile0 = 0) { return (((tile0 + m / 32) * KQ + k / 16) * 64 + (k % 16 / 8) * 32 + m % 32) * 8 + k % 8; }

// dense weights as conv_weight_layout() asks: 0 = rows [taps][cout_pad][cin_pad], 1 = fragment order, every tap cout_pad / 32 tiles behind the last
// (with one tap and cin_pad = cin: the [rows][K] fragment matrix of a separable block's pointwise half and of a head's first layer)
inline std::vector<__half> dense16(const float* w, int cout, int taps, int cin, int cout_pad, int cin_pad, int w_layout)
{
    std::vector<__half> packed((size_t)taps * cout_pad * cin_pad, __float2half(0.f));
    const int KQ = cin_pad / 16;
    for (int co = 0; co < cout; ++co)
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < cin; ++ci) {
                const size_t at = w_layout == 1
                    ? frag16(co, ci, KQ, (size_t)t * (cout_pad / 32))
                    : ((size_t)t * cout_pad + co) * cin_pad + ci;
                packed[at] = __float2half(w[((size_t)co * taps + t) * cin + ci]);
            }
    return packed;
}
// mlp_head_kernel's second layer (head_params::w2): [cout2][HID] rows padded to 64, the hidden channel c = 128 wv + 32 ii + r32 at K-step
// 8 wv + 2 ii + ss, lane half hh, element ee
inline std::vector<__half> head_w2(const float* w2, int cout2, int HID)
{
    std::vector<__half> w2p((size_t)64 * HID, __float2half(0.f));
    for (int m = 0; m < cout2; ++m)
        for (int c = 0; c < HID; ++c) {
            const int wv = c / 128, ii = (c % 128) / 32, r32 = c % 32;
            const int hh = (r32 >> 2) & 1, r = (r32 & 3) + 4 * (r32 >> 3), ss = r >> 3, ee = r & 7;
            w2p[((((size_t)(m / 32) * 32 + 8 * wv + 2 * ii + ss) * 64) + hh * 32 + m % 32) * 8 + ee] = __float2half(w2[(size_t)m * HID + c]);
        }
    return w2p;
}
// fragment order of first_conv_f16_kernel: [cout][KS][KS][3] with kernel rows padded to ROWP (a multiple of 8), K' = KS * ROWP in steps of 16
inline std::vector<__half> first_conv_frag16(const float* w, int cout, int KS)
{
    const int ROWP = (KS * 3 + 7) / 8 * 8, KP = KS * ROWP, STEPS = (KP + 15) / 16, MT = cout <= 32 ? 1 : 2;
    std::vector<__half> w16((size_t)MT * STEPS * 64 * 8, __float2half(0.f));
    for (int co = 0; co < cout; ++co)
        for (int ky = 0; ky < KS; ++ky)
            for (int r = 0; r < KS * 3; ++r)
                w16[frag16(co, ky * ROWP + r, STEPS)] = __float2half(w[((size_t)co * KS + ky) * KS * 3 + r]);
    return w16;
}

// ---- int8 weights, symmetric per output channel: s_w[c] = max |w| / 127 (1 for an all-zero channel), q_w = clamp(rint(w / s_w[c]), -127, 127)
// in fp32, round-half-even; rows [tap][cout_pad][cin_pad] as conv_i8_kernel reads them
struct i8_rows {
    std::vector<float> s_w; // [cout]
    std::vector<int8_t> q;
};
inline i8_rows quantize_rows(const float* w, int cout, int taps, int cin, int cout_pad, int cin_pad)
{
    i8_rows r{ std::vector<float>(cout), std::vector<int8_t>((size_t)taps * cout_pad * cin_pad, 0) };
    for (int co = 0; co < cout; ++co) {
        const float* wc = w + (size_t)co * taps * cin;
        float m = 0.f;
        for (size_t k = 0; k < (size_t)taps * cin; ++k)
            m = std::max(m, std::fabs(wc[k]));
        const float sc = m > 0.f ? m / 127.f : 1.f;
        r.s_w[co] = sc;
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < cin; ++ci)
                r.q[((size_t)t * cout_pad + co) * cin_pad + ci] = (int8_t)std::min(std::max(std::rint(wc[(size_t)t * cin + ci] / sc), -127.f), 127.f);
    }
    return r;
}
// the same q_w in conv_i8_direct_kernel's fragment order
inline std::vector<int8_t> i8_direct(const std::vector<int8_t>& wq, int taps, int cout_pad, int cin_pad)
{
    std::vector<int8_t> wd(wq.size(), 0);
    for (int t = 0; t < taps; ++t)
        for (int co = 0; co < cout_pad; ++co)
            for (int ci = 0; ci < cin_pad; ++ci)
                wd[conv_i8_direct_index(t, co, ci, cin_pad, cout_pad)] = wq[((size_t)t * cout_pad + co) * cin_pad + ci];
    return wd;
}

} // namespace wpack
} // namespace hp
