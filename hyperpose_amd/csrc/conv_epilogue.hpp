// conv_epilogue.hpp — the generic epilogue of the fp16 MFMA convolutions (bias, piecewise-linear activation, residual,
// fp16 NHWC store and the fp32 NCHW network-output copy), shared by conv_kernels.hip and the int8 kernels of conv_i8.hip.
#pragma once
#include "conv_device.hpp"

namespace hp {

// Shared epilogue.  Lane holds, for MFMA tile (i, j), pixel j-th "column" (given by pb/py/px/pv) and channels
// m_wave + i*32 + 8g + 4*(lane>>5) + {0..3}, g = 0..3.  Activations are piecewise linear:
// y = v > 0 ? min(v, hi) : v * slope  (none / relu / relu6 / leaky / prelu).
template <int TM, int TN, int EPI>
__device__ __forceinline__ void conv_epilogue(const conv_params& p, const floatx16 (&acc)[TM][TN], int m_wave, int lane,
    const int (&pb)[TN], const int (&py)[TN], const int (&px)[TN], const bool (&pv)[TN])
{
    const float hi = p.act_hi;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const bool nvalid = pv[j];
        long o_off = 0, r_off = 0, f_off = 0;
        if (nvalid) {
            if (p.out.p)
                o_off = tv_off(p.out, pb[j], py[j], px[j]);
            if (p.res.p)
                r_off = tv_off(p.res, pb[j], py[j], px[j]);
            if (EPI == 1)
                f_off = ((long)pb[j] * p.Cout * p.OH + py[j]) * p.OW + px[j];
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int m = m_wave + i * 32 + 8 * g + 4 * (lane >> 5);
                if (nvalid && m < p.Cout) {
                    const float4 bs = *reinterpret_cast<const float4*>(p.bias + m);
                    float4 sl = make_float4(p.act_slope, p.act_slope, p.act_slope, p.act_slope);
                    if (p.alpha)
                        sl = *reinterpret_cast<const float4*>(p.alpha + m);
                    float v0 = acc[i][j][4 * g + 0] + bs.x, v1 = acc[i][j][4 * g + 1] + bs.y;
                    float v2 = acc[i][j][4 * g + 2] + bs.z, v3 = acc[i][j][4 * g + 3] + bs.w;
                    float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
                    if (p.res.p) {
                        const __half* rp = p.res.p + r_off + m;
                        if (EPI == 0) {
                            const half4 h = *reinterpret_cast<const half4*>(rp);
                            r0 = (float)h[0], r1 = (float)h[1], r2 = (float)h[2], r3 = (float)h[3];
                        } else {
                            r0 = __half2float(rp[0]);
                            r1 = m + 1 < p.Cout ? __half2float(rp[1]) : 0.f;
                            r2 = m + 2 < p.Cout ? __half2float(rp[2]) : 0.f;
                            r3 = m + 3 < p.Cout ? __half2float(rp[3]) : 0.f;
                        }
                        if (p.res_before_act)
                            v0 += r0, v1 += r1, v2 += r2, v3 += r3, r0 = r1 = r2 = r3 = 0.f;
                    }
                    v0 = (v0 > 0.f ? fminf(v0, hi) : v0 * sl.x) + r0;
                    v1 = (v1 > 0.f ? fminf(v1, hi) : v1 * sl.y) + r1;
                    v2 = (v2 > 0.f ? fminf(v2, hi) : v2 * sl.z) + r2;
                    v3 = (v3 > 0.f ? fminf(v3, hi) : v3 * sl.w) + r3;
                    if (EPI == 0) {
                        half4 h;
                        h[0] = (_Float16)v0, h[1] = (_Float16)v1, h[2] = (_Float16)v2, h[3] = (_Float16)v3;
                        *reinterpret_cast<half4*>(p.out.p + o_off + m) = h;
                    } else {
                        const bool c1 = m + 1 < p.Cout, c2 = m + 2 < p.Cout, c3 = m + 3 < p.Cout;
                        if (p.out.p) {
                            __half* op = p.out.p + o_off + m;
                            op[0] = __float2half(v0);
                            if (c1)
                                op[1] = __float2half(v1);
                            if (c2)
                                op[2] = __float2half(v2);
                            if (c3)
                                op[3] = __float2half(v3);
                        }
                        if (p.out_f32) {
                            const long plane = (long)p.OH * p.OW;
                            float* fp = p.out_f32 + f_off + (long)m * plane;
                            fp[0] = v0;
                            if (c1)
                                fp[plane] = v1;
                            if (c2)
                                fp[2 * plane] = v2;
                            if (c3)
                                fp[3 * plane] = v3;
                        }
                    }
                }
            }
        }
    }
}

} // namespace hp
