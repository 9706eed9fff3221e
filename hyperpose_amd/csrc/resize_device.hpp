// resize_device.hpp — the ONE statement of the stream front-end's resize arithmetic (cv::resize INTER_LINEAR on CV_8UC3, see resize.hip and
// oracle/resize_oracle.cpp), shared by the kernels that differ only in where a source pixel's (b, g, r) come from:
//   bgr_taps     an 8-bit BGR HWC frame                                  (resize.hip,     resize_u8c3_kernel)
//   yuv420_taps  a YUV 4:2:0 frame, converted as the pixel is fetched    (resize_yuv.hip, resize_yuv420_kernel)
//   yuv_taps<>   any hp_yuv_image layout (resize_yuv_device.hpp)             (resize_yuv_formats.hip; resize_rois.hip: many regions of one frame,
//                                                                         every Taps type moved to a region's origin with Taps::at)
// A `Taps` type has  __device__ void load(int x, int y, int (&c)[3]) const  returning the B, G, R of source pixel (x, y), each in 0..255.
// resize_pixel() derives the source coordinates and the 11-bit coefficients of one output pixel, fetches at most 2 x 2 taps through
// Taps::load and writes the pixel; rz_prepare() is the host side: argument checks and the choice between the three modes.
#pragma once
#include "hp_common.hpp"

#include <cmath>

namespace hp_resize {

struct rz_geom {
    int sw, sh;
    uint8_t* dst;
    int dw, dh, dst_stride; // full destination frame
    int iw, ih;             // resized region (top-left); the rest of the frame gets the border colour
    int mode;               // 0 linear, 1 area 2x2, 2 copy
    double scale_x, scale_y;
    int bg[3];
};

struct bgr_taps {
    const uint8_t* src;
    int stride;
    __host__ __device__ __forceinline__ void load(int x, int y, int (&c)[3]) const
    {
        const uint8_t* s = src + (size_t)y * stride + x * 3;
        c[0] = s[0], c[1] = s[1], c[2] = s[2];
    }
    // the taps of the sub-image whose pixel (0, 0) is this frame's (rx, ry) (resize_rois.hip)
    __device__ __forceinline__ bgr_taps at(int rx, int ry) const { return bgr_taps{ src + (size_t)ry * stride + rx * 3, stride }; }
};

// (host and device: the scale ensemble's host twin, hp_scale_stage_u8c3_host, runs resize_pixel on the CPU; the device code is unchanged)
__host__ __device__ __forceinline__ short sat_short_rn(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int r = __float2int_rn(v);
#else
    const int r = (int)std::nearbyint(v); // round half to even, as __float2int_rn, in the default rounding mode
#endif
    return (short)min(max(r, -32768), 32767);
}

// one output pixel (x, y) of the destination frame; the caller has checked x < dw, y < dh
template <class Taps> __host__ __device__ __forceinline__ void resize_pixel(const rz_geom& p, const Taps& t, int x, int y)
{
    uint8_t* d = p.dst + (size_t)y * p.dst_stride + x * 3;
    if (x >= p.iw || y >= p.ih) {
        d[0] = (uint8_t)p.bg[0], d[1] = (uint8_t)p.bg[1], d[2] = (uint8_t)p.bg[2];
        return;
    }
    int t00[3], t01[3], t10[3], t11[3];
    if (p.mode == 2) {
        t.load(x, y, t00);
        d[0] = (uint8_t)t00[0], d[1] = (uint8_t)t00[1], d[2] = (uint8_t)t00[2];
        return;
    }
    if (p.mode == 1) {
        t.load(2 * x, 2 * y, t00), t.load(2 * x + 1, 2 * y, t01), t.load(2 * x, 2 * y + 1, t10), t.load(2 * x + 1, 2 * y + 1, t11);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            d[c] = (uint8_t)((t00[c] + t01[c] + t10[c] + t11[c] + 2) >> 2);
        return;
    }
    float fx = (float)((x + 0.5) * p.scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= sx;
    if (sx < 0)
        fx = 0.f, sx = 0;
    const bool two_tap = sx + 1 < p.sw; // dx < xmax
    if (sx >= p.sw - 1)
        fx = 0.f, sx = p.sw - 1;
    const int a0 = sat_short_rn((1.f - fx) * 2048.f), a1 = sat_short_rn(fx * 2048.f);
    float fy = (float)((y + 0.5) * p.scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= sy;
    const int b0 = sat_short_rn((1.f - fy) * 2048.f), b1 = sat_short_rn(fy * 2048.f);
    const int y0 = min(max(sy, 0), p.sh - 1), y1 = min(max(sy + 1, 0), p.sh - 1);
    const int x1 = two_tap ? sx + 1 : sx; // the second column is read only where it exists
    t.load(sx, y0, t00), t.load(x1, y0, t01), t.load(sx, y1, t10), t.load(x1, y1, t11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int h0 = two_tap ? t00[c] * a0 + t01[c] * a1 : t00[c] * 2048;
        const int h1 = two_tap ? t10[c] * a0 + t11[c] * a1 : t10[c] * 2048;
        d[c] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
    }
}

// the thread -> pixel map of both kernels: blocks of 32 x 8 output pixels, 256 threads
constexpr int RZ_BLOCK_W = 32, RZ_BLOCK_H = 8;
inline dim3 rz_grid(const rz_geom& g) { return dim3(hp::ceil_div(g.dw, RZ_BLOCK_W), hp::ceil_div(g.dh, RZ_BLOCK_H)); }

// host side: checks the geometry and picks the mode as cv::resize does (2 x 2 down-scale -> area average, equal sizes -> copy)
inline int rz_prepare(rz_geom& p, int sw, int sh, uint8_t* dst, int dw, int dh, int dst_stride, int iw, int ih, const int bg[3])
{
    HP_REQUIRE(dst && sw > 0 && sh > 0 && dw > 0 && dh > 0 && iw >= 0 && ih >= 0 && iw <= dw && ih <= dh, HP_ERR_INVALID, "resize: bad geometry");
    HP_REQUIRE(dst_stride >= dw * 3, HP_ERR_INVALID, "resize: row stride smaller than a row");
    p.sw = sw, p.sh = sh, p.dst = dst, p.dw = dw, p.dh = dh, p.dst_stride = dst_stride;
    p.iw = iw, p.ih = ih, p.bg[0] = bg[0], p.bg[1] = bg[1], p.bg[2] = bg[2];
    p.mode = 0, p.scale_x = 1, p.scale_y = 1;
    if (iw > 0 && ih > 0) {
        const double inv_scale_x = (double)iw / sw, inv_scale_y = (double)ih / sh;
        p.scale_x = 1. / inv_scale_x, p.scale_y = 1. / inv_scale_y;
        const int iscale_x = (int)std::lrint(p.scale_x), iscale_y = (int)std::lrint(p.scale_y);
        const bool is_area_fast = std::abs(p.scale_x - iscale_x) < 2.220446049250313e-16 && std::abs(p.scale_y - iscale_y) < 2.220446049250313e-16;
        if (sw == iw && sh == ih)
            p.mode = 2;
        else if (is_area_fast && iscale_x == 2 && iscale_y == 2)
            p.mode = 1;
    }
    return HP_OK;
}

} // namespace hp_resize
