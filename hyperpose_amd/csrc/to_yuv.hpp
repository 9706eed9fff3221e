// to_yuv.hpp — the ONE statement of hp_rgb_to_yuv (include/hp_hip.h, "encoder hand-off"): a packed RGB or grey frame (hp_rgb_image) as the samples
// of any hp_yuv_image layout in the target's matrix, range and bit depth, padded by edge replication to the size an encoder takes.  The forward
// counterpart of hp_resize_yuv.  Shared by the kernels and the C ABI (to_yuv.hip) and quoted by DESIGN.md 1.1 "Encoder hand-off"; the tests restate
// it in numpy with Python integers (tests/to_yuv_ref.py).  The coefficients are host doubles rounded once, everything after them is exact int32
// arithmetic: GPU, host twin and tests agree byte for byte.  The host side needs nothing but hp_hip.h and the pure headers beside it and compiles with
// a plain C++ compiler: tests/cpp/to_yuv_rules.cpp runs it under sanitizers on frames allocated with no slack.
//
// 1. Coefficients (host, float64).  kr, kb of the matrix (yuv_colour.hpp), kg = 1 - kr - kb, d = 8 or 10, S = 18.
//      LIMITED  ys = 219 * 2^(d-8) / 255, cs = 224 * 2^(d-8) / 255, y_off = 16 * 2^(d-8), c_off = 128 * 2^(d-8)
//      FULL     ys = cs = (2^d - 1) / 255, y_off = 0, c_off = 2^(d-1)
//      YR = rint(kr ys 2^S), YB = rint(kb ys 2^S), YG = rint(ys 2^S) - YR - YB
//      UB = rint(0.5 cs 2^S), UR = -rint(kr / (2 (1 - kb)) cs 2^S), UG = -UB - UR
//      VR = rint(0.5 cs 2^S), VB = -rint(kb / (2 (1 - kr)) cs 2^S), VG = -VR - VB
//    table = { y_off, c_off, YR, YG, YB, UR, UG, UB, VR, VG, VB }.  The chroma rows sum to zero: a grey pixel gives exactly c_off.
// 2. Pixel.  R, G, B are the 8-bit values of hp_rgb_to_bgr_host's definition (rgb_formats.hpp; GRAY8: all three are the sample, a fourth byte is
//    ignored).  Y = clip((YR R + YG G + YB B + (y_off << S) + (1 << (S - 1))) >> S), clip to [0, 2^d - 1].
// 3. Chroma.  One sample covers n = 1 (4:4:4), 2 (4:2:2) or 4 (4:2:0) luma pixels; Rs, Gs, Bs are the sums over them (the box mean, the inverse of
//    the replication hp_resize_yuv states):  U = clip((UR Rs + UG Gs + UB Bs + n ((c_off << S) + (1 << (S - 1)))) >> (S + log2 n)), V likewise.
//    Every shifted value is non-negative and below 2^31 (checked over all 2^24 colours of the twelve tables: at least 131 072, at most 1 073 741 800
//    for n = 4), so int32 suffices on the device.
// 4. Padding.  dst.width >= src.width, dst.height >= src.height; output pixel (x, y) takes source pixel (min(x, sw - 1), min(y, sh - 1)).
// 5. Samples lie where hp_yuv::map_samples says; 16-bit layouts store value << shift, the other bits zero.  No byte of dst outside the samples of its
//    width x height is written, no byte of src outside width * pixel bytes of a row is read.
#pragma once
#include <cmath>
#include <stdint.h>

#include "rgb_formats.hpp"
#include "yuv_colour.hpp"
#include "yuv_formats.hpp"

#if defined(__HIPCC__)
#define HP_ENC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HP_ENC_HD inline
#endif

namespace hp_enc {

constexpr int S = 18;         // the coefficients are multiples of 2^-18
constexpr int MAX_DIM = 8192; // the largest side of an output
constexpr int MAX_ALIGN = 256;

// the table as the kernels and the host twin read it: rows in (R, G, B) order
struct table {
    int32_t y_off, c_off;
    int32_t y[3], u[3], v[3];
};

// ---- 1. coefficients: matrix, range and depth (8 or 10) have been checked ------------------------------------------------------------------------

inline void forward_coefficients(int matrix, int range, int depth, int32_t out[11])
{
    const double kr = hp_yuv::KR[matrix], kb = hp_yuv::KB[matrix], one = (double)(1 << S), up = (double)(1 << (depth - 8));
    const bool limited = range == HP_YUV_LIMITED;
    const double ys = limited ? 219. * up / 255. : (double)((1 << depth) - 1) / 255.;
    const double cs = limited ? 224. * up / 255. : (double)((1 << depth) - 1) / 255.;
    out[0] = limited ? 16 << (depth - 8) : 0;
    out[1] = 1 << (depth - 1);
    const int32_t YR = (int32_t)std::rint(kr * ys * one), YB = (int32_t)std::rint(kb * ys * one), YG = (int32_t)std::rint(ys * one) - YR - YB;
    const int32_t UB = (int32_t)std::rint(0.5 * cs * one), UR = -(int32_t)std::rint(kr / (2. * (1. - kb)) * cs * one), UG = -UB - UR;
    const int32_t VR = (int32_t)std::rint(0.5 * cs * one), VB = -(int32_t)std::rint(kb / (2. * (1. - kr)) * cs * one), VG = -VR - VB;
    out[2] = YR, out[3] = YG, out[4] = YB;
    out[5] = UR, out[6] = UG, out[7] = UB;
    out[8] = VR, out[9] = VG, out[10] = VB;
}

inline table table_of(int matrix, int range, int depth)
{
    int32_t k[11];
    forward_coefficients(matrix, range, depth, k);
    return table{ k[0], k[1], { k[2], k[3], k[4] }, { k[5], k[6], k[7] }, { k[8], k[9], k[10] } };
}

// ---- 2., 3. samples -------------------------------------------------------------------------------------------------------------------------------

HP_ENC_HD int clip(int v, int top) { return v < 0 ? 0 : v > top ? top : v; }

HP_ENC_HD int luma(const table& t, int r, int g, int b, int top)
{
    return clip((t.y[0] * r + t.y[1] * g + t.y[2] * b + (t.y_off << S) + (1 << (S - 1))) >> S, top);
}

// `row` is table::u or table::v; rs, gs, bs the sums over the 1 << log2n pixels of the sample
HP_ENC_HD int chroma(const int32_t (&row)[3], int c_off, int rs, int gs, int bs, int log2n, int top)
{
    return clip((row[0] * rs + row[1] * gs + row[2] * bs + (((c_off << S) + (1 << (S - 1))) << log2n)) >> (S + log2n), top);
}

// ---- 4. padding -----------------------------------------------------------------------------------------------------------------------------------

// the smallest size >= (w, h) whose sides are multiples of `align` (1 .. MAX_ALIGN) and of what the layout needs; w, h > 0
inline void padded_size(const hp_yuv::layout& l, int w, int h, int align, int* pw, int* ph)
{
    auto lcm = [](int a, int b) {
        int x = a, y = b;
        while (y) {
            const int r = x % y;
            x = y, y = r;
        }
        return a / x * b;
    };
    const int ax = lcm(align, 1 << l.sx), ay = lcm(align, 1 << l.sy);
    *pw = (w + ax - 1) / ax * ax, *ph = (h + ay - 1) / ay * ay;
}

// What hp_rgb_to_yuv asks beyond the checks of the two descriptions; 0, or -1 with the refusal in msg (it names the layout and the quantity)
inline int check_sizes(const hp_rgb_image& src, const hp_yuv_image& dst, const char* who, char* msg, size_t cap)
{
    const char* name = hp_yuv::layout_of(dst.format)->name;
    if (dst.width > MAX_DIM || dst.height > MAX_DIM)
        return snprintf(msg, cap, "%s: %s: an output of %d x %d is beyond %d x %d", who, name, dst.width, dst.height, MAX_DIM, MAX_DIM), -1;
    if (dst.width < src.width)
        return snprintf(msg, cap, "%s: %s: output width %d is smaller than the %s frame's %d", who, name, dst.width, hp_rgb::layout_of(src.format)->name,
                   src.width),
               -1;
    if (dst.height < src.height)
        return snprintf(msg, cap, "%s: %s: output height %d is smaller than the %s frame's %d", who, name, dst.height, hp_rgb::layout_of(src.format)->name,
                   src.height),
               -1;
    return 0;
}

// ---- host twin: both descriptions have been checked; samples are read and written bytewise (hp_yuv::host_put) ---------------------------------------

inline void convert_host(const hp_rgb_image& src, const hp_yuv_image& dst)
{
    const hp_rgb::layout& in = *hp_rgb::layout_of(src.format);
    const hp_yuv::layout& l = *hp_yuv::layout_of(dst.format);
    const hp_yuv::sample_map m = hp_yuv::map_samples(dst, l);
    const int depth = l.sample_bytes == 2 ? 10 : 8, top = (1 << depth) - 1;
    const table t = table_of(dst.matrix, dst.range, depth);
    uint8_t *py = const_cast<uint8_t*>(m.y), *pu = const_cast<uint8_t*>(m.u), *pv = const_cast<uint8_t*>(m.v);
    for (int by = 0; by < dst.height >> l.sy; ++by)
        for (int bx = 0; bx < dst.width >> l.sx; ++bx) {
            int rs = 0, gs = 0, bs = 0;
            for (int dy = 0; dy < (1 << l.sy); ++dy)
                for (int dx = 0; dx < (1 << l.sx); ++dx) {
                    const int x = (bx << l.sx) + dx, y = (by << l.sy) + dy;
                    const int sx = x < src.width - 1 ? x : src.width - 1, sy = y < src.height - 1 ? y : src.height - 1;
                    const uint8_t* p = (const uint8_t*)src.data + (size_t)sy * src.stride + (size_t)sx * in.pixel_bytes;
                    const int r = p[in.r], g = p[in.g], b = p[in.b];
                    rs += r, gs += g, bs += b;
                    hp_yuv::host_put(py + (size_t)y * m.y_stride + (size_t)x * m.y_step, l.sample_bytes, l.shift, luma(t, r, g, b, top));
                }
            const size_t at = (size_t)by * m.c_stride + (size_t)bx * m.c_step;
            hp_yuv::host_put(pu + at, l.sample_bytes, l.shift, chroma(t.u, t.c_off, rs, gs, bs, l.sx + l.sy, top));
            hp_yuv::host_put(pv + at + (ptrdiff_t)by * m.v_extra, l.sample_bytes, l.shift, chroma(t.v, t.c_off, rs, gs, bs, l.sx + l.sy, top));
        }
}

} // namespace hp_enc
