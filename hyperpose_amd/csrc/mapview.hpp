// mapview.hpp — the ONE statement of the picture hp_mapview_draw_* blends into a frame (include/hp_hip.h): a colour-mapped, up-sampled view of the
// network's own maps (confidence maps, part-affinity fields) over the frame they were computed from.  Shared by the kernels and the host twins
// (mapview.hip) and quoted by DESIGN.md 1.1 "Map view"; the tests restate it in numpy with Python integers (tests/mapview_ref.py).  The index plane
// is fp32 without fused operations, the taps are host doubles computed once and READ by kernel and host twin alike, everything after them is exact
// integer arithmetic: GPU, host twin and tests agree byte for byte.  The host side needs nothing but hp_hip.h and the pure headers beside it and
// compiles with a plain C++ compiler: tests/cpp/mapview_rules.cpp runs it under sanitizers on planes allocated with no slack.
//
// 1. Index plane.  A frame's maps [C][mh][mw] (fp32) become one uint8 plane [mh][mw].  Channels c_k = c0 + k * c_step, k < cn.
//      HP_MAPVIEW_MAX    m = 0; per channel in order: if (v > m) m = v           (NaN and negative values leave m alone)
//      HP_MAPVIEW_FIELD  the channels are pairs (c_k, c_k + 1) = (x, y) of a vector field (the PAF parser's pairing):
//                        e = ax * ax + ay * ay (two products, one sum); if (e > m2) m2 = e; at the end m = sqrt(m2), correctly rounded
//    then t = m * gain; t = t < 1.f ? t : 1.f; q = (int)rintf(t * 255.f).  gain is finite and > 0.
// 2. Taps (host, double).  The frame covers the fraction `cover` in (0, 1] of the m cells of one axis (iw / (double)dw of hp_letterbox_inner for a
//    letter-boxed slot, 1 for a plain resize).  For U upright pixels: scale = (cover * m) / U, s = (u + 0.5) * scale - 0.5; s < 0: {0, 0, 0}; else
//    i = floor(s): { min(i, m - 1), min(i + 1, m - 1), (int)nearbyint((s - i) * 2048) } - the half-pixel convention of the parser's up-sampling.
// 3. Pixel index (int32).  Column tap (x0, x1, wx), row tap (y0, y1, wy), plane p:  top = p[y0][x0] * (2048 - wx) + p[y0][x1] * wx, bot likewise on
//    row y1, idx = (top * (2048 - wy) + bot * wy + (1 << 21)) >> 22, in [0, 255]; top <= 255 * 2^11 and the sum <= 255 * 2^22 + 2^21 < 2^31.
// 4. Geometry.  roi in stored pixels inside the frame (none: the whole frame).  With hp_orient::axes_of(code) and stored pixel (lx, ly) local to a
//    w x h roi: a = flip_x ? w - 1 - lx : lx, b = flip_y ? h - 1 - ly : ly, (ux, uy) = swap ? (b, a) : (a, b).  The x table has swap ? h : w entries
//    over mw with cover_x, the y table the other count over mh with cover_y.  Pixels outside the roi have no index.
// 5. Palette.  256 entries (R, G, B, A) in [0, 255]; palette_entry() gives the built-in ones (float64, t = i / 255, nearbyint(255 * clamp(c))).  A YUV
//    frame takes each entry through hp_yuv::colour_of (yuv_colour.hpp) at the frame's matrix, range and depth (SDR formulas; 10-bit frames at depth 10).
// 6. Samples.  W = nearbyint(opacity * 256), opacity in (0, 1]; a pixel's weight w = (W * A[idx] + 127) / 255.  A B / G / R or luma sample with w > 0
//    becomes (c * w + old * (256 - w) + 128) >> 8 on code values (P010: word >> 6, stored << 6; I010: & 1023).  A chroma sample covers 1 x 1, 2 x 1 or
//    2 x 2 pixels and takes the LARGEST idx among those of its pixels that lie in the roi (equal idx = equal colour); U and V are blended with that
//    idx's weight.  Weight 0, or no pixel in the roi: the sample keeps its value.  No byte outside the roi's samples is read or written.
#pragma once
#include <cmath>
#include <stdint.h>

#include "orientation.hpp"
#include "part_points.hpp"
#include "yuv_colour.hpp"
#include "yuv_formats.hpp"

#if defined(__HIPCC__)
#define HP_MV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HP_MV_HD inline
#endif

namespace hp_mv {

using hp_pts::MAX_DIM;
constexpr int ONE = 2048;             // a tap's weight is in [0, ONE]
constexpr int MAX_MAP_SIDE = 65535;   // a packed tap holds its first cell in 16 bits
constexpr int MAX_MAP_CELLS = 1 << 24;

// ---- 1. index plane ---------------------------------------------------------------------------------------------------------------------------

HP_MV_HD float root_rn(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsqrt_rn(v);
#else
    return std::sqrt(v);
#endif
}

// `maps`: the frame's [C][cells]; the channel choice has been checked against C
HP_MV_HD int index_of(const float* maps, int cells, int cell, int c0, int cn, int c_step, int mode, float gain)
{
    float m = 0.f;
    if (mode == HP_MAPVIEW_MAX) {
        for (int k = 0; k < cn; ++k) {
            const float v = maps[(size_t)(c0 + k * c_step) * cells + cell];
            if (v > m)
                m = v;
        }
    } else {
        float m2 = 0.f;
        for (int k = 0; k < cn; ++k) {
            const float* at = maps + (size_t)(c0 + k * c_step) * cells + cell;
            const float ax = at[0], ay = at[cells];
            const float xx = ax * ax, yy = ay * ay, e = xx + yy;
            if (e > m2)
                m2 = e;
        }
        m = root_rn(m2);
    }
    float t = m * gain;
    t = t < 1.f ? t : 1.f;
    return (int)rintf(t * 255.f);
}

// ---- 2. taps ----------------------------------------------------------------------------------------------------------------------------------

struct tap {
    int32_t i0, i1, w;
};

inline tap tap_of(int u, int U, int m, double cover)
{
    const double scale = (cover * m) / U, s = (u + 0.5) * scale - 0.5;
    if (s < 0)
        return tap{ 0, 0, 0 };
    const double fl = std::floor(s);
    const int i = (int)fl;
    return tap{ i < m - 1 ? i : m - 1, i + 1 < m - 1 ? i + 1 : m - 1, (int)std::nearbyint((s - fl) * (double)ONE) };
}

// a tap as the tables hold it: first cell, whether the second is the next one, the weight
inline uint32_t pack_tap(const tap& t) { return (uint32_t)t.i0 | ((uint32_t)(t.i1 - t.i0) << 16) | ((uint32_t)t.w << 17); }

// ---- 3. pixel index ---------------------------------------------------------------------------------------------------------------------------

HP_MV_HD int pixel_index(const uint8_t* plane, int mw, uint32_t tx, uint32_t ty)
{
    const int x0 = (int)(tx & 0xffffu), x1 = x0 + (int)((tx >> 16) & 1u), wx = (int)(tx >> 17);
    const int y0 = (int)(ty & 0xffffu), y1 = y0 + (int)((ty >> 16) & 1u), wy = (int)(ty >> 17);
    const uint8_t *r0 = plane + (size_t)y0 * mw, *r1 = plane + (size_t)y1 * mw;
    const int top = r0[x0] * (ONE - wx) + r0[x1] * wx, bot = r1[x0] * (ONE - wx) + r1[x1] * wx;
    return (top * (ONE - wy) + bot * wy + (1 << 21)) >> 22;
}

// ---- 5. palettes ------------------------------------------------------------------------------------------------------------------------------

inline void palette_entry(int kind, int alpha_mode, int i, int32_t out[4])
{
    auto clamp = [](double c) { return c < 0. ? 0. : c > 1. ? 1. : c; };
    const double t = i / 255.;
    double r, g, b;
    if (kind == HP_MAPVIEW_JET)
        r = clamp(1.5 - std::fabs(4. * t - 3.)), g = clamp(1.5 - std::fabs(4. * t - 2.)), b = clamp(1.5 - std::fabs(4. * t - 1.));
    else if (kind == HP_MAPVIEW_HEAT)
        r = clamp(3. * t), g = clamp(3. * t - 1.), b = clamp(3. * t - 2.);
    else
        r = g = b = clamp(t);
    out[0] = (int32_t)std::nearbyint(255. * r), out[1] = (int32_t)std::nearbyint(255. * g), out[2] = (int32_t)std::nearbyint(255. * b);
    out[3] = alpha_mode == HP_MAPVIEW_ALPHA_SCALED ? i : 255;
}

// ---- 6. samples -------------------------------------------------------------------------------------------------------------------------------

inline int opacity_weight(float opacity) { return (int)std::nearbyint((double)opacity * 256.); }
HP_MV_HD int weight_of(int W, int A) { return (W * A + 127) / 255; }
HP_MV_HD int blend(int c, int old, int w) { return (c * w + old * (256 - w) + 128) >> 8; }

// one palette entry as the painters read it: the three samples of the frame's kind (B, G, R or Y, U, V), 10 bits each, and the entry's weight
struct entry {
    uint32_t c, w;
};
inline entry pack_entry(int c0, int c1, int c2, int w) { return entry{ (uint32_t)c0 | ((uint32_t)c1 << 10) | ((uint32_t)c2 << 20), (uint32_t)w }; }

// ---- what a call paints: the same description for the kernels (device pointers) and the host twin (host pointers) ---------------------------------

struct view {
    const entry* pal;      // [256]
    const uint32_t* xtab;  // packed taps over mw, one per upright x of the roi
    const uint32_t* ytab;  // packed taps over mh, one per upright y
    const uint8_t* plane;  // the index plane [mh][mw]
    int mw;
    int rx, ry, rw, rh;    // the roi, stored pixels
    int swap, flip_x, flip_y;
};

struct target {
    int bgr;
    int sx, sy, sample_bytes, shift, planes;
    uint8_t* base; // BGR
    int stride;
    hp_yuv::sample_map map;
};

inline void describe_bgr(target& f, uint8_t* bgr, int stride)
{
    f = target();
    f.bgr = 1, f.sample_bytes = 1, f.planes = 1, f.base = bgr, f.stride = stride;
}

// the image has been validated
inline void describe_yuv(target& f, const hp_yuv_image& im)
{
    const hp_yuv::layout& l = *hp_yuv::layout_of(im.format);
    f = target();
    f.sx = l.sx, f.sy = l.sy, f.sample_bytes = l.sample_bytes, f.shift = l.shift, f.planes = l.planes;
    f.map = hp_yuv::map_samples(im, l);
}

// the host tables of a call: U packed taps of one axis, and the 256 entries of a frame's kind (`im` null: BGR) at W = opacity_weight(opacity)
inline void build_taps(int U, int m, double cover, uint32_t* out)
{
    for (int u = 0; u < U; ++u)
        out[u] = pack_tap(tap_of(u, U, m, cover));
}

inline void build_entries(const hp_yuv_image* im, const int32_t (*palette)[4], int W, entry* out)
{
    for (int i = 0; i < 256; ++i) {
        const int w = weight_of(W, palette[i][3]);
        if (!im) {
            out[i] = pack_entry(palette[i][2], palette[i][1], palette[i][0], w);
            continue;
        }
        int32_t yuv[3];
        hp_yuv::colour_of(palette[i][0], palette[i][1], palette[i][2], im->matrix, im->range, hp_yuv::layout_of(im->format)->sample_bytes == 2 ? 10 : 8, yuv);
        out[i] = pack_entry(yuv[0], yuv[1], yuv[2], w);
    }
}

// 4. the index of stored pixel (x, y), which lies inside the roi
HP_MV_HD int index_at(const view& v, int x, int y)
{
    const int lx = x - v.rx, ly = y - v.ry;
    const int a = v.flip_x ? v.rw - 1 - lx : lx, b = v.flip_y ? v.rh - 1 - ly : ly;
    const int ux = v.swap ? b : a, uy = v.swap ? a : b;
    return pixel_index(v.plane, v.mw, v.xtab[ux], v.ytab[uy]);
}

// ---- host twin: samples are read and written bytewise (hp_yuv::host_get / host_put) -----------------------------------------------------------------

inline void host_mix(const target& f, uint8_t* q, int c, int w)
{
    hp_yuv::host_put(q, f.sample_bytes, f.shift, blend(c, hp_yuv::host_get(q, f.sample_bytes, f.shift), w));
}

inline void paint_host(const target& f, const view& v)
{
    const int x_end = v.rx + v.rw, y_end = v.ry + v.rh;
    for (int by = v.ry >> f.sy; by <= (y_end - 1) >> f.sy; ++by)
        for (int bx = v.rx >> f.sx; bx <= (x_end - 1) >> f.sx; ++bx) {
            int best = -1;
            for (int dy = 0; dy < (1 << f.sy); ++dy)
                for (int dx = 0; dx < (1 << f.sx); ++dx) {
                    const int x = (bx << f.sx) + dx, y = (by << f.sy) + dy;
                    if (x < v.rx || x >= x_end || y < v.ry || y >= y_end)
                        continue;
                    const int idx = index_at(v, x, y);
                    best = idx > best ? idx : best;
                    const entry e = v.pal[idx];
                    if (e.w == 0)
                        continue;
                    if (f.bgr) {
                        uint8_t* q = f.base + (size_t)y * f.stride + (size_t)x * 3;
                        for (int ch = 0; ch < 3; ++ch)
                            host_mix(f, q + ch, (int)((e.c >> (10 * ch)) & 1023u), (int)e.w);
                    } else
                        host_mix(f, const_cast<uint8_t*>(f.map.y) + (size_t)y * f.map.y_stride + (size_t)x * f.map.y_step, (int)(e.c & 1023u), (int)e.w);
                }
            if (f.bgr || best < 0 || v.pal[best].w == 0)
                continue;
            const entry e = v.pal[best];
            const size_t at = (size_t)by * f.map.c_stride + (size_t)bx * f.map.c_step;
            host_mix(f, const_cast<uint8_t*>(f.map.u) + at, (int)((e.c >> 10) & 1023u), (int)e.w);
            host_mix(f, const_cast<uint8_t*>(f.map.v) + at + (ptrdiff_t)by * f.map.v_extra, (int)((e.c >> 20) & 1023u), (int)e.w);
        }
}

} // namespace hp_mv
