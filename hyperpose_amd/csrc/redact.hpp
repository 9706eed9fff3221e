// redact.hpp — the ONE statement of the picture hp_redact_* leaves behind (include/hp_hip.h): which regions a frame's humans give, which cells
// of the frame a region reaches and what a reached cell becomes.  Shared by the kernels and the host twins (redact.hip) and quoted by DESIGN.md
// 1.1 "Redaction"; the tests restate it in numpy with Python integers (tests/redact_ref.py).  Everything past the part points is exact integer
// arithmetic, so the GPU, the host twin and the tests agree byte for byte.  The host side (everything but the kernels) needs nothing but
// hp_hip.h and the two pure headers beside it - part_points.hpp (the part-point rule and the coordinate limits) and yuv_formats.hpp (the layouts) -
// and compiles with a plain C++ compiler: tests/cpp/redact_rules.cpp runs it under sanitizers on planes allocated with no slack.
//
// Regions.  RECT covers the pixels of [x0, x1] x [y0, y1], inclusive (x0 <= x1, y0 <= y1); DISC has centre (x0, y0) and radius x1 >= 0, y1 == 0.
// Coordinates lie in [COORD_MIN, COORD_MAX] = [-8192, 16383] (part_points.hpp) and radii in [0, MAX_R = 16384] - the overlay's ranges - so with
// pixels in [0, 8191] every difference is below 2^15 in magnitude and every sum of two squares below 2^31: int64 holds all of it.
//
// Region list (build_regions, host only, fp32 without fused operations).  A part's point, and whether it counts ("present" below), is
// hp_pts::part_points' px, py and ok (part_points.hpp): has_value != 0, x and y finite, both coordinates in [COORD_MIN, COORD_MAX].
// m = nearbyint(margin * 256) for margin in (0, 8].  Per human, in order:
//   head disc   F = the present parts among {0, 14, 15, 16, 17} (nose, eyes, ears); none: no disc.  lo, hi = the bounding box of F; centre
//               (floor((lo_x + hi_x) / 2), floor((lo_y + hi_y) / 2)); e = max(hi_x - lo_x, hi_y - lo_y); nk = isqrt(|p1 - p0|^2) when neck and
//               nose are present, else 0; sh = isqrt(|p2 - p5|^2) >> 1 when both shoulders are, else 0 (isqrt: floor square root on int64);
//               b = max(e, nk, sh, 1); r = min(16384, max(1, (b * m + 128) >> 8)).
//   HEAD        the disc and nothing else.
//   BODY        first a RECT: lo, hi over ALL present parts (none: no RECT), p = max(1, (max(hi_x - lo_x, hi_y - lo_y) * m + 1024) >> 11), the
//               rectangle [lo - p, hi + p] clamped into [COORD_MIN, COORD_MAX]; then the head disc if there is one.
//
// Cells.  `cell` is even, 2 .. 128; the grid is anchored at pixel (0, 0); cell (i, j) owns the pixel columns [i * cell, min(W, (i + 1) * cell) - 1]
// and the rows likewise (edge cells are partial).  Since cell is even every chroma sample and every YUY2 / UYVY macropixel lies in one cell.
// A cell [X0, X1] x [Y0, Y1] is HIT when any region reaches it: RECT when the rectangles intersect; DISC when, with dx = x0 - clamp(x0, X0, X1)
// and dy = y0 - clamp(y0, Y0, Y1), dx * dx + dy * dy <= r * r (int64).  The regions form a union: order and overlap do not matter.
//
// Effect.  A hit cell is rewritten whole, every sample of every plane inside it; nothing else of the frame is written (row padding included) and no
// byte outside the planes' picture rows is read.  PIXELATE: each channel (B, G, R; Y, U, V) of the cell becomes (sum + cnt / 2) / cnt over that
// channel's samples in the cell - for U and V the chroma samples the cell owns - on code values (P010 reads word >> 6 and stores mean << 6, I010
// reads word & 1023); sum <= 128 * 128 * 1023 < 2^24 needs int32.  BLACK: BGR (0, 0, 0); YUV Y = 16 << (d - 8) in limited range and 0 in full
// range, U = V = 1 << (d - 1), in the layout's stored form.
//
// How a frame is walked (host twin and kernel alike): a frame is up to three SPANS, one per memory plane.  A span's rows hold `k` samples per
// chroma block column - BGR 3, a Y / U / V plane 1, an interleaved UV plane 2, a YUY2 / UYVY row 4 per macropixel - and sample j of a row belongs
// to channel pat[j % k].  Cell (i, j) owns of a span the rows [Y0 >> sy, Y1 >> sy] and the samples [(X0 >> sx) * k, ((X1 >> sx) + 1) * k).
#pragma once
#include <cmath>
#include <stdint.h>

#include "part_points.hpp"
#include "yuv_formats.hpp"

#if defined(__HIPCC__)
#define HP_RED_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HP_RED_HD inline
#endif

namespace hp_red {

using hp_pts::COORD_MAX;
using hp_pts::COORD_MIN;
using hp_pts::MAX_DIM;
constexpr int MAX_R = 16384;
constexpr int MIN_CELL = 2, MAX_CELL = 128;
constexpr int FACE_PARTS[5] = { 0, 14, 15, 16, 17 };

// ---- coverage -----------------------------------------------------------------------------------------------------------------------------

HP_RED_HD bool hits(const hp_redact_region& g, int X0, int Y0, int X1, int Y1)
{
    if (g.kind == HP_REDACT_RECT)
        return g.x0 <= X1 && g.x1 >= X0 && g.y0 <= Y1 && g.y1 >= Y0;
    const int cx = g.x0 < X0 ? X0 : g.x0 > X1 ? X1 : g.x0, cy = g.y0 < Y0 ? Y0 : g.y0 > Y1 ? Y1 : g.y0;
    const int64_t dx = g.x0 - cx, dy = g.y0 - cy, r = g.x1;
    return dx * dx + dy * dy <= r * r;
}

// the rectangle outside which a region reaches no pixel
HP_RED_HD void reach(const hp_redact_region& g, int& lo_x, int& lo_y, int& hi_x, int& hi_y)
{
    if (g.kind == HP_REDACT_RECT)
        lo_x = g.x0, lo_y = g.y0, hi_x = g.x1, hi_y = g.y1;
    else
        lo_x = g.x0 - g.x1, lo_y = g.y0 - g.x1, hi_x = g.x0 + g.x1, hi_y = g.y0 + g.x1;
}

inline bool coord_ok(int v) { return v >= COORD_MIN && v <= COORD_MAX; }

// nullptr, or what is wrong with the region
inline const char* region_fault(const hp_redact_region& g)
{
    if (g.kind == HP_REDACT_RECT) {
        if (!(coord_ok(g.x0) && coord_ok(g.y0) && coord_ok(g.x1) && coord_ok(g.y1)))
            return "a rectangle's corner outside [-8192, 16383]";
        return g.x0 <= g.x1 && g.y0 <= g.y1 ? nullptr : "a rectangle with x0 > x1 or y0 > y1";
    }
    if (g.kind == HP_REDACT_DISC) {
        if (!(coord_ok(g.x0) && coord_ok(g.y0)))
            return "a disc's centre outside [-8192, 16383]";
        if (g.x1 < 0 || g.x1 > MAX_R)
            return "a disc's radius outside [0, 16384]";
        return g.y1 == 0 ? nullptr : "a disc with y1 != 0";
    }
    return "an unknown kind";
}

inline bool cell_ok(int cell) { return cell >= MIN_CELL && cell <= MAX_CELL && (cell & 1) == 0; }
inline bool margin_ok(float margin) { return margin > 0.f && margin <= 8.f; }

// the cells the list can reach, clipped to the frame (inclusive): false when there are none
inline bool cell_rect(const hp_redact_region* regs, int n, int w, int h, int cell, int& cx0, int& cy0, int& cx1, int& cy1)
{
    int x0 = w, y0 = h, x1 = -1, y1 = -1;
    for (int i = 0; i < n; ++i) {
        int lx, ly, hx, hy;
        reach(regs[i], lx, ly, hx, hy);
        if (hx < 0 || hy < 0 || lx >= w || ly >= h)
            continue;
        x0 = x0 < lx ? x0 : lx < 0 ? 0 : lx, y0 = y0 < ly ? y0 : ly < 0 ? 0 : ly;
        x1 = x1 > hx ? x1 : hx > w - 1 ? w - 1 : hx, y1 = y1 > hy ? y1 : hy > h - 1 ? h - 1 : hy;
    }
    if (x1 < x0 || y1 < y0)
        return false;
    cx0 = x0 / cell, cy0 = y0 / cell, cx1 = x1 / cell, cy1 = y1 / cell;
    return true;
}

// ---- the region list ------------------------------------------------------------------------------------------------------------------------

inline int64_t isqrt(int64_t v)
{
    int64_t r = (int64_t)std::sqrt((double)v);
    while (r * r > v)
        --r;
    while ((r + 1) * (r + 1) <= v)
        ++r;
    return r;
}

// the bounding box of the points added so far
struct box {
    int lx = 0, ly = 0, hx = 0, hy = 0;
    bool any = false;
    void add(int x, int y)
    {
        lx = any && lx < x ? lx : x, hx = any && hx > x ? hx : x;
        ly = any && ly < y ? ly : y, hy = any && hy > y ? hy : y;
        any = true;
    }
    int longer_side() const { return hx - lx > hy - ly ? hx - lx : hy - ly; }
};

inline int clamp_coord(int64_t v) { return (int)(v < COORD_MIN ? COORD_MIN : v > COORD_MAX ? COORD_MAX : v); }

// returns the count; writes at most cap entries.  The arguments have been checked (w, h in 1 .. MAX_DIM, what, margin).
inline int build_regions(const hp_human* humans, int n, int w, int h, int what, float margin, hp_redact_region* out, int cap)
{
    const int64_t m = (int64_t)std::nearbyint((double)margin * 256.);
    int count = 0;
    auto emit = [&](const hp_redact_region& g) {
        if (count < cap)
            out[count] = g;
        ++count;
    };
    for (int i = 0; i < n; ++i) {
        int32_t px[HP_COCO_N_PARTS], py[HP_COCO_N_PARTS];
        bool ok[HP_COCO_N_PARTS];
        hp_pts::part_points(humans[i], w, h, px, py, ok);
        if (what == HP_REDACT_BODY) {
            box all;
            for (int k = 0; k < HP_COCO_N_PARTS; ++k)
                if (ok[k])
                    all.add(px[k], py[k]);
            if (all.any) {
                const int64_t grown = ((int64_t)all.longer_side() * m + 1024) >> 11, p = grown > 1 ? grown : 1;
                emit(hp_redact_region{ HP_REDACT_RECT, clamp_coord(all.lx - p), clamp_coord(all.ly - p), clamp_coord(all.hx + p), clamp_coord(all.hy + p), i });
            }
        }
        box face;
        for (int k : FACE_PARTS)
            if (ok[k])
                face.add(px[k], py[k]);
        if (!face.any)
            continue;
        auto dist = [&](int a, int b) {
            const int64_t dx = px[a] - px[b], dy = py[a] - py[b];
            return isqrt(dx * dx + dy * dy);
        };
        int64_t b = face.longer_side();
        const int64_t nk = ok[1] && ok[0] ? dist(1, 0) : 0, sh = ok[2] && ok[5] ? dist(2, 5) >> 1 : 0;
        b = b > nk ? b : nk, b = b > sh ? b : sh, b = b > 1 ? b : 1;
        int64_t r = (b * m + 128) >> 8;
        r = r < 1 ? 1 : r > MAX_R ? MAX_R : r;
        emit(hp_redact_region{ HP_REDACT_DISC, (face.lx + face.hx) >> 1, (face.ly + face.hy) >> 1, (int32_t)r, 0, i }); // >> 1 of a negative sum: the floor
    }
    return count;
}

// ---- a frame as spans ---------------------------------------------------------------------------------------------------------------------------

struct span {
    uint8_t* base;
    int stride;  // bytes between rows
    int sx, sy;  // pixel (x, y) lies in chroma block column x >> sx, row y >> sy of this span
    int k;       // samples per chroma block column: 1, 2, 3 or 4
    int pat;     // channel of sample q of a block, two bits each: (pat >> 2 * q) & 3
};

struct frame {
    int w = 0, h = 0;
    int n_spans = 0;
    span s[3];
    int sample_bytes = 1, shift = 0; // 16-bit little-endian words: value = (word >> shift) & 1023, stored as value << shift
    int black[3] = { 0, 0, 0 };      // what HP_REDACT_BLACK writes, per channel
};

inline void describe_bgr(frame& f, uint8_t* bgr, int w, int h, int stride)
{
    f = frame();
    f.w = w, f.h = h, f.n_spans = 1;
    f.s[0] = span{ bgr, stride, 0, 0, 3, 0 | (1 << 2) | (2 << 4) };
}

// The image has been validated.  One span per memory plane, from the layout's entry and its sample map (yuv_formats.hpp): a block of a plane
// is what lies between two chroma samples of it (a luma plane: between two luma samples), and a sample's channel is read off where the map
// puts the first Y (and every y_step bytes after it), U and V sample - no format is named here.
inline void describe_yuv(frame& f, const hp_yuv_image& im)
{
    const hp_yuv::layout& l = *hp_yuv::layout_of(im.format);
    const hp_yuv::sample_map m = hp_yuv::map_samples(im, l);
    const int sb = l.sample_bytes;
    const bool packed = l.planes == 1;
    f = frame();
    f.w = im.width, f.h = im.height, f.sample_bytes = sb, f.shift = l.shift, f.n_spans = l.planes;
    f.s[0] = span{ (uint8_t*)im.plane[0], im.stride[0], packed ? l.sx : 0, packed ? l.sy : 0, (packed ? m.c_step : m.y_step) / sb, 0 };
    for (int k = 1; k < l.planes; ++k)
        f.s[k] = span{ (uint8_t*)im.plane[k], im.stride[k], l.sx, l.sy, m.c_step / sb, 0 };
    auto mark = [&](span& s, const uint8_t* at, int channel) {
        const int q = (int)(at - s.base) / sb;
        s.pat = (s.pat & ~(3 << (2 * q))) | (channel << (2 * q));
    };
    for (int at = 0; at < f.s[0].k * sb; at += m.y_step)
        mark(f.s[0], m.y + at, 0);
    mark(f.s[l.planes > 1], m.u, 1), mark(f.s[l.planes - 1], m.v, 2);
    const int d = sb == 2 ? 10 : 8;
    f.black[0] = im.range == HP_YUV_LIMITED ? 16 << (d - 8) : 0, f.black[1] = f.black[2] = 1 << (d - 1);
}

// what cell (ci, cj) owns of span s: rows [r0, r1] and samples [j0, j1) of each
HP_RED_HD void cell_of_span(const span& s, int X0, int Y0, int X1, int Y1, int& r0, int& r1, int& j0, int& j1)
{
    r0 = Y0 >> s.sy, r1 = Y1 >> s.sy;
    j0 = (X0 >> s.sx) * s.k, j1 = ((X1 >> s.sx) + 1) * s.k;
}

// sample j of a row (j counted from a block boundary) belongs to this channel
HP_RED_HD int channel_of(const span& s, int j)
{
    const int q = s.k == 3 ? j - 3 * (int)(((unsigned)j * 43691u) >> 17) : j & (s.k - 1); // j / 3 for j < 2^16
    return (s.pat >> (2 * q)) & 3;
}

// ---- host twin ----------------------------------------------------------------------------------------------------------------------------------

// the arguments have been checked (regions, effect, cell); samples are read and written bytewise (hp_yuv::host_get / host_put)
inline void paint_host(const frame& f, const hp_redact_region* regs, int n, int effect, int cell)
{
    int cx0, cy0, cx1, cy1;
    if (n == 0 || !cell_rect(regs, n, f.w, f.h, cell, cx0, cy0, cx1, cy1))
        return;
    for (int cj = cy0; cj <= cy1; ++cj)
        for (int ci = cx0; ci <= cx1; ++ci) {
            const int X0 = ci * cell, Y0 = cj * cell, X1 = (X0 + cell < f.w ? X0 + cell : f.w) - 1, Y1 = (Y0 + cell < f.h ? Y0 + cell : f.h) - 1;
            bool hit = false;
            for (int i = 0; i < n && !hit; ++i)
                hit = hits(regs[i], X0, Y0, X1, Y1);
            if (!hit)
                continue;
            int32_t value[3] = { f.black[0], f.black[1], f.black[2] };
            if (effect == HP_REDACT_PIXELATE) {
                int32_t sum[3] = { 0, 0, 0 }, cnt[3] = { 0, 0, 0 };
                for (int k = 0; k < f.n_spans; ++k) {
                    int r0, r1, j0, j1;
                    cell_of_span(f.s[k], X0, Y0, X1, Y1, r0, r1, j0, j1);
                    for (int r = r0; r <= r1; ++r)
                        for (int j = j0; j < j1; ++j) {
                            const int c = channel_of(f.s[k], j);
                            sum[c] += hp_yuv::host_get(f.s[k].base + (size_t)r * f.s[k].stride + (size_t)j * f.sample_bytes, f.sample_bytes, f.shift), ++cnt[c];
                        }
                }
                for (int c = 0; c < 3; ++c)
                    value[c] = cnt[c] ? (sum[c] + cnt[c] / 2) / cnt[c] : 0;
            }
            for (int k = 0; k < f.n_spans; ++k) {
                int r0, r1, j0, j1;
                cell_of_span(f.s[k], X0, Y0, X1, Y1, r0, r1, j0, j1);
                for (int r = r0; r <= r1; ++r)
                    for (int j = j0; j < j1; ++j)
                        hp_yuv::host_put(f.s[k].base + (size_t)r * f.s[k].stride + (size_t)j * f.sample_bytes, f.sample_bytes, f.shift, value[channel_of(f.s[k], j)]);
            }
        }
}

} // namespace hp_red
