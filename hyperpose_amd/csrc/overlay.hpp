// overlay.hpp — the ONE statement of the picture hp_overlay_draw_* paints (include/hp_hip.h): which pixels a skeleton covers, which colour a
// covered sample takes and how it is blended.  Shared by the kernels and the host twins (overlay.hip) and quoted by DESIGN.md 1.1; the
// tests restate it in numpy with Python integers (tests/overlay_ref.py).  Everything here is exact integer arithmetic, so the GPU, the
// host twin and the tests agree byte for byte - the float capsule test of hyperpose::detail::capsule (include/hyperpose/utility/human.hpp)
// depends on contraction and rounding and cannot be held to that.
//
// Primitive list (build_primitives, host only, fp32 without fused operations).  For a W x H frame and humans h = 0..n-1 in order, each human
// contributes its limbs pair_id = 0..18 (COCO_PAIRS, colour pair_id), each where both parts are present, as a CAPSULE, then its parts 0..17
// (colour = part index), each present one, as a DISC.  A part is present when has_value != 0 and x and y are finite.  End points and centres
// are int(p.x * W), int(p.y * H) in fp32 - what draw_human computes (hp_pts::part_points, part_points.hpp, states both).  Thickness T = the caller's `thickness` when > 0, else the reference's rule
// (src/human.cpp:7-39) per human: T = max(1, int(sqrtf((e - w) * (s - n) * (W * H))) / 32) over the present parts, n = min(1, y..), s = max(0, y..),
// w = min(1, x..), e = max(0, x..); the square root is capped at 32 * MAX_T before the cast, so T <= MAX_T.
//
// Range limit (the constants: part_points.hpp).  W, H <= MAX_DIM = 8192.  A primitive with an end point outside [COORD_MIN, COORD_MAX] = [-8192, 16383] is dropped: such a point
// is more than a frame away from the picture.  With pixels in [0, 8191] every difference below is at most 24575 < 2^14.6 in magnitude, so
// |cross| < 2^30.2, 4 * cross^2 < 2^62.4 < 2^63, and T^2 * L <= 2^28 * 2^30.2 < 2^63: everything fits signed 64 bits.
//
// Coverage of pixel (x, y), int64 throughout.  p = (x - x0, y - y0), d = (x1 - x0, y1 - y0), L = d.d, s = p.d.
//   capsule   L == 0 or s <= 0:  4 (p.p) <= T^2          s >= L:  4 ((p - d).(p - d)) <= T^2          else:  4 (p.x d.y - p.y d.x)^2 <= T^2 L
//   disc      (x - cx)^2 + (y - cy)^2 <= T^2
// the geometry of detail::capsule / detail::disc (half-width T / 2, radius T) without the float rounding.  Every covered pixel lies within T of
// the segment's bounding box in both axes: reach() below is what the culling and the host loops use.
//
// Painter's order: a covered pixel takes the colour of the LAST primitive in list order that covers it.  A chroma sample covers 1 x 1, 2 x 1 or
// 2 x 2 luma pixels; it is written when ANY of them is covered and takes the colour of the primitive with the highest list index among those
// that cover any of its pixels.  A sample that no primitive covers is not written (and not read).
//
// Blend: w = nearbyint(opacity * 256) in [0, 256] for opacity in (0, 1]; a written sample is (c * w + old * (256 - w) + 128) >> 8 at 8 or 10 bits;
// w == 256 writes c and does not read; w == 0 (opacity below 1 / 512) writes every covered sample back as it was.  P010 stores value << 6 (low six bits zero, the old value is word >> 6), I010 stores the value (high six bits zero).
#pragma once
#include <stdint.h>

#include "part_points.hpp"

#if defined(__HIPCC__)
#define HP_OVL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HP_OVL_HD inline
#endif

namespace hp_ovl {

using hp_pts::COORD_MAX;
using hp_pts::COORD_MIN;
using hp_pts::MAX_DIM;
constexpr int MAX_T = 16384;
constexpr int PRIMS_PER_HUMAN = HP_COCO_N_PAIRS + HP_COCO_N_PARTS; // 37
constexpr int KIND_CAPSULE = 0, KIND_DISC = 1;

// limb table and colours of include/hyperpose/utility/human.hpp:55-59 (src/coco.hpp:32-51, src/color.hpp:16-36)
constexpr int COCO_PAIRS[HP_COCO_N_PAIRS][2] = { { 1, 2 }, { 1, 5 }, { 2, 3 }, { 3, 4 }, { 5, 6 }, { 6, 7 }, { 1, 8 }, { 8, 9 }, { 9, 10 }, { 1, 11 },
    { 11, 12 }, { 12, 13 }, { 1, 0 }, { 0, 14 }, { 14, 16 }, { 0, 15 }, { 15, 17 }, { 2, 16 }, { 5, 17 } };
constexpr uint8_t COCO_COLOURS_RGB[19][3] = { { 255, 0, 0 }, { 255, 85, 0 }, { 255, 170, 0 }, { 255, 255, 0 }, { 170, 255, 0 }, { 85, 255, 0 }, { 0, 255, 0 },
    { 0, 255, 85 }, { 0, 255, 170 }, { 0, 255, 255 }, { 0, 170, 255 }, { 0, 85, 255 }, { 0, 0, 255 }, { 85, 0, 255 }, { 170, 0, 255 }, { 255, 0, 255 },
    { 255, 0, 170 }, { 255, 0, 85 }, { 127, 127, 127 } };

HP_OVL_HD bool covers(int kind, int x0, int y0, int x1, int y1, int t, int x, int y)
{
    const int64_t px = x - x0, py = y - y0, tt = (int64_t)t * t;
    if (kind == KIND_DISC)
        return px * px + py * py <= tt;
    const int64_t dx = x1 - x0, dy = y1 - y0, L = dx * dx + dy * dy, s = px * dx + py * dy;
    if (L == 0 || s <= 0)
        return 4 * (px * px + py * py) <= tt;
    if (s >= L) {
        const int64_t qx = px - dx, qy = py - dy;
        return 4 * (qx * qx + qy * qy) <= tt;
    }
    const int64_t cross = px * dy - py * dx;
    return 4 * cross * cross <= tt * L;
}

// the rectangle [lo_x, hi_x] x [lo_y, hi_y] outside which a primitive covers nothing
HP_OVL_HD void reach(int x0, int y0, int x1, int y1, int t, int& lo_x, int& lo_y, int& hi_x, int& hi_y)
{
    lo_x = (x0 < x1 ? x0 : x1) - t, hi_x = (x0 < x1 ? x1 : x0) + t;
    lo_y = (y0 < y1 ? y0 : y1) - t, hi_y = (y0 < y1 ? y1 : y0) + t;
}

HP_OVL_HD int blend(int c, int old, int w) { return (c * w + old * (256 - w) + 128) >> 8; }

} // namespace hp_ovl
