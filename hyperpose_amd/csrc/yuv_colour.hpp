// yuv_colour.hpp — one 8-bit R'G'B' colour as the d-bit (Y, U, V) code values of a matrix / range / depth: the formulas hp_yuv_colours states
// (include/hp_hip.h), float64 then nearbyint, clipped to [0, 2^d - 1].  Shared by the units that paint colours into YUV frames: the overlay's 19
// skeleton colours (overlay.hip) and the map view's palettes (mapview.hpp); the encoder hand-off (to_yuv.hpp) takes its luma weights from here.
// Host only and pure: <cmath> and hp_hip.h's constants.
#pragma once
#include <algorithm>
#include <cmath>
#include <stdint.h>

#include "../../include/hp_hip.h"

namespace hp_yuv {

// the luma weights of HP_YUV_BT601, _BT709, _BT2020 (kg = 1 - kr - kb); to_yuv.hpp derives the forward integer table from the same numbers
constexpr double KR[3] = { 0.299, 0.2126, 0.2627 }, KB[3] = { 0.114, 0.0722, 0.0593 };

// r, g, b in [0, 255]; matrix, range and depth (8 or 10) have been checked
inline void colour_of(int r8, int g8, int b8, int matrix, int range, int depth, int32_t out[3])
{
    const double kr = KR[matrix], kb = KB[matrix], kg = 1. - kr - kb;
    const double top = (double)((1 << depth) - 1), up = (double)(1 << (depth - 8)), half = (double)(1 << (depth - 1));
    auto clip = [&](double v) { return (int32_t)std::min(top, std::max(0., std::nearbyint(v))); };
    const double r = r8 / 255., g = g8 / 255., b = b8 / 255.;
    const double y = kr * r + kg * g + kb * b, cb = (b - y) / (2. * (1. - kb)), cr = (r - y) / (2. * (1. - kr));
    if (range == HP_YUV_LIMITED)
        out[0] = clip((16. + 219. * y) * up), out[1] = clip((128. + 224. * cb) * up), out[2] = clip((128. + 224. * cr) * up);
    else
        out[0] = clip(y * top), out[1] = clip(half + cb * top), out[2] = clip(half + cr * top);
}

} // namespace hp_yuv
