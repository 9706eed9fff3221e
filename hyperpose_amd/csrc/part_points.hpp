// part_points.hpp — the ONE statement of where a human's parts lie in a W x H frame, for the units that write into frames (overlay.hip,
// redact.hpp), and of the coordinate limits their integer rules are proved for.  Host only; needs nothing but hp_hip.h and compiles with a plain
// C++ compiler.  fp32 without fused operations (both units are built with -ffp-contract=off; tests/overlay_ref.py and tests/redact_ref.py
// restate it bit for bit).
//
// A part is PRESENT when has_value != 0 and x and y are finite.  Its pixel is (int)(x * (float)W), (int)(y * (float)H) in fp32 - what the
// reference's draw_human computes - and the part is OK (usable as an end point, a centre, a corner) only when both coordinates lie in
// [COORD_MIN, COORD_MAX]: a point outside is more than a frame away from a picture of at most MAX_DIM x MAX_DIM.
#pragma once
#include <cmath>
#include <stdint.h>

#include "../../include/hp_hip.h"

namespace hp_pts {

constexpr int MAX_DIM = 8192;
constexpr int COORD_MIN = -8192, COORD_MAX = 16383;

inline bool present(const hp_body_part& p) { return p.has_value != 0 && std::isfinite(p.x) && std::isfinite(p.y); }

// v = coordinate * size lies inside [COORD_MIN, COORD_MAX] once cast to int
inline bool in_range(float v) { return v > (float)(COORD_MIN - 1) && v < (float)(COORD_MAX + 1); }

// ok[k], and where it holds the pixel (px[k], py[k]), of every part of one human (0, 0 elsewhere)
inline void part_points(const hp_human& hm, int w, int h, int32_t px[HP_COCO_N_PARTS], int32_t py[HP_COCO_N_PARTS], bool ok[HP_COCO_N_PARTS])
{
    const float fw = (float)w, fh = (float)h;
    for (int k = 0; k < HP_COCO_N_PARTS; ++k) {
        const hp_body_part& p = hm.parts[k];
        const float fx = p.x * fw, fy = p.y * fh;
        ok[k] = present(p) && in_range(fx) && in_range(fy);
        px[k] = ok[k] ? (int32_t)fx : 0, py[k] = ok[k] ? (int32_t)fy : 0;
    }
}

} // namespace hp_pts
