// orientation.hpp — the HP_ORIENT_* code (include/hp_hip.h: code = q + 4 * m, q quarter turns clockwise to upright, m = mirrored left-right first) as the
// three facts every user of it needs, host and device: do the axes swap, and which stored axis runs backwards.  With (ux, uy) an upright pixel of a
// stored sw x sh frame, a = swap ? uy : ux and b = swap ? ux : uy:
//     stored x = flip_x ? sw - 1 - a : a        stored y = flip_y ? sh - 1 - b : b
// which is the header's table with the mirror folded in (the mirror acts on the stored x only, so it toggles flip_x).
// Under a plain C++ compiler the header is pure (no HIP include): mapview.hpp's host rules use it so (tests/cpp/mapview_rules.cpp).
#pragma once
#if defined(__HIPCC__)
#include "hp_common.hpp"
#define HP_ORIENT_HD __host__ __device__ __forceinline__
#else
#define HP_ORIENT_HD inline
#endif

namespace hp_orient {

struct axes {
    int swap, flip_x, flip_y;
};

HP_ORIENT_HD axes axes_of(int code)
{
    const int q = code & 3, m = (code >> 2) & 1;
    return axes{ q & 1, ((q >> 1) & 1) ^ m, (q ^ (q >> 1)) & 1 };
}

inline bool valid(int code) { return code >= 0 && code <= 7; }

} // namespace hp_orient
