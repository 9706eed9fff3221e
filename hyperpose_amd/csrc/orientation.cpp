// orientation.cpp — the host side of HP_ORIENT_* (include/hp_hip.h): sizes, the EXIF table, regions, the materialised upright BGR frame (the
// definition the oriented resize calls are tested against, and the fallback of a caller without a device) and the humans' way between the
// upright and the stored frame.  Plain C++, no device; the human formulas are fp32 exactly as the header writes them (no fused operations:
// this unit is built with -ffp-contract=off), tests/orient_ref.py restates all of it in numpy.
#include "orientation.hpp"

extern "C" {

int hp_oriented_size(int orientation, int sw, int sh, int* uw, int* uh)
{
    HP_REQUIRE(hp_orient::valid(orientation), HP_ERR_INVALID, "hp_oriented_size: orientation %d is no HP_ORIENT_* code (0 .. 7)", orientation);
    HP_REQUIRE(sw > 0 && sh > 0, HP_ERR_INVALID, "hp_oriented_size: empty stored frame (%d x %d)", sw, sh);
    HP_REQUIRE(uw && uh, HP_ERR_INVALID, "hp_oriented_size: null output");
    const bool turned = (orientation & 1) != 0;
    *uw = turned ? sh : sw, *uh = turned ? sw : sh;
    return HP_OK;
}

int hp_orientation_from_exif(int exif)
{
    static const int code[8] = { HP_ORIENT_NONE, HP_ORIENT_HFLIP, HP_ORIENT_180, HP_ORIENT_HFLIP_180, HP_ORIENT_HFLIP_CW270, HP_ORIENT_CW90,
        HP_ORIENT_HFLIP_CW90, HP_ORIENT_CW270 };
    HP_REQUIRE(exif >= 1 && exif <= 8, HP_ERR_INVALID, "hp_orientation_from_exif: exif orientation %d (1 .. 8)", exif);
    return code[exif - 1];
}

int hp_orient_roi(const hp_roi* upright, int orientation, int sw, int sh, hp_roi* stored)
{
    HP_REQUIRE(upright && stored, HP_ERR_INVALID, "hp_orient_roi: null argument");
    int uw = 0, uh = 0;
    HP_TRY(hp_oriented_size(orientation, sw, sh, &uw, &uh));
    const hp_roi u = *upright;
    HP_REQUIRE(u.w > 0 && u.h > 0 && u.x >= 0 && u.y >= 0 && (int64_t)u.x + u.w <= uw && (int64_t)u.y + u.h <= uh, HP_ERR_INVALID,
        "hp_orient_roi: upright region (%d x %d at %d, %d) is empty or not inside the %d x %d upright frame", u.w, u.h, u.x, u.y, uw, uh);
    const hp_orient::axes m = hp_orient::axes_of(orientation);
    // along each stored axis the region keeps its extent and starts at its first upright coordinate, or ends there when the axis runs backwards
    const int a = m.swap ? u.y : u.x, aw = m.swap ? u.h : u.w, b = m.swap ? u.x : u.y, bh = m.swap ? u.w : u.h;
    stored->x = m.flip_x ? sw - a - aw : a, stored->w = aw;
    stored->y = m.flip_y ? sh - b - bh : b, stored->h = bh;
    return HP_OK;
}

int hp_orient_u8c3_host(const uint8_t* src, int sw, int sh, int src_stride, int orientation, uint8_t* dst, int dst_stride)
{
    int uw = 0, uh = 0;
    HP_TRY(hp_oriented_size(orientation, sw, sh, &uw, &uh));
    HP_REQUIRE(src && dst, HP_ERR_INVALID, "hp_orient_u8c3_host: null frame");
    HP_REQUIRE(src_stride >= sw * 3, HP_ERR_INVALID, "hp_orient_u8c3_host: src_stride %d is smaller than a stored row (%d bytes)", src_stride, sw * 3);
    HP_REQUIRE(dst_stride >= uw * 3, HP_ERR_INVALID, "hp_orient_u8c3_host: dst_stride %d is smaller than an upright row (%d bytes)", dst_stride, uw * 3);
    const hp_orient::axes m = hp_orient::axes_of(orientation);
    for (int uy = 0; uy < uh; ++uy)
        for (int ux = 0; ux < uw; ++ux) {
            const int a = m.swap ? uy : ux, b = m.swap ? ux : uy;
            const uint8_t* s = src + (size_t)(m.flip_y ? sh - 1 - b : b) * src_stride + (size_t)(m.flip_x ? sw - 1 - a : a) * 3;
            uint8_t* d = dst + (size_t)uy * dst_stride + (size_t)ux * 3;
            d[0] = s[0], d[1] = s[1], d[2] = s[2];
        }
    return HP_OK;
}

int hp_humans_orient(hp_human* humans, int n, int orientation, int to_stored)
{
    HP_REQUIRE(hp_orient::valid(orientation), HP_ERR_INVALID, "hp_humans_orient: orientation %d is no HP_ORIENT_* code (0 .. 7)", orientation);
    HP_REQUIRE(n >= 0, HP_ERR_INVALID, "hp_humans_orient: a negative number of humans (%d)", n);
    HP_REQUIRE(humans || n == 0, HP_ERR_INVALID, "hp_humans_orient: null humans");
    const int q = orientation & 3, m = orientation >> 2;
    for (int i = 0; i < n; ++i)
        for (auto& p : humans[i].parts) {
            if (!p.has_value)
                continue;
            if (to_stored) {
                const float u = p.x, v = p.y;
                const float x = q == 0 ? u : q == 1 ? v : q == 2 ? 1.0f - u : 1.0f - v;
                const float y = q == 0 ? v : q == 1 ? 1.0f - u : q == 2 ? 1.0f - v : u;
                p.x = m ? 1.0f - x : x, p.y = y;
            } else {
                const float x = m ? 1.0f - p.x : p.x, y = p.y;
                p.x = q == 0 ? x : q == 1 ? 1.0f - y : q == 2 ? 1.0f - x : y;
                p.y = q == 0 ? y : q == 1 ? x : q == 2 ? 1.0f - y : 1.0f - x;
            }
        }
    return HP_OK;
}

} // extern "C"
