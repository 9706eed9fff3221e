// resize_oriented_host.hpp — the host side that every unit with oriented kernels shares (resize_oriented.hip: 8-bit BGR and hp_yuv_image feeds;
// resize_rgb.hip: hp_rgb_image feeds): the choice between the two thread maps, the geometry of a per-frame call and the region table of a rois call,
// both taken from the UPRIGHT size.  Host code only: no kernel is declared or instantiated here.
#pragma once
#include "resize_oriented_device.hpp"

#include <cstdlib>
#include <cstring>

namespace hp_resize {

// The thread map of a per-frame call, from the code alone (never from the data).  Measured on the MI355X for bgr, nv12, yuy2 and p010-hdr
// (profiles/orientation_bench.json, DESIGN.md 1.1 "Orientation"; us per launch, rows / cols):
//     a quarter turn   1280 x 720 -> 1440 x 2560 (device-bound)   55.1 / 39.0   78.2 / 32.7   78.2 / 44.3   82.9 / 40.5     COLS, by 1.4 - 2.4 x
//                      letter-boxed into 432 x 368 (launch-bound)  4.10 / 3.70   5.16 / 3.71   5.17 / 4.40   5.67 / 4.77    COLS again
//     half turn, mirror  -> 2560 x 1440                            20.4 / 71.9   22.3 / 92.0   26.4 / 94.6   33.9 / 97.9     ROWS, by 2.9 - 4.1 x
// Shrinking and enlarging agree, so the geometry does not enter the rule: lanes run along whichever destination axis is the stored x axis.
// HP_ORIENT_MAP=rows|cols (read at a unit's first call) forces one for measurements.
inline bool oriented_cols(int code)
{
    static const int forced = [] {
        const char* e = getenv("HP_ORIENT_MAP");
        return !e ? -1 : strcmp(e, "cols") == 0 ? 1 : strcmp(e, "rows") == 0 ? 0 : -1;
    }();
    if (forced >= 0)
        return forced != 0;
    return (code & 1) != 0;
}

template <class Taps> oriented_taps<Taps> orient(const Taps& in, int code, int sw, int sh)
{
    oriented_taps<Taps> t{ in, 0, 0, code };
    oriented_origin(code, hp_roi{ 0, 0, sw, sh }, t.ox, t.oy);
    return t;
}

// the geometry of a per-frame call: the resize runs from the upright size
inline int prepare_frame(int code, int sw, int sh, int keep_ratio, const int bg[3], uint8_t* dst, int dw, int dh, int dst_stride, rz_geom& g)
{
    int uw = 0, uh = 0;
    HP_TRY(hp_oriented_size(code, sw, sh, &uw, &uh));
    int iw = dw, ih = dh;
    if (keep_ratio)
        hp_letterbox_inner(uw, uh, dw, dh, &iw, &ih);
    return rz_prepare(g, uw, uh, dst, dw, dh, dst_stride, iw, ih, bg);
}

// the region table of a rois call: checked and sorted as upright regions of the upright frame (for a turned frame the alignment pair is swapped,
// which is the stored rectangle's alignment), then every entry's origin becomes the stored corner its walk starts from
inline int prepare_oriented_rois(const char* who, const char* format, int code, int sw, int sh, int ax, int ay, const hp_roi* rois, int n, int keep_ratio,
    uint8_t* dst, int dw, int dh, int dst_stride, size_t slot_stride, const int bg[3], roi_geom (&geom)[ROIS_MAX])
{
    int uw = 0, uh = 0;
    HP_TRY(hp_oriented_size(code, sw, sh, &uw, &uh));
    const bool turned = (code & 1) != 0;
    HP_TRY(prepare_rois(who, format, uw, uh, turned ? ay : ax, turned ? ax : ay, rois, n, keep_ratio, dst, dw, dh, dst_stride, slot_stride, bg, geom));
    for (int k = 0; k < n; ++k) {
        const hp_roi upright{ geom[k].x, geom[k].y, geom[k].sw, geom[k].sh };
        hp_roi stored;
        HP_TRY(hp_orient_roi(&upright, code, sw, sh, &stored));
        oriented_origin(code, stored, geom[k].x, geom[k].y);
    }
    return HP_OK;
}

#define HP_CHECK_ORIENTATION(who, code) \
    HP_REQUIRE(hp_orient::valid(code), HP_ERR_INVALID, "%s: orientation %d is no HP_ORIENT_* code (0 .. 7)", who, code)

} // namespace hp_resize
