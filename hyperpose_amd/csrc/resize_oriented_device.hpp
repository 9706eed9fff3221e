// resize_oriented_device.hpp — an orientation (include/hp_hip.h, HP_ORIENT_*) as a coordinate map in front of any `Taps` type (resize_device.hpp):
// the resize kernels ask for pixel (ux, uy) of the UPRIGHT picture, oriented_taps turns that into the stored pixel and lets the inner Taps fetch
// it - by its own rule, so a YUV frame's chroma stays "replicated over the luma pixels it covers in the stored frame".  resize_pixel() and
// resize_rois_body() stay the one statement of the arithmetic: they see an upright frame (or region) of uw x uh.
//
// What the map holds.  With hp_orient::axes_of(code) = (swap, flip_x, flip_y), a = swap ? uy : ux, b = swap ? ux : uy and the stored rectangle
// (rx, ry, rw, rh) that the upright frame or region covers (hp_orient_roi):
//     stored x = rx + (flip_x ? rw - 1 - a : a)        stored y = ry + (flip_y ? rh - 1 - b : b)
// so all the map needs of the rectangle is the corner its walk starts from, (ox, oy) = (rx + (flip_x ? rw - 1 : 0), ry + (flip_y ? rh - 1 : 0)):
// a backwards axis is a negative step.  The inner Taps stays the whole frame's and is asked for absolute stored coordinates; at(ox, oy) - the call
// resize_rois_body() makes with a region's origin - only replaces the corner, the host puts a region's start corner where roi_geom has its origin.
#pragma once
#include "orientation.hpp"
#include "resize_rois_device.hpp"

namespace hp_resize {

template <class Taps> struct oriented_taps {
    Taps in;    // the stored frame
    int ox, oy; // stored pixel of upright (0, 0)
    int code;
    __device__ __forceinline__ void load(int ux, int uy, int (&c)[3]) const
    {
        const hp_orient::axes m = hp_orient::axes_of(code); // wave-uniform: scalar selects
        const int a = m.swap ? uy : ux, b = m.swap ? ux : uy;
        in.load(ox + (m.flip_x ? -a : a), oy + (m.flip_y ? -b : b), c);
    }
    __device__ __forceinline__ oriented_taps at(int x, int y) const
    {
        oriented_taps t = *this;
        t.ox = x, t.oy = y;
        return t;
    }
};

// the start corner of the walk over the stored rectangle r
inline void oriented_origin(int code, const hp_roi& r, int& ox, int& oy)
{
    const hp_orient::axes m = hp_orient::axes_of(code);
    ox = r.x + (m.flip_x ? r.w - 1 : 0), oy = r.y + (m.flip_y ? r.h - 1 : 0);
}

// The thread -> pixel map of the per-frame kernels.  ROWS is resize.hip's: the 32 lanes of a half-wave along a destination row.  Behind a quarter
// turn neighbouring destination pixels of a row are neighbouring stored ROWS - one cache line per lane and tap - so COLS puts the lanes along a
// destination column instead (8 x 32 pixels per block): the reads fall into a few lines again, the 3-byte writes are a row apart.  The host picks
// one per call (resize_oriented.hip, oriented_cols(): COLS behind a quarter turn, ROWS otherwise - both were measured for both).
template <bool COLS> __device__ __forceinline__ void oriented_pixel_of_thread(int& x, int& y)
{
    const int lane = threadIdx.x & 31, row = threadIdx.x >> 5;
    x = COLS ? blockIdx.x * RZ_BLOCK_H + row : blockIdx.x * RZ_BLOCK_W + lane;
    y = COLS ? blockIdx.y * RZ_BLOCK_W + lane : blockIdx.y * RZ_BLOCK_H + row;
}
inline dim3 oriented_grid(const rz_geom& g, bool cols)
{
    return cols ? dim3(hp::ceil_div(g.dw, RZ_BLOCK_H), hp::ceil_div(g.dh, RZ_BLOCK_W)) : rz_grid(g);
}

} // namespace hp_resize
