// resize_yuv_device.hpp — where a source pixel's (b, g, r) come from when the frame is an hp_yuv_image: the `Taps` type (see
// resize_device.hpp) of every kernel that reads video frames where they lie, and the host code that fills it from an image description.
// Shared by resize_yuv_formats.hip (one frame per launch) and resize_rois.hip (many regions of one frame per launch); the conversion
// contract is stated at the top of resize_yuv_formats.hip and restated in tests/yuv_formats_ref.py.
#pragma once
#include "resize_device.hpp"
#include "yuv_formats.hpp"

namespace hp_resize {

constexpr int YUV_SHIFT = 20;

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

template <int SAMPLE_BYTES, int Y_STEP> struct yuv_taps {
    const uint8_t *y, *u, *v; // byte address of the first Y, U and V sample (semi-planar and packed: inside the same plane)
    int y_stride, c_stride;   // row strides in bytes (c_stride: the U plane's, or the plane U and V share)
    int v_extra;              // V plane's row stride - c_stride: a planar frame may give its V plane a pitch of its own (0 otherwise)
    int c_step;               // bytes between horizontally neighbouring chroma samples
    int sx, sy;               // chroma shifts
    int shift;                // 16-bit samples: right shift before the 10-bit mask
    int y_off, c_off, cy, cub, cug, cvg, cvr;
    __device__ __forceinline__ int sample(const uint8_t* p) const
    {
        if constexpr (SAMPLE_BYTES == 2)
            return (*reinterpret_cast<const uint16_t*>(p) >> shift) & 1023;
        else
            return *p;
    }
    // the samples of source pixel (px, py): Y as stored, U and V with c_off subtracted (also what yuv_hdr_taps, resize_yuv_hdr.hip, starts from)
    __device__ __forceinline__ void fetch(int px, int py, int& Y, int& U, int& V) const
    {
        const size_t at = (size_t)(py >> sy) * c_stride + (size_t)(px >> sx) * c_step;
        Y = sample(y + (size_t)py * y_stride + (size_t)px * (Y_STEP * SAMPLE_BYTES));
        U = sample(u + at) - c_off, V = sample(v + at + (ptrdiff_t)(py >> sy) * v_extra) - c_off;
    }
    __device__ __forceinline__ void load(int px, int py, int (&c)[3]) const
    {
        int Y, U, V;
        fetch(px, py, Y, U, V);
        // 24-bit multiplies (full rate; a 32-bit v_mul_lo_u32 is not), exact here: every coefficient is below 2^23 (the largest, CUB of
        // BT.2020 limited, is 2 245 836), the samples are below 2^10, and the low 32 bits of the product are the product (|sum| <= 5.81e8).
        // resize_yuv420_kernel gets the same instructions from its literal constants
        const int yy = __mul24(max(0, Y - y_off), cy) + (1 << (YUV_SHIFT - 1));
        c[0] = sat8((yy + __mul24(cub, U)) >> YUV_SHIFT);
        c[1] = sat8((yy + __mul24(cvg, V) + __mul24(cug, U)) >> YUV_SHIFT);
        c[2] = sat8((yy + __mul24(cvr, V)) >> YUV_SHIFT);
    }
    // the taps of the sub-frame whose pixel (0, 0) is this frame's (rx, ry): its sub-planes.  rx and ry are multiples of the layout's
    // chroma sub-sampling (hp_yuv_roi_alignment), so (ry + py) >> sy == (ry >> sy) + (py >> sy) for every py, and likewise in x
    __device__ __forceinline__ yuv_taps at(int rx, int ry) const
    {
        yuv_taps t = *this;
        const ptrdiff_t c = (ptrdiff_t)(ry >> sy) * c_stride + (ptrdiff_t)(rx >> sx) * c_step;
        t.y += (ptrdiff_t)ry * y_stride + (ptrdiff_t)rx * (Y_STEP * SAMPLE_BYTES);
        t.u += c;
        t.v += c + (ptrdiff_t)(ry >> sy) * v_extra;
        return t;
    }
};

template <class Taps> void fill_taps(Taps& t, const hp_yuv_image& im, const hp_yuv::layout& l, const int32_t k[7])
{
    const hp_yuv::sample_map m = hp_yuv::map_samples(im, l);
    t.sx = l.sx, t.sy = l.sy, t.shift = l.shift;
    t.y = m.y, t.u = m.u, t.v = m.v;
    t.y_stride = m.y_stride, t.c_stride = m.c_stride, t.c_step = m.c_step, t.v_extra = m.v_extra;
    t.y_off = k[0], t.c_off = k[1], t.cy = k[2], t.cub = k[3], t.cug = k[4], t.cvg = k[5], t.cvr = k[6];
}

// The one statement of "image description -> Taps" for an SDR frame: every check of the description (hp_yuv::validate, then the matrix integers),
// then `f` is called with the frame's filled Taps - yuv_taps<2, 1> for the 16-bit layouts, <1, 2> for the packed ones, <1, 1> for the rest - and
// its result is returned.  An entry point is "this, and inside f: geometry, then the launch of the unit's kernel for that Taps type".
// (with a tone-map: resize_yuv_hdr_device.hpp's overload, which adds yuv_hdr_taps)
template <class F> int with_yuv_taps(const char* who, const hp_yuv_image* im, F&& f)
{
    HP_TRY(hp_yuv::validate(im, who));
    const hp_yuv::layout& l = *hp_yuv::layout_of(im->format);
    int32_t k[7];
    HP_TRY(hp_yuv_coefficients(im->matrix, im->range, l.sample_bytes == 2 ? 10 : 8, k));
    const auto filled = [&](auto t) {
        fill_taps(t, *im, l, k);
        return f(t);
    };
    return l.sample_bytes == 2 ? filled(yuv_taps<2, 1>{}) : l.planes == 1 ? filled(yuv_taps<1, 2>{}) : filled(yuv_taps<1, 1>{});
}

} // namespace hp_resize
