// resize_yuv_hdr_device.hpp — where a source pixel's (b, g, r) come from when the frame is a PQ / HLG 10-bit hp_yuv_image: the `Taps` type that ends in
// table reads instead of sat8 (the rule is tonemap.hpp's convert()), the block's LDS copy of the tables and the host code that fills the taps from a
// frame and an hp_tonemap.  Shared by resize_yuv_hdr.hip (the stored picture; the placement of the tables is discussed at its top) and
// resize_oriented.hip (the same taps behind a coordinate map).
#pragma once
#include "resize_rois_device.hpp"
#include "tonemap.hpp"

#include <cstring>

namespace hp_resize {

struct yuv_hdr_taps : yuv_taps<2, 1> {
    const uint16_t* lin; // A [1024]: device memory as launched; an LDS kernel points both at its block's copy
    const uint8_t* out;  // O [4096]
    int m[9];
    int primaries;
    __device__ __forceinline__ void load(int px, int py, int (&c)[3]) const
    {
        int Y, U, V;
        fetch(px, py, Y, U, V);
        hp_hdr::convert(Y, U, V, y_off, cy, cub, cug, cvg, cvr, lin, m, primaries != 0, out, c);
    }
    __device__ __forceinline__ yuv_hdr_taps at(int rx, int ry) const
    {
        yuv_hdr_taps t = *this;
        static_cast<yuv_taps<2, 1>&>(t) = yuv_taps<2, 1>::at(rx, ry);
        return t;
    }
};

// the block's copy of the tables: all 256 threads take part (before any of them leaves), 8 bytes per thread and step
template <bool LDS> __device__ __forceinline__ void stage_tables(yuv_hdr_taps& t, uint2* lds)
{
    if constexpr (LDS) {
        const uint2* src = reinterpret_cast<const uint2*>(t.lin); // A, then O, in one allocation (hp_tonemap::dev)
#pragma unroll
        for (int i = 0; i < (int)(hp_hdr::TABLE_BYTES / sizeof(uint2) / 256); ++i)
            lds[i * 256 + threadIdx.x] = src[i * 256 + threadIdx.x];
        __syncthreads();
        t.lin = reinterpret_cast<const uint16_t*>(lds);
        t.out = reinterpret_cast<const uint8_t*>(lds) + hp_hdr::LIN_N * sizeof(uint16_t);
    }
}
static_assert(hp_hdr::TABLE_BYTES % (sizeof(uint2) * 256) == 0, "stage_tables: a whole number of 8-byte steps per thread");

// the checks every HDR call makes first, and the taps of the frame
inline int prepare_hdr(const char* who, const hp_yuv_image* im, const hp_tonemap* tm, yuv_hdr_taps& t)
{
    HP_REQUIRE(tm, HP_ERR_INVALID, "%s: null hp_tonemap handle", who);
    HP_TRY(hp_hdr::check_frame(im, who, true));
    int32_t k[7];
    HP_TRY(hp_yuv_coefficients(im->matrix, im->range, 10, k));
    fill_taps(t, *im, *hp_yuv::layout_of(im->format), k);
    t.lin = static_cast<const uint16_t*>(tm->dev);
    t.out = static_cast<const uint8_t*>(tm->dev) + hp_hdr::LIN_N * sizeof(uint16_t);
    memcpy(t.m, tm->m, sizeof(t.m));
    t.primaries = tm->desc.to_bt709 != 0;
    return HP_OK;
}

// "image description (+ optional tone-map) -> Taps" for the calls that take both kinds of frame: with a tone-map prepare_hdr()'s checks and
// yuv_hdr_taps, without one resize_yuv_device.hpp's SDR statement; `f` gets the filled Taps either way
template <class F> int with_yuv_taps(const char* who, const hp_yuv_image* im, const hp_tonemap* tm, F&& f)
{
    if (!tm)
        return with_yuv_taps(who, im, f);
    yuv_hdr_taps t;
    HP_TRY(prepare_hdr(who, im, tm, t)); // refuses an 8-bit layout by name
    return f(t);
}

} // namespace hp_resize
