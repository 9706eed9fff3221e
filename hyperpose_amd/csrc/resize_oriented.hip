// resize_oriented.hip — hp_resize_oriented_* / hp_resize_rois_oriented_*: the fused resize of every feed (8-bit BGR, every SDR hp_yuv_image layout,
// PQ / HLG 10-bit) reading a frame that is stored turned and / or mirrored (include/hp_hip.h, HP_ORIENT_*), so that the network sees it upright
// without a rotation pass over the full-resolution surface.  The contract: the bytes written equal "convert the whole stored frame to 8-bit BGR by
// the feed's own rule, orient it (hp_orient_u8c3_host), then hp_resize_u8c3 / hp_letterbox_u8c3 from uw x uh".  Nothing of the arithmetic is
// restated: the kernels are resize_pixel() / resize_rois_body() over oriented_taps<Taps> (resize_oriented_device.hpp), which maps an upright
// pixel to its stored one and lets the feed's Taps fetch it.  Mode, letterbox inner size and the region table are picked from the UPRIGHT size.
//
// Orientation 0 never reaches this unit's kernels: every call forwards to its un-oriented twin (same kernels, same bytes, same refusals).
//
// Kernels (256 threads, one thread = one output pixel):
//     resize_oriented_{u8c3,planar8,packed8,word16,hdr}_kernel<COLS>   one frame per launch, both thread maps (resize_oriented_device.hpp)
//     resize_rois_oriented_{u8c3,planar8,packed8,word16,hdr}_kernel    up to 16 upright regions per launch (resize_rois_body's map: lanes along rows)
// The HDR kernels always stage the tone-map tables in LDS (resize_yuv_hdr.hip's default placement).
//
// Which thread map a per-frame call takes is decided by oriented_cols() (resize_oriented_host.hpp) from the code alone; HP_ORIENT_MAP=rows|cols (read
// at the first call) forces one for measurements (tools/orientation_bench.py; DESIGN.md 1.1 "Orientation" holds both columns).
#include "resize_oriented_host.hpp"
#include "resize_yuv_hdr_device.hpp"

namespace {

using namespace hp_resize;

template <bool COLS, class Taps> __device__ __forceinline__ void resize_oriented_body(const rz_geom& g, const Taps& t)
{
    int x, y;
    oriented_pixel_of_thread<COLS>(x, y);
    if (x >= g.dw || y >= g.dh)
        return;
    resize_pixel(g, t, x, y);
}

template <bool COLS> __global__ __launch_bounds__(256) void resize_oriented_u8c3_kernel(const rz_geom g, const oriented_taps<bgr_taps> t)
{
    resize_oriented_body<COLS>(g, t);
}
template <bool COLS> __global__ __launch_bounds__(256) void resize_oriented_planar8_kernel(const rz_geom g, const oriented_taps<yuv_taps<1, 1>> t)
{
    resize_oriented_body<COLS>(g, t);
}
template <bool COLS> __global__ __launch_bounds__(256) void resize_oriented_packed8_kernel(const rz_geom g, const oriented_taps<yuv_taps<1, 2>> t)
{
    resize_oriented_body<COLS>(g, t);
}
template <bool COLS> __global__ __launch_bounds__(256) void resize_oriented_word16_kernel(const rz_geom g, const oriented_taps<yuv_taps<2, 1>> t)
{
    resize_oriented_body<COLS>(g, t);
}
template <bool COLS> __global__ __launch_bounds__(256) void resize_oriented_hdr_kernel(const rz_geom g, oriented_taps<yuv_hdr_taps> t)
{
    __shared__ uint2 tables[hp_hdr::TABLE_BYTES / sizeof(uint2)];
    stage_tables<true>(t.in, tables);
    resize_oriented_body<COLS>(g, t);
}

__global__ __launch_bounds__(256) void resize_rois_oriented_u8c3_kernel(const roi_batch b, const oriented_taps<bgr_taps> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_oriented_planar8_kernel(const roi_batch b, const oriented_taps<yuv_taps<1, 1>> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_oriented_packed8_kernel(const roi_batch b, const oriented_taps<yuv_taps<1, 2>> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_oriented_word16_kernel(const roi_batch b, const oriented_taps<yuv_taps<2, 1>> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_oriented_hdr_kernel(const roi_batch b, oriented_taps<yuv_hdr_taps> t)
{
    __shared__ uint2 tables[hp_hdr::TABLE_BYTES / sizeof(uint2)];
    stage_tables<true>(t.in, tables);
    resize_rois_body(b, t);
}

// this unit's kernels for each Taps type: the per-frame one under either thread map, and the regions one (BGR regions: named at their one call)
auto frame_kernel(const oriented_taps<bgr_taps>&, bool cols) { return cols ? resize_oriented_u8c3_kernel<true> : resize_oriented_u8c3_kernel<false>; }
auto frame_kernel(const oriented_taps<yuv_hdr_taps>&, bool cols) { return cols ? resize_oriented_hdr_kernel<true> : resize_oriented_hdr_kernel<false>; }
auto frame_kernel(const oriented_taps<yuv_taps<2, 1>>&, bool cols) { return cols ? resize_oriented_word16_kernel<true> : resize_oriented_word16_kernel<false>; }
auto frame_kernel(const oriented_taps<yuv_taps<1, 2>>&, bool cols) { return cols ? resize_oriented_packed8_kernel<true> : resize_oriented_packed8_kernel<false>; }
auto frame_kernel(const oriented_taps<yuv_taps<1, 1>>&, bool cols) { return cols ? resize_oriented_planar8_kernel<true> : resize_oriented_planar8_kernel<false>; }
auto rois_kernel(const oriented_taps<yuv_hdr_taps>&) { return resize_rois_oriented_hdr_kernel; }
auto rois_kernel(const oriented_taps<yuv_taps<2, 1>>&) { return resize_rois_oriented_word16_kernel; }
auto rois_kernel(const oriented_taps<yuv_taps<1, 2>>&) { return resize_rois_oriented_packed8_kernel; }
auto rois_kernel(const oriented_taps<yuv_taps<1, 1>>&) { return resize_rois_oriented_planar8_kernel; }

template <class Taps> int launch_frame(const rz_geom& g, const oriented_taps<Taps>& t, hipStream_t s)
{
    const bool cols = oriented_cols(t.code);
    hipLaunchKernelGGL(frame_kernel(t, cols), oriented_grid(g, cols), dim3(256), 0, s, g, t);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

} // namespace

extern "C" {

int hp_resize_oriented_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, int orientation, int keep_ratio, int b, int g, int r,
    uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream)
{
    HP_CHECK_ORIENTATION("hp_resize_oriented_u8c3", orientation);
    if (orientation == HP_ORIENT_NONE)
        return keep_ratio ? hp_letterbox_u8c3(dev_src, sw, sh, src_stride, dev_dst, dw, dh, dst_stride, b, g, r, stream)
                          : hp_resize_u8c3(dev_src, sw, sh, src_stride, dev_dst, dw, dh, dst_stride, stream);
    HP_REQUIRE(dev_src && sw > 0 && sh > 0, HP_ERR_INVALID, "hp_resize_oriented_u8c3: BGR: empty source");
    HP_REQUIRE(src_stride >= sw * 3, HP_ERR_INVALID, "hp_resize_oriented_u8c3: BGR: row stride smaller than a row");
    const int bg[3] = { b, g, r };
    rz_geom geom;
    HP_TRY(prepare_frame(orientation, sw, sh, keep_ratio, bg, dev_dst, dw, dh, dst_stride, geom));
    return launch_frame(geom, orient(bgr_taps{ dev_src, src_stride }, orientation, sw, sh), (hipStream_t)stream);
}

int hp_resize_oriented_yuv(const hp_yuv_image* src, const hp_tonemap* tm, int orientation, int keep_ratio, int b, int g, int r, uint8_t* dev_dst,
    int dw, int dh, int dst_stride, void* stream)
{
    const char* who = "hp_resize_oriented_yuv";
    HP_CHECK_ORIENTATION(who, orientation);
    if (orientation == HP_ORIENT_NONE) {
        if (tm)
            return keep_ratio ? hp_letterbox_yuv_hdr(src, tm, dev_dst, dw, dh, dst_stride, b, g, r, stream)
                              : hp_resize_yuv_hdr(src, tm, dev_dst, dw, dh, dst_stride, stream);
        return keep_ratio ? hp_letterbox_yuv(src, dev_dst, dw, dh, dst_stride, b, g, r, stream) : hp_resize_yuv(src, dev_dst, dw, dh, dst_stride, stream);
    }
    return with_yuv_taps(who, src, tm, [&](const auto& in) -> int {
        const int bg[3] = { b, g, r };
        rz_geom geom;
        HP_TRY(prepare_frame(orientation, src->width, src->height, keep_ratio, bg, dev_dst, dw, dh, dst_stride, geom));
        return launch_frame(geom, orient(in, orientation, src->width, src->height), (hipStream_t)stream);
    });
}

int hp_resize_rois_oriented_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, int orientation, const hp_roi* rois, int n, int keep_ratio,
    int b, int g, int r, uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream)
{
    const char* who = "hp_resize_rois_oriented_u8c3";
    HP_CHECK_ORIENTATION(who, orientation);
    if (orientation == HP_ORIENT_NONE)
        return hp_resize_rois_u8c3(dev_src, sw, sh, src_stride, rois, n, keep_ratio, b, g, r, dev_dst, dw, dh, dst_stride, slot_stride, stream);
    HP_REQUIRE(dev_src && sw > 0 && sh > 0, HP_ERR_INVALID, "%s: BGR: empty source", who);
    HP_REQUIRE(src_stride >= sw * 3, HP_ERR_INVALID, "%s: BGR: row stride smaller than a row", who);
    const int bg[3] = { b, g, r };
    roi_geom geom[ROIS_MAX];
    HP_TRY(prepare_oriented_rois(who, "BGR", orientation, sw, sh, 1, 1, rois, n, keep_ratio, dev_dst, dw, dh, dst_stride, slot_stride, bg, geom));
    const oriented_taps<bgr_taps> t{ bgr_taps{ dev_src, src_stride }, 0, 0, orientation };
    return launch_rois(resize_rois_oriented_u8c3_kernel, t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, (hipStream_t)stream);
}

int hp_resize_rois_oriented_yuv(const hp_yuv_image* src, const hp_tonemap* tm, int orientation, const hp_roi* rois, int n, int keep_ratio, int b, int g,
    int r, uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream)
{
    const char* who = "hp_resize_rois_oriented_yuv";
    HP_CHECK_ORIENTATION(who, orientation);
    if (orientation == HP_ORIENT_NONE)
        return tm ? hp_resize_rois_yuv_hdr(src, tm, rois, n, keep_ratio, b, g, r, dev_dst, dw, dh, dst_stride, slot_stride, stream)
                  : hp_resize_rois_yuv(src, rois, n, keep_ratio, b, g, r, dev_dst, dw, dh, dst_stride, slot_stride, stream);
    return with_yuv_taps(who, src, tm, [&](const auto& in) -> int {
        const hp_yuv::layout& l = *hp_yuv::layout_of(src->format);
        const int bg[3] = { b, g, r };
        roi_geom geom[ROIS_MAX];
        HP_TRY(prepare_oriented_rois(who, l.name, orientation, src->width, src->height, 1 << l.sx, 1 << l.sy, rois, n, keep_ratio, dev_dst, dw, dh,
            dst_stride, slot_stride, bg, geom));
        const oriented_taps<std::decay_t<decltype(in)>> t{ in, 0, 0, orientation }; // (the origin is each region's, from geom)
        return launch_rois(rois_kernel(t), t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, (hipStream_t)stream);
    });
}

} // extern "C"
