// resize_yuv_formats.hip — hp_resize_yuv / hp_letterbox_yuv: a video frame described by hp_yuv_image (include/hp_hip.h: 8- and 10-bit,
// 4:2:0 / 4:2:2 / 4:4:4, planar, semi-planar and packed, BT.601 / BT.709 / BT.2020, limited and full range) straight to the network's
// 8-bit BGR HWC input, colour conversion fused into the resize.  The generalisation of resize_yuv.hip's yuv420_taps: the resize arithmetic
// is resize_device.hpp's resize_pixel(), this file adds only where a source pixel's (b, g, r) come from.
//
// Conversion (the contract tests/yuv_formats_ref.py restates): chroma replicated over the luma pixels it covers, no interpolation, and
//     u = U - c_off   v = V - c_off   yy = max(0, Y - y_off) * CY + (1 << 19)
//     B = sat8((yy + CUB*u) >> 20)   G = sat8((yy + CVG*v + CUG*u) >> 20)   R = sat8((yy + CVR*v) >> 20)        int32, arithmetic shift
// on the d-bit samples (d = 8 or 10): a 10-bit frame is converted at its own precision, it is not narrowed first.  The seven integers
// come from hp_yuv_coefficients() below: OpenCV's ITUR_BT_601_* set for (BT.601, limited, 8 bits) - the one resize_yuv.hip holds, so
// NV12 / I420 through this file give the bytes of hp_resize_yuv420, and YUY2 / UYVY those of cv::cvtColor(COLOR_YUV2BGR_YUY2 / _UYVY) -
// and for every other combination the rounded 2^20 multiples of the matrix's own terms.  The largest |sum| over all twelve tables is
// 5.81e8 (BT.2020 limited 10-bit): inside int32.
//
// Everything that describes the layout is uniform per launch and travels in the kernel-argument struct (SGPRs): plane addresses, byte
// strides, the byte step between neighbouring chroma samples, the chroma shifts and the table.  What changes the instructions of a load
// is a template parameter, so there are three kernels and no per-thread branch on the format:
//     resize_yuv_planar8_kernel   one byte per sample, luma at byte x          NV12 I420 NV16 I422 I444
//     resize_yuv_packed8_kernel   one byte per sample, luma at byte 2x (+1)    YUY2 UYVY (U and V inside the same plane, step 4)
//     resize_yuv_word16_kernel    16-bit words, value = (word >> shift) & 1023  P010 (shift 6) I010 (shift 0)
// Each keeps the shape of resize_yuv420_kernel: one thread = one output pixel, 32 x 8 pixels per block of 256 threads, byte / 16-bit
// loads whose neighbours in a wavefront fall into the same few cache lines.
#include "resize_yuv_device.hpp"

#include <cstring>

namespace {

using namespace hp_resize;

// yuv_taps<>, fill_taps() and with_yuv_taps(): resize_yuv_device.hpp, shared with the multi-region kernels of resize_rois.hip

template <class Taps> __device__ __forceinline__ void resize_yuv_body(const rz_geom& g, const Taps& t)
{
    const int x = blockIdx.x * RZ_BLOCK_W + (threadIdx.x & 31), y = blockIdx.y * RZ_BLOCK_H + (threadIdx.x >> 5);
    if (x >= g.dw || y >= g.dh)
        return;
    resize_pixel(g, t, x, y);
}

__global__ __launch_bounds__(256) void resize_yuv_planar8_kernel(const rz_geom g, const yuv_taps<1, 1> t) { resize_yuv_body(g, t); }
__global__ __launch_bounds__(256) void resize_yuv_packed8_kernel(const rz_geom g, const yuv_taps<1, 2> t) { resize_yuv_body(g, t); }
__global__ __launch_bounds__(256) void resize_yuv_word16_kernel(const rz_geom g, const yuv_taps<2, 1> t) { resize_yuv_body(g, t); }

// this unit's kernel for each Taps type that with_yuv_taps() hands out
auto kernel_of(const yuv_taps<2, 1>&) { return resize_yuv_word16_kernel; }
auto kernel_of(const yuv_taps<1, 2>&) { return resize_yuv_packed8_kernel; }
auto kernel_of(const yuv_taps<1, 1>&) { return resize_yuv_planar8_kernel; }

int launch_resize_yuv_image(const hp_yuv_image* im, const char* who, uint8_t* dst, int dw, int dh, int dst_stride, bool letterbox, const int bg[3],
    hipStream_t s)
{
    return with_yuv_taps(who, im, [&](const auto& t) -> int {
        int iw = dw, ih = dh;
        if (letterbox)
            hp_letterbox_inner(im->width, im->height, dw, dh, &iw, &ih);
        rz_geom g;
        HP_TRY(rz_prepare(g, im->width, im->height, dst, dw, dh, dst_stride, iw, ih, bg));
        hipLaunchKernelGGL(kernel_of(t), rz_grid(g), dim3(256), 0, s, g, t);
        HP_HIP_TRY(hipGetLastError());
        return HP_OK;
    });
}

} // namespace

int hp_yuv::validate(const hp_yuv_image* im, const char* who, bool kernel_access)
{
    HP_REQUIRE(im, HP_ERR_INVALID, "%s: null image", who);
    const hp_yuv::layout* l = hp_yuv::layout_of(im->format);
    HP_REQUIRE(l, HP_ERR_INVALID, "%s: unknown format %d (HP_YUV_NV12 .. HP_YUV_I444)", who, im->format);
    HP_REQUIRE(im->matrix >= HP_YUV_BT601 && im->matrix <= HP_YUV_BT2020, HP_ERR_INVALID, "%s: %s: unknown matrix %d (HP_YUV_BT601, _BT709, _BT2020)", who,
        l->name, im->matrix);
    HP_REQUIRE(im->range == HP_YUV_LIMITED || im->range == HP_YUV_FULL, HP_ERR_INVALID, "%s: %s: unknown range %d (HP_YUV_LIMITED, HP_YUV_FULL)", who, l->name,
        im->range);
    HP_REQUIRE(im->width > 0 && im->height > 0, HP_ERR_INVALID, "%s: %s: empty frame (%d x %d)", who, l->name, im->width, im->height);
    HP_REQUIRE(hp_yuv::size_ok(*l, im->width, im->height), HP_ERR_INVALID, "%s: %s frames need %s, got %d x %d", who, l->name,
        l->sy ? "even width and height" : "an even width", im->width, im->height);
    for (int k = 0; k < l->planes; ++k) {
        HP_REQUIRE(im->plane[k], HP_ERR_INVALID, "%s: %s: plane %d is null", who, l->name, k);
        HP_REQUIRE(im->stride[k] > 0 && (size_t)im->stride[k] >= hp_yuv::row_bytes(*l, k, im->width), HP_ERR_INVALID,
            "%s: %s: stride %d of plane %d is smaller than a row (%zu bytes)", who, l->name, im->stride[k], k, hp_yuv::row_bytes(*l, k, im->width));
        HP_REQUIRE(!kernel_access || l->sample_bytes == 1 || (im->stride[k] % 2 == 0 && (uintptr_t)im->plane[k] % 2 == 0), HP_ERR_INVALID,
            "%s: %s: plane %d (16-bit words) needs an even address and an even stride", who, l->name, k);
    }
    return HP_OK;
}

extern "C" {

int hp_yuv_coefficients(int matrix, int range, int depth, int32_t out[7])
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_yuv_coefficients: null output");
    HP_REQUIRE(matrix >= HP_YUV_BT601 && matrix <= HP_YUV_BT2020, HP_ERR_INVALID, "hp_yuv_coefficients: unknown matrix %d", matrix);
    HP_REQUIRE(range == HP_YUV_LIMITED || range == HP_YUV_FULL, HP_ERR_INVALID, "hp_yuv_coefficients: unknown range %d", range);
    HP_REQUIRE(depth == 8 || depth == 10, HP_ERR_INVALID, "hp_yuv_coefficients: depth %d (8 or 10)", depth);
    if (matrix == HP_YUV_BT601 && range == HP_YUV_LIMITED && depth == 8) { // OpenCV's ITUR_BT_601_* set, as in resize_yuv.hip
        const int32_t cv[7] = { 16, 128, 1220542, 2116026, -409993, -852492, 1673527 };
        memcpy(out, cv, sizeof(cv));
        return HP_OK;
    }
    static const double KR[3] = { 0.299, 0.2126, 0.2627 }, KB[3] = { 0.114, 0.0722, 0.0593 };
    const double kr = KR[matrix], kb = KB[matrix], kg = 1. - kr - kb, one = (double)(1 << YUV_SHIFT);
    const int up = depth - 8;
    const double ys = range == HP_YUV_LIMITED ? 255. / (219 << up) : 255. / ((1 << depth) - 1);
    const double cs = range == HP_YUV_LIMITED ? 255. / (224 << up) : 255. / ((1 << depth) - 1);
    out[0] = range == HP_YUV_LIMITED ? 16 << up : 0;
    out[1] = 1 << (depth - 1);
    out[2] = (int32_t)std::rint(ys * one);
    out[3] = (int32_t)std::rint(2. * (1. - kb) * cs * one);
    out[4] = -(int32_t)std::rint(2. * kb * (1. - kb) / kg * cs * one);
    out[5] = -(int32_t)std::rint(2. * kr * (1. - kr) / kg * cs * one);
    out[6] = (int32_t)std::rint(2. * (1. - kr) * cs * one);
    return HP_OK;
}

int hp_yuv_plane_layout(int format, int k, int width, int height, size_t* row_bytes, int* rows)
{
    const hp_yuv::layout* l = hp_yuv::layout_of(format);
    if (!l)
        return 0;
    const bool ok = k >= 0 && k < l->planes && hp_yuv::size_ok(*l, width, height);
    if (row_bytes)
        *row_bytes = ok ? hp_yuv::row_bytes(*l, k, width) : 0;
    if (rows)
        *rows = ok ? hp_yuv::rows(*l, k, height) : 0;
    return l->planes;
}

size_t hp_yuv_packed_bytes(int format, int width, int height)
{
    const hp_yuv::layout* l = hp_yuv::layout_of(format);
    if (!l || !hp_yuv::size_ok(*l, width, height))
        return 0;
    size_t n = 0;
    for (int k = 0; k < l->planes; ++k)
        n += hp_yuv::row_bytes(*l, k, width) * hp_yuv::rows(*l, k, height);
    return n;
}

int hp_resize_yuv(const hp_yuv_image* src, uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream)
{
    const int bg[3] = { 0, 0, 0 };
    return launch_resize_yuv_image(src, "hp_resize_yuv", dev_dst, dw, dh, dst_stride, false, bg, (hipStream_t)stream);
}

int hp_letterbox_yuv(const hp_yuv_image* src, uint8_t* dev_dst, int dw, int dh, int dst_stride, int b, int g, int r, void* stream)
{
    const int bg[3] = { b, g, r };
    return launch_resize_yuv_image(src, "hp_letterbox_yuv", dev_dst, dw, dh, dst_stride, true, bg, (hipStream_t)stream);
}

} // extern "C"
