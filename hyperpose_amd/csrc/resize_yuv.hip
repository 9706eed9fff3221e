// resize_yuv.hip — video frames as decoders deliver them: YUV 4:2:0 (NV12 from hardware decoders, I420 from software ones) straight to the
// network's 8-bit BGR HWC input, colour conversion fused into the resize.  The result is bit-identical to "convert the whole frame to BGR
// (cv::cvtColor COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420), then hp_resize_u8c3 / hp_letterbox_u8c3": an output pixel reads at most 2 x 2
// source pixels, so only those are converted.  The resize arithmetic is resize_device.hpp's resize_pixel(), the same statement
// resize_u8c3_kernel runs; this file adds only where a source pixel's (b, g, r) come from.
//
// Conversion: OpenCV's 8-bit fixed-point BT.601 limited-range form (imgproc color_yuv, ITUR_BT_601_* constants, shift 20), chroma
// replicated over its 2 x 2 luma pixels without interpolation.  Restated from the constants (tests/yuv_ref.py holds the same statement in
// numpy); parity unpinned: no OpenCV in the build image.  All sums stay inside int32 (largest magnitude about 5.6e8); the shift is
// arithmetic on possibly negative sums.
//
// The two layouts are one kernel with a different chroma address: NV12 keeps (U, V) byte pairs in one plane (step 2, V one byte after U),
// I420 a U plane and a V plane (step 1).  Loads are single bytes, as in the BGR kernel: neighbouring threads read neighbouring Y bytes
// (stride = the scale factor) and pairs of threads share a chroma byte, so a wavefront's row of taps falls into a few cache lines.
// One thread = one output pixel.
#include "resize_device.hpp"

namespace {

using namespace hp_resize;

constexpr int YUV_SHIFT = 20;
constexpr int YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527;

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

struct yuv420_taps {
    const uint8_t *y, *u, *v; // NV12: v = u + 1
    int y_stride, uv_stride, uv_step;
    __device__ __forceinline__ void load(int px, int py, int (&c)[3]) const
    {
        const size_t at = (size_t)(py >> 1) * uv_stride + (size_t)(px >> 1) * uv_step;
        const int Y = y[(size_t)py * y_stride + px], U = u[at] - 128, V = v[at] - 128;
        const int yy = max(0, Y - 16) * YUV_CY + (1 << (YUV_SHIFT - 1));
        c[0] = sat8((yy + YUV_CUB * U) >> YUV_SHIFT);
        c[1] = sat8((yy + YUV_CVG * V + YUV_CUG * U) >> YUV_SHIFT);
        c[2] = sat8((yy + YUV_CVR * V) >> YUV_SHIFT);
    }
};

__global__ __launch_bounds__(256) void resize_yuv420_kernel(const rz_geom g, const yuv420_taps t)
{
    const int x = blockIdx.x * RZ_BLOCK_W + (threadIdx.x & 31), y = blockIdx.y * RZ_BLOCK_H + (threadIdx.x >> 5);
    if (x >= g.dw || y >= g.dh)
        return;
    resize_pixel(g, t, x, y);
}

int launch_resize_yuv(int format, const uint8_t* dev_y, int y_stride, const uint8_t* dev_u, const uint8_t* dev_v, int uv_stride, int sw, int sh,
    uint8_t* dst, int dw, int dh, int dst_stride, int iw, int ih, const int bg[3], hipStream_t s)
{
    HP_REQUIRE(format == HP_YUV_NV12 || format == HP_YUV_I420, HP_ERR_INVALID, "resize_yuv420: unknown format %d (HP_YUV_NV12, HP_YUV_I420)", format);
    HP_REQUIRE(dev_y && dev_u && (format == HP_YUV_NV12 || dev_v), HP_ERR_INVALID, "resize_yuv420: null plane");
    HP_REQUIRE(sw > 0 && sh > 0 && sw % 2 == 0 && sh % 2 == 0, HP_ERR_INVALID, "resize_yuv420: 4:2:0 frames need even width and height, got %d x %d", sw, sh);
    HP_REQUIRE(y_stride >= sw && uv_stride >= (format == HP_YUV_NV12 ? sw : sw / 2), HP_ERR_INVALID, "resize_yuv420: plane stride smaller than a row");
    rz_geom g;
    HP_TRY(rz_prepare(g, sw, sh, dst, dw, dh, dst_stride, iw, ih, bg));
    yuv420_taps t;
    t.y = dev_y, t.u = dev_u, t.v = format == HP_YUV_NV12 ? dev_u + 1 : dev_v;
    t.y_stride = y_stride, t.uv_stride = uv_stride, t.uv_step = format == HP_YUV_NV12 ? 2 : 1;
    hipLaunchKernelGGL(resize_yuv420_kernel, rz_grid(g), dim3(256), 0, s, g, t);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

} // namespace

extern "C" {

int hp_resize_yuv420(int format, const uint8_t* dev_y, int y_stride, const uint8_t* dev_u, const uint8_t* dev_v, int uv_stride, int sw, int sh,
    uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream)
{
    const int bg[3] = { 0, 0, 0 };
    return launch_resize_yuv(format, dev_y, y_stride, dev_u, dev_v, uv_stride, sw, sh, dev_dst, dw, dh, dst_stride, dw, dh, bg, (hipStream_t)stream);
}

int hp_letterbox_yuv420(int format, const uint8_t* dev_y, int y_stride, const uint8_t* dev_u, const uint8_t* dev_v, int uv_stride, int sw, int sh,
    uint8_t* dev_dst, int dw, int dh, int dst_stride, int b, int g, int r, void* stream)
{
    HP_REQUIRE(sw > 0 && sh > 0, HP_ERR_INVALID, "letterbox_yuv420: empty source");
    int iw = 0, ih = 0;
    hp_letterbox_inner(sw, sh, dw, dh, &iw, &ih);
    const int bg[3] = { b, g, r };
    return launch_resize_yuv(format, dev_y, y_stride, dev_u, dev_v, uv_stride, sw, sh, dev_dst, dw, dh, dst_stride, iw, ih, bg, (hipStream_t)stream);
}

} // extern "C"
