// resize.hip — the stream front-end's per-frame geometry on gfx950: cv::resize (INTER_LINEAR, CV_8UC3) and
// hyperpose::non_scaling_resize (reference src/data.cpp:53-69, used at src/stream.cpp:89-103 and
// src/tensorrt.cpp:448), plus resume_ratio (include/hyperpose/utility/human.hpp:44-58) for the way back.
//
// One thread = one output pixel.  Every output pixel re-derives its own source coordinates and 11-bit fixed-point
// coefficients with exactly OpenCV's arithmetic (double scale, float fractional part, round-half-even to short,
// integer horizontal pass, ((b*(S>>4))>>16) vertical pass, 2x2 down-scale rerouted to the area average, equal sizes
// copied) - see oracle/resize_oracle.cpp for the derivation; the two agree bit for bit (tests/test_resize_gpu.py).  That arithmetic is
// stated once, in resize_device.hpp, and shared with the YUV 4:2:0 front-end (resize_yuv.hip).
// Frames are a few hundred KB: the kernels are latency-trivial next to the conv stack; what matters is that the
// frames never go back to the host between decode and parse.
#include "resize_device.hpp"

namespace {

using namespace hp_resize;

// the arithmetic is resize_device.hpp's resize_pixel(); this kernel feeds it BGR source pixels
__global__ __launch_bounds__(256) void resize_u8c3_kernel(const rz_geom g, const bgr_taps t)
{
    const int x = blockIdx.x * RZ_BLOCK_W + (threadIdx.x & 31), y = blockIdx.y * RZ_BLOCK_H + (threadIdx.x >> 5);
    if (x >= g.dw || y >= g.dh)
        return;
    resize_pixel(g, t, x, y);
}

int launch_resize(const uint8_t* src, int sw, int sh, int src_stride, uint8_t* dst, int dw, int dh, int dst_stride, int iw, int ih,
    const int bg[3], hipStream_t s)
{
    HP_REQUIRE(src, HP_ERR_INVALID, "resize: bad geometry");
    rz_geom g;
    HP_TRY(rz_prepare(g, sw, sh, dst, dw, dh, dst_stride, iw, ih, bg));
    HP_REQUIRE(src_stride >= sw * 3, HP_ERR_INVALID, "resize: row stride smaller than a row");
    const bgr_taps t{ src, src_stride };
    hipLaunchKernelGGL(resize_u8c3_kernel, rz_grid(g), dim3(256), 0, s, g, t);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

} // namespace

extern "C" {

int hp_resize_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream)
{
    const int bg[3] = { 0, 0, 0 };
    return launch_resize(dev_src, sw, sh, src_stride, dev_dst, dw, dh, dst_stride, dw, dh, bg, (hipStream_t)stream);
}

void hp_letterbox_inner(int sw, int sh, int dw, int dh, int* iw, int* ih)
{
    // src/data.cpp:57-64, doubles truncated by cv::Size(int, int)
    const double h1 = dw * (sh / (double)sw);
    const double w2 = dh * (sw / (double)sh);
    if (h1 <= dh)
        *iw = dw, *ih = (int)h1;
    else
        *iw = (int)w2, *ih = dh;
}

int hp_letterbox_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, uint8_t* dev_dst, int dw, int dh, int dst_stride, int b, int g,
    int r, void* stream)
{
    HP_REQUIRE(sw > 0 && sh > 0, HP_ERR_INVALID, "letterbox: empty source");
    int iw = 0, ih = 0;
    hp_letterbox_inner(sw, sh, dw, dh, &iw, &ih);
    const int bg[3] = { b, g, r };
    return launch_resize(dev_src, sw, sh, src_stride, dev_dst, dw, dh, dst_stride, iw, ih, bg, (hipStream_t)stream);
}

void hp_resume_ratio(hp_human* humans, int n, int src_w, int src_h, int dst_w, int dst_h)
{
    // include/hyperpose/utility/human.hpp:44-58 (float *= double: promote, multiply, narrow)
    if (!humans)
        return;
    if ((long)src_h * dst_w > (long)src_w * dst_h) {
        const double xratio = (double)dst_w * src_h / ((double)dst_h * src_w);
        for (int i = 0; i < n; ++i)
            for (auto& part : humans[i].parts)
                part.x = (float)(part.x * xratio);
    } else {
        const double yratio = (double)dst_h * src_w / ((double)dst_w * src_h);
        for (int i = 0; i < n; ++i)
            for (auto& part : humans[i].parts)
                part.y = (float)(part.y * yratio);
    }
}

} // extern "C"
