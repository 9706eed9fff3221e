// hyperpose::to_yuv — addition: the frame a video encoder takes, made from a packed RGB or grey frame (screen capture, a canvas, a renderer, a grey
// camera, a cv::Mat): any yuv_frame layout in the matrix, range and bit depth the stream is tagged with, padded by edge replication to the size the
// encoder needs (hp_rgb_to_yuv, include/hp_hip.h "encoder hand-off"; the exact integer rule: DESIGN.md 1.1 "Encoder hand-off").  The forward
// counterpart of what the engine does with a yuv_frame.  With both frames `on_device` the conversion is one kernel launch on `stream` (asynchronous,
// stream-ordered) and draw_humans / redact_humans / draw_maps then work on `dst` as on a decoder's surface: capture -> to_yuv -> redact / maps /
// skeletons -> encoder without a copy to the host.  With both frames in host memory the library's host twin gives the same bytes.  `dst` describes
// planes the caller owns (padded_size and yuv_frame::row_bytes / rows size them); `dst.plane[]` is WRITTEN and must not overlap `src`.  Errors of the
// C ABI (a size the layout cannot hold, dst smaller than src or over 8192, a null plane, misaligned device planes) throw std::logic_error, and so
// does a pair of frames of which only one is on the device.  No resize, no orientation, no HDR transfer, no alpha.
#pragma once
#include <stdexcept>
#include <string>

#include "data.hpp"

namespace hyperpose {

namespace detail {
    inline void to_yuv_check(int rc)
    {
        if (rc < HP_OK)
            throw std::logic_error(std::string("hyperpose::to_yuv: ") + hp_last_error());
    }
} // namespace detail

/// the smallest size at least `size` whose sides are multiples of `align` (1 .. 256) and of what `format` needs (4:2:0: even width and height)
inline cv::Size padded_size(int format, cv::Size size, int align = 1)
{
    int w = 0, h = 0;
    if (hp_yuv_padded_size(format, size.width, size.height, align, &w, &h) < HP_OK)
        throw std::logic_error(std::string("hyperpose::padded_size: ") + hp_last_error());
    return cv::Size(w, h);
}

/// `dst.plane[]` is WRITTEN (the struct declares it const because the engine only reads it)
inline void to_yuv(const rgb_frame& src, yuv_frame& dst, void* stream = nullptr)
{
    if (src.on_device != dst.on_device)
        throw std::logic_error("hyperpose::to_yuv: source and destination must both be in host memory or both on the device");
    const hp_rgb_image in = src.image();
    const hp_yuv_image out = dst.image();
    detail::to_yuv_check(src.on_device ? hp_rgb_to_yuv(&in, &out, stream) : hp_rgb_to_yuv_host(&in, &out));
}

/// a BGR picture in host memory into a yuv_frame in host memory
inline void to_yuv(const cv::Mat& bgr, yuv_frame& dst)
{
#ifdef HYPERPOSE_USE_OPENCV
    if (bgr.type() != CV_8UC3)
        throw std::logic_error("hyperpose::to_yuv: the picture must be 8-bit BGR (CV_8UC3)");
    const int stride = (int)bgr.step;
#else
    const int stride = bgr.cols * 3;
#endif
    to_yuv(rgb_frame(HP_RGB_BGR24, detail::mat_data(bgr), bgr.cols, bgr.rows, stride), dst);
}

} // namespace hyperpose
