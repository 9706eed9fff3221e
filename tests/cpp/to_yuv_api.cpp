// hyperpose::to_yuv and hyperpose::padded_size (include/hyperpose/utility/encode.hpp) on frames in HOST memory: a host program against the mirror
// headers, no device needed.  An rgb_frame with a padded pitch and a cv::Mat give the bytes of the C ABI's hp_rgb_to_yuv_host on planes sized by
// padded_size, yuv_frame::row_bytes and yuv_frame::rows; the row padding keeps its fill; a destination smaller than the source, a size the layout
// cannot hold and a pair of frames of which one is on the device throw std::logic_error.  Prints "OK <compared> <threw>"; run by
// tests/test_cpp_to_yuv.py.
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

namespace hp = hyperpose;

struct surface {
    hp::yuv_frame frame;
    std::vector<std::vector<uint8_t>> planes;
    surface(int format, cv::Size size, int matrix, int range, int pitch)
    {
        frame.format = format, frame.matrix = matrix, frame.range = range, frame.width = size.width, frame.height = size.height;
        for (int k = 0; k < hp::yuv_frame::plane_count(format); ++k) {
            frame.stride[k] = (int)hp::yuv_frame::row_bytes(format, k, size.width, size.height) + pitch;
            planes.emplace_back((size_t)frame.stride[k] * hp::yuv_frame::rows(format, k, size.width, size.height), (uint8_t)0xA5);
            frame.plane[k] = planes.back().data();
        }
    }
};

int main()
{
    int compared = 0, threw = 0;
    if (hp::padded_size(HP_YUV_NV12, cv::Size(1920, 1080), 16) != cv::Size(1920, 1088) || hp::padded_size(HP_YUV_I444, cv::Size(3, 5)) != cv::Size(3, 5)
        || hp::padded_size(HP_YUV_I420, cv::Size(31, 3), 1) != cv::Size(32, 4) || hp::padded_size(HP_YUV_YUY2, cv::Size(30, 20), 16) != cv::Size(32, 32))
        return 3;
    unsigned s = 99;
    auto rnd = [&] { return (uint8_t)((s = s * 1664525u + 1013904223u) >> 24); };
    const int w = 31, h = 21;
    const int formats[] = { HP_YUV_NV12, HP_YUV_P010, HP_YUV_I422, HP_YUV_UYVY, HP_YUV_I444 };
    for (int format : formats) {
        const cv::Size size = hp::padded_size(format, cv::Size(w, h), 16);
        // an ARGB frame with a pitch
        std::vector<uint8_t> argb((size_t)(w * 4 + 12) * h);
        for (auto& b : argb)
            b = rnd();
        const hp::rgb_frame src(HP_RGB_ARGB32, argb.data(), w, h, w * 4 + 12);
        surface a(format, size, HP_YUV_BT709, HP_YUV_LIMITED, 7), b(format, size, HP_YUV_BT709, HP_YUV_LIMITED, 7);
        hp::to_yuv(src, a.frame);
        const hp_rgb_image in = src.image();
        const hp_yuv_image out = b.frame.image();
        if (hp_rgb_to_yuv_host(&in, &out) != HP_OK)
            return 4;
        if (a.planes != b.planes || a.planes[0] == std::vector<uint8_t>(a.planes[0].size(), 0xA5) || a.planes[0][(size_t)a.frame.stride[0] - 1] != 0xA5)
            return 5;
        ++compared;
        // a BGR cv::Mat
        cv::Mat bgr(h, w, CV_8UC3);
        for (size_t i = 0; i < (size_t)w * h * 3; ++i)
            bgr.data()[i] = rnd();
        surface c(format, size, HP_YUV_BT2020, HP_YUV_FULL, 2), d(format, size, HP_YUV_BT2020, HP_YUV_FULL, 2);
        hp::to_yuv(bgr, c.frame);
        const hp_rgb_image in2 = { HP_RGB_BGR24, w, h, bgr.data(), w * 3 };
        const hp_yuv_image out2 = d.frame.image();
        if (hp_rgb_to_yuv_host(&in2, &out2) != HP_OK)
            return 6;
        if (c.planes != d.planes || c.planes == a.planes)
            return 7;
        ++compared;
    }
    std::vector<uint8_t> grey(8 * 8, 128);
    const hp::rgb_frame g = hp::rgb_frame::packed(HP_RGB_GRAY8, grey.data(), 8, 8);
    auto throws = [&](hp::yuv_frame& dst, const hp::rgb_frame& src) {
        try {
            hp::to_yuv(src, dst);
        } catch (const std::logic_error&) {
            ++threw;
        }
    };
    surface small(HP_YUV_NV12, cv::Size(6, 8), 0, 0, 0), odd(HP_YUV_NV12, cv::Size(8, 8), 0, 0, 0), dev(HP_YUV_NV12, cv::Size(8, 8), 0, 0, 0);
    throws(small.frame, g); // narrower than the source
    odd.frame.height = 9;
    throws(odd.frame, g); // 4:2:0 cannot hold an odd height
    dev.frame.on_device = true;
    throws(dev.frame, g); // one frame on the device, one in host memory
    try {
        (void)hp::padded_size(HP_YUV_NV12, cv::Size(8, 8), 0);
    } catch (const std::logic_error&) {
        ++threw;
    }
    for (const surface* x : { &small, &odd, &dev })
        for (const auto& p : x->planes)
            for (uint8_t b : p)
                if (b != 0xA5)
                    return 8; // a refused call wrote
    std::printf("OK %d %d\n", compared, threw);
    return threw == 4 ? 0 : 9;
}
