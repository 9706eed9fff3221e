// The C++ mirror's packed RGB / grey frames (include/hyperpose/utility/data.hpp rgb_frame; dnn::tensorrt::inference(std::vector<rgb_frame>),
// inference(rgb_frame, regions), calibrate(std::vector<rgb_frame>); hip_stream::push(std::vector<rgb_frame>)) against the cv::Mat overloads on the
// same frames converted to BGR with hp_rgb_to_bgr_host: identical packets (maps by memcmp) and identical poses, for every layout, tight and padded
// rows, host and device-resident frames, plain, under set_orientation and with the flip ensemble; too many frames and a bad description throw
// std::logic_error.  Prints "OK <comparisons> <threw>"; run by tests/test_cpp_rgb.py on the GPU box.
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

namespace hp = hyperpose;

struct host_frame {
    int format, w, h, stride;
    std::vector<uint8_t> bytes;
    hp::rgb_frame view() const { return hp::rgb_frame(format, bytes.data(), w, h, stride); }
    cv::Mat to_bgr() const
    {
        cv::Mat m(h, w);
        const hp_rgb_image im = view().image();
        if (hp_rgb_to_bgr_host(&im, m.data(), w * 3) != HP_OK)
            std::printf("hp_rgb_to_bgr_host: %s\n", hp_last_error());
        return m;
    }
};

static host_frame make_frame(int format, int w, int h, int pad, unsigned seed)
{
    host_frame f{ format, w, h, w * hp_rgb_pixel_bytes(format) + pad, {} };
    unsigned s = seed * 2654435761u + 12345u;
    f.bytes.resize((size_t)f.stride * h);
    for (auto& b : f.bytes)
        s = s * 1664525u + 1013904223u, b = (uint8_t)(s >> 24);
    return f;
}

static bool same_maps(const std::vector<hp::internal_t>& a, const std::vector<hp::internal_t>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].size() != b[i].size())
            return false;
        for (size_t k = 0; k < a[i].size(); ++k) {
            if (a[i][k].shape() != b[i][k].shape() || a[i][k].name() != b[i][k].name())
                return false;
            size_t n = sizeof(float);
            for (int d : a[i][k].shape())
                n *= (size_t)d;
            if (std::memcmp(a[i][k].view<float>(), b[i][k].view<float>(), n) != 0)
                return false;
        }
    }
    return true;
}

template <class F> static bool throws_logic_error(F f)
{
    try {
        f();
    } catch (const std::logic_error&) {
        return true;
    }
    return false;
}

int main()
{
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    const int formats[7] = { HP_RGB_BGR24, HP_RGB_RGB24, HP_RGB_BGRA32, HP_RGB_RGBA32, HP_RGB_ARGB32, HP_RGB_ABGR32, HP_RGB_GRAY8 };
    int compared = 0, threw = 0;
    for (int keep_ratio = 0; keep_ratio < 2; ++keep_ratio) {
        hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 4, keep_ratio != 0);
        for (int format : formats) {
            // camera-sized, a 2x down-scale (area mode), network-sized, and padded rows (an odd pitch: a host frame has no alignment rule)
            const std::vector<host_frame> frames = { make_frame(format, 320, 240, 0, 1), make_frame(format, 192, 160, 0, 2), make_frame(format, 96, 80, 0, 3),
                make_frame(format, 201, 121, 13, 4) };
            std::vector<hp::rgb_frame> rgb;
            std::vector<cv::Mat> bgr;
            for (const auto& f : frames)
                rgb.push_back(f.view()), bgr.push_back(f.to_bgr());
            if (!same_maps(engine.inference(rgb), engine.inference(bgr)))
                return 10 + keep_ratio;
            if (!same_maps(engine.inference(std::vector<hp::rgb_frame>{ hp::rgb_frame::packed(format, frames[0].bytes.data(), 320, 240) }),
                    engine.inference(std::vector<cv::Mat>{ bgr[0] })))
                return 12 + keep_ratio;
            // regions of one frame, one of them ending in the bottom-right pixel
            const std::vector<cv::Rect> regions = { cv::Rect(0, 0, 320, 240), cv::Rect(33, 17, 192, 160), cv::Rect(224, 160, 96, 80) };
            if (!same_maps(engine.inference(rgb[0], regions), engine.inference(bgr[0], regions)))
                return 14 + keep_ratio;
            compared += 3;
        }
        // a device-resident frame with a pitch that is a multiple of 4
        const host_frame f = make_frame(HP_RGB_ARGB32, 200, 120, 16, 5);
        void* dev = nullptr;
        if (hp_malloc(&dev, f.bytes.size()) != HP_OK || hp_memcpy_h2d(dev, f.bytes.data(), f.bytes.size()) != HP_OK)
            return 3;
        const hp::rgb_frame on_device(HP_RGB_ARGB32, dev, 200, 120, f.stride, true);
        if (!same_maps(engine.inference(std::vector<hp::rgb_frame>{ on_device }), engine.inference(std::vector<cv::Mat>{ f.to_bgr() })))
            return 16 + keep_ratio;
        // stored turned: both overloads read the frame upright
        engine.set_orientation(hp::orientation::from_code(HP_ORIENT_HFLIP_CW90));
        if (!same_maps(engine.inference(std::vector<hp::rgb_frame>{ on_device, f.view() }), engine.inference(std::vector<cv::Mat>{ f.to_bgr(), f.to_bgr() })))
            return 18 + keep_ratio;
        if (!same_maps(engine.inference(f.view(), { cv::Rect(1, 3, 119, 197) }), engine.inference(f.to_bgr(), { cv::Rect(1, 3, 119, 197) })))
            return 20 + keep_ratio;
        engine.set_orientation(hp::orientation{});
        engine.set_flip_ensemble(true);
        if (!same_maps(engine.inference(std::vector<hp::rgb_frame>{ f.view(), on_device }), engine.inference(std::vector<cv::Mat>{ f.to_bgr(), f.to_bgr() })))
            return 22 + keep_ratio;
        threw += throws_logic_error([&] { engine.inference(std::vector<hp::rgb_frame>(3, f.view())); }); // 3 > 4 / 2 under the flip ensemble
        engine.set_flip_ensemble(false);
        compared += 4;
        threw += throws_logic_error([&] { engine.inference(std::vector<hp::rgb_frame>(5, f.view())); });
        threw += throws_logic_error([&] { engine.inference(std::vector<hp::rgb_frame>{ hp::rgb_frame(9, f.bytes.data(), 200, 120, f.stride) }); });
        threw += throws_logic_error([&] { engine.inference(std::vector<hp::rgb_frame>{ hp::rgb_frame(HP_RGB_ARGB32, f.bytes.data(), 200, 120, 799) }); });
        threw += throws_logic_error([&] { engine.inference(std::vector<hp::rgb_frame>{ hp::rgb_frame(HP_RGB_ARGB32, nullptr, 200, 120, 800) }); });
        // a device plane of 4-byte pixels at an address that is no multiple of 4: the C ABI's refusal
        threw += throws_logic_error([&] { engine.inference(std::vector<hp::rgb_frame>{ hp::rgb_frame(HP_RGB_ARGB32, (const uint8_t*)dev + 2, 199, 120, f.stride, true) }); });
        threw += throws_logic_error([&] { engine.inference(f.view(), { cv::Rect(150, 0, 51, 10) }); }); // not inside the frame
        if (!engine.inference(std::vector<hp::rgb_frame>{}).empty())
            return 6;
        hp_free(dev);
    }
    {   // kINT8: calibrating from RGBA frames == calibrating from the converted frames
        const std::vector<host_frame> frames = { make_frame(HP_RGB_RGBA32, 160, 120, 4, 21), make_frame(HP_RGB_GRAY8, 96, 80, 0, 22) };
        std::vector<hp::rgb_frame> rgb;
        std::vector<cv::Mat> bgr;
        for (const auto& f : frames)
            rgb.push_back(f.view()), bgr.push_back(f.to_bgr());
        hp::dnn::tensorrt q1(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 2, false, hp::data_type::kINT8);
        hp::dnn::tensorrt q2(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 2, false, hp::data_type::kINT8);
        threw += throws_logic_error([&] { q1.inference(rgb); });
        q1.calibrate(rgb);
        q2.calibrate(bgr);
        if (!q1.calibrated() || !same_maps(q1.inference(rgb), q2.inference(bgr)))
            return 41;
        ++compared;
    }
    {   // the stream: a batch of rgb_frames returns the poses of the converted cv::Mat batch
        hp::hip_stream stream(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 4, /*keep_ratio*/ true, /*n_pipes*/ 2);
        const std::vector<host_frame> frames = { make_frame(HP_RGB_BGRA32, 320, 240, 0, 31), make_frame(HP_RGB_RGB24, 201, 121, 5, 32),
            make_frame(HP_RGB_GRAY8, 96, 80, 3, 33) };
        std::vector<hp::rgb_frame> rgb;
        std::vector<cv::Mat> bgr;
        for (const auto& f : frames)
            rgb.push_back(f.view()), bgr.push_back(f.to_bgr());
        stream.push(rgb);
        stream.push(bgr);
        const auto a = stream.pop(), b = stream.pop();
        if (a.size() != 3 || b.size() != 3)
            return 50;
        for (size_t i = 0; i < 3; ++i) {
            if (a[i].size() != b[i].size())
                return 51;
            for (size_t k = 0; k < a[i].size(); ++k) {
                if (std::memcmp(&a[i][k].score, &b[i][k].score, sizeof(float)) != 0)
                    return 52;
                for (size_t j = 0; j < a[i][k].parts.size(); ++j) {
                    const hp::body_part_t &p = a[i][k].parts[j], &q = b[i][k].parts[j];
                    if (p.has_value != q.has_value || std::memcmp(&p.x, &q.x, sizeof(float)) || std::memcmp(&p.y, &q.y, sizeof(float))
                        || std::memcmp(&p.score, &q.score, sizeof(float)))
                        return 53;
                }
            }
        }
        ++compared;
        std::vector<hp::rgb_frame> mixed = rgb;
        mixed[1].on_device = true;
        threw += throws_logic_error([&] { stream.push(mixed); });
    }
    std::printf("OK %d %d\n", compared, threw);
    return 0;
}
