// dnn::tensorrt::inference(std::vector<yuv420_frame>) against the cv::Mat overload on the same frames converted on the CPU with OpenCV's
// fixed-point BT.601 arithmetic (restated from its constants, as in tests/yuv_ref.py): the maps must be equal by memcmp, for NV12 and
// I420, stretched and letter-boxed, camera-sized, network-sized and padded-pitch frames; an over-size batch throws; a kINT8 engine
// calibrated from YUV frames equals one calibrated from the converted frames.
// Prints "OK <comparisons> <threw>"; run by tests/test_cpp_yuv.py on the GPU box.
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

namespace hp = hyperpose;

static uint8_t sat8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

struct host_frame {
    int format, w, h, pitch; // pitch: extra bytes at the end of every plane row
    std::vector<uint8_t> y, u, v; // NV12: u holds the interleaved plane
    hp::yuv420_frame view() const
    {
        hp::yuv420_frame f;
        f.format = format, f.width = w, f.height = h;
        f.y = y.data(), f.u = u.data(), f.v = format == HP_YUV_I420 ? v.data() : nullptr;
        f.y_stride = w + pitch, f.uv_stride = (format == HP_YUV_NV12 ? w : w / 2) + pitch;
        return f;
    }
    void sample(int px, int py, int& Y, int& U, int& V) const
    {
        Y = y[(size_t)py * (w + pitch) + px];
        if (format == HP_YUV_NV12) {
            const uint8_t* p = u.data() + (size_t)(py / 2) * (w + pitch) + (px / 2) * 2;
            U = p[0], V = p[1];
        } else {
            const size_t at = (size_t)(py / 2) * (w / 2 + pitch) + px / 2;
            U = u[at], V = v[at];
        }
    }
    cv::Mat to_bgr() const
    {
        cv::Mat m(h, w);
        for (int py = 0; py < h; ++py)
            for (int px = 0; px < w; ++px) {
                int Y, U, V;
                sample(px, py, Y, U, V);
                const int yy = (Y > 16 ? Y - 16 : 0) * 1220542 + (1 << 19), uu = U - 128, vv = V - 128;
                uint8_t* d = m.data() + ((size_t)py * w + px) * 3;
                d[0] = sat8((yy + 2116026 * uu) >> 20);
                d[1] = sat8((yy - 852492 * vv - 409993 * uu) >> 20);
                d[2] = sat8((yy + 1673527 * vv) >> 20);
            }
        return m;
    }
};

static host_frame make_frame(int format, int w, int h, int pitch, unsigned seed)
{
    host_frame f{ format, w, h, pitch, {}, {}, {} };
    unsigned s = seed * 2654435761u + 12345u;
    auto fill = [&](std::vector<uint8_t>& p, size_t n) {
        p.resize(n);
        for (auto& b : p)
            s = s * 1664525u + 1013904223u, b = (uint8_t)(s >> 24);
    };
    fill(f.y, (size_t)(w + pitch) * h);
    if (format == HP_YUV_NV12)
        fill(f.u, (size_t)(w + pitch) * (h / 2));
    else
        fill(f.u, (size_t)(w / 2 + pitch) * (h / 2)), fill(f.v, (size_t)(w / 2 + pitch) * (h / 2));
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

int main()
{
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    int compared = 0;
    for (int keep_ratio = 0; keep_ratio < 2; ++keep_ratio) {
        hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 4, keep_ratio != 0);
        for (int format : { HP_YUV_NV12, HP_YUV_I420 }) {
            // camera-sized, a 2x down-scale (area mode), network-sized (conversion alone), and a padded-pitch surface
            const std::vector<host_frame> frames = { make_frame(format, 320, 240, 0, 1), make_frame(format, 192, 160, 0, 2), make_frame(format, 96, 80, 0, 3),
                make_frame(format, 200, 120, 24, 4) };
            std::vector<hp::yuv420_frame> yuv;
            std::vector<cv::Mat> bgr;
            for (const auto& f : frames)
                yuv.push_back(f.view()), bgr.push_back(f.to_bgr());
            const auto a = engine.inference(yuv);
            const auto b = engine.inference(bgr);
            if (a.size() != 4 || !same_maps(a, b))
                return 10 + keep_ratio * 2 + format;
            // all frames network-sized: the cv::Mat overload then uploads the batch in one copy, the YUV one still converts on the device
            std::vector<hp::yuv420_frame> yuv_net(3, frames[2].view());
            std::vector<cv::Mat> bgr_net(3, bgr[2]);
            if (!same_maps(engine.inference(yuv_net), engine.inference(bgr_net)))
                return 20 + keep_ratio * 2 + format;
            // the packed() helper describes one contiguous buffer
            const host_frame& p = frames[0];
            std::vector<uint8_t> flat(p.y);
            flat.insert(flat.end(), p.u.begin(), p.u.end());
            flat.insert(flat.end(), p.v.begin(), p.v.end());
            if (!same_maps(engine.inference(std::vector<hp::yuv420_frame>{ hp::yuv420_frame::packed(format, flat.data(), p.w, p.h) }), engine.inference(std::vector<cv::Mat>{ bgr[0] })))
                return 30 + keep_ratio * 2 + format;
            compared += 3;
        }
        bool threw = false;
        const host_frame f = make_frame(HP_YUV_NV12, 64, 48, 0, 9);
        try {
            engine.inference(std::vector<hp::yuv420_frame>(5, f.view()));
        } catch (const std::logic_error&) {
            threw = true;
        }
        if (!threw)
            return 4;
        threw = false;
        try { // odd sizes are refused before anything is launched
            hp::yuv420_frame odd = f.view();
            odd.width = 63;
            engine.inference(std::vector<hp::yuv420_frame>{ odd });
        } catch (const std::logic_error&) {
            threw = true;
        }
        if (!threw)
            return 5;
        if (!engine.inference(std::vector<hp::yuv420_frame>{}).empty())
            return 6;
    }
    {   // kINT8: inference before calibration throws for YUV frames too; calibrating from YUV frames == calibrating from the converted frames
        const std::vector<host_frame> frames = { make_frame(HP_YUV_NV12, 160, 120, 0, 21), make_frame(HP_YUV_NV12, 96, 80, 0, 22) };
        std::vector<hp::yuv420_frame> yuv;
        std::vector<cv::Mat> bgr;
        for (const auto& f : frames)
            yuv.push_back(f.view()), bgr.push_back(f.to_bgr());
        hp::dnn::tensorrt q1(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 2, false, hp::data_type::kINT8);
        hp::dnn::tensorrt q2(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 2, false, hp::data_type::kINT8);
        bool threw = false;
        try {
            q1.inference(yuv);
        } catch (const std::logic_error&) {
            threw = true;
        }
        if (!threw || q1.calibrated())
            return 40;
        q1.calibrate(yuv);
        q2.calibrate(bgr);
        if (!q1.calibrated() || !same_maps(q1.inference(yuv), q2.inference(bgr)))
            return 41;
        ++compared;
        threw = false;
        try {
            hp::dnn::tensorrt f32(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 2);
            f32.calibrate(yuv);
        } catch (const std::logic_error&) {
            threw = true;
        }
        if (!threw)
            return 42;
    }
    std::printf("OK %d %d\n", compared, 1);
    return 0;
}
