// The C++ mirror of "upright input": hyperpose::orientation, oriented_size, to_stored / to_upright, draw_humans(.., orientation) and
// dnn::tensorrt::set_orientation.
//   orientation_api.bin host   no device: the type's code, from_code and from_exif agree with the C ABI for all eight codes; oriented_size is
//                              hp_oriented_size; to_stored / to_upright give the floats of hp_humans_orient and leave absent parts and scores alone;
//                              draw_humans with an orientation on a HOST NV12 frame gives the bytes of hp_overlay_draw_yuv_host on the to_stored
//                              records; bad arguments throw.  Prints "HOST_OK".
//   orientation_api.bin        on the GPU: with set_orientation, inference(std::vector<cv::Mat>), inference(std::vector<yuv_frame>) and
//                              inference(frame, regions) of stored frames return the maps of the same calls on the frames oriented by
//                              hp_orient_u8c3_host, by memcmp.  Prints "OK <comparisons>".
// Run by tests/test_cpp_orientation.py.
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

namespace hp = hyperpose;

static std::vector<hp::human_t> some_humans()
{
    std::vector<hp::human_t> out(2);
    unsigned s = 7;
    for (auto& h : out) {
        h = hp::human_t{};
        for (int k = 0; k < hp::COCO_N_PARTS; ++k) {
            s = s * 1664525u + 1013904223u;
            h.parts[k].has_value = (s >> 20) % 3 != 0;
            h.parts[k].x = (float)((s >> 8) & 0xffff) / 65535.f, h.parts[k].y = (float)((s >> 4) & 0xfff) / 4095.f, h.parts[k].score = 0.25f * (k + 1);
        }
        h.score = 3.5f;
    }
    out[0].parts[0].has_value = false, out[0].parts[1].has_value = true;
    return out;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int host_part()
{
    if (!hp::orientation{}.upright() || hp::orientation{}.code() != HP_ORIENT_NONE)
        return 20;
    const int exif_codes[8] = { 0, 4, 2, 6, 7, 1, 5, 3 };
    for (int e = 1; e <= 8; ++e)
        if (hp::orientation::from_exif(e).code() != exif_codes[e - 1] || hp_orientation_from_exif(e) != exif_codes[e - 1])
            return 21;
    const auto humans = some_humans();
    const auto list = hp::detail::to_c_humans(humans);
    for (int code = 0; code < 8; ++code) {
        const hp::orientation o = hp::orientation::from_code(code);
        if (o.code() != code || o.quarter_turns != (code & 3) || o.mirrored != (code >= 4))
            return 22;
        int uw = 0, uh = 0;
        const cv::Size u = hp::oriented_size(cv::Size(7, 5), o);
        if (hp_oriented_size(code, 7, 5, &uw, &uh) != HP_OK || u.width != uw || u.height != uh || uw != (code & 1 ? 5 : 7))
            return 23;
        for (int to_stored = 0; to_stored < 2; ++to_stored) {
            auto mine = humans;
            to_stored ? hp::to_stored(mine, o) : hp::to_upright(mine, o);
            auto c = list;
            if (hp_humans_orient(c.data(), (int)c.size(), code, to_stored) != HP_OK)
                return 24;
            for (size_t i = 0; i < mine.size(); ++i) {
                if (!same_bits(mine[i].score, humans[i].score))
                    return 25;
                for (int k = 0; k < hp::COCO_N_PARTS; ++k) {
                    const auto &p = mine[i].parts[k], &was = humans[i].parts[k];
                    if (!same_bits(p.x, c[i].parts[k].x) || !same_bits(p.y, c[i].parts[k].y) || !same_bits(p.score, was.score) || p.has_value != was.has_value)
                        return 26;
                    if (!was.has_value && (!same_bits(p.x, was.x) || !same_bits(p.y, was.y)))
                        return 27;
                }
            }
        }
        // upright humans drawn into the stored frame
        std::vector<uint8_t> n1((size_t)64 * 48 * 3 / 2, 90), n2 = n1;
        hp::yuv_frame f1 = hp::yuv_frame::packed(HP_YUV_NV12, n1.data(), 64, 48), f2 = hp::yuv_frame::packed(HP_YUV_NV12, n2.data(), 64, 48);
        hp::draw_humans(f1, humans, o);
        auto c = list;
        const hp_yuv_image im = f2.image();
        if (hp_humans_orient(c.data(), (int)c.size(), code, 1) != HP_OK || hp_overlay_draw_yuv_host(&im, c.data(), (int)c.size(), 1.f, 0) != HP_OK)
            return 28;
        if (n1 != n2 || n1 == std::vector<uint8_t>(n1.size(), 90))
            return 29;
    }
    int threw = 0;
    try {
        hp::orientation::from_exif(9);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        hp::oriented_size(cv::Size(0, 5), hp::orientation{ 1, false });
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    if (threw != 2)
        return 30;
    std::printf("HOST_OK\n");
    return 0;
}

static bool same_maps(const std::vector<hp::internal_t>& a, const std::vector<hp::internal_t>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].size() != b[i].size())
            return false;
        for (size_t k = 0; k < a[i].size(); ++k) {
            if (a[i][k].shape() != b[i][k].shape())
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

static cv::Mat random_mat(int w, int h, unsigned seed)
{
    cv::Mat m(h, w);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < (size_t)w * h * 3; ++i)
        s = s * 1664525u + 1013904223u, m.data()[i] = (uint8_t)(s >> 24);
    return m;
}

static cv::Mat upright_of(const cv::Mat& stored, const hp::orientation& o)
{
    const cv::Size u = hp::oriented_size(cv::Size(stored.cols, stored.rows), o);
    cv::Mat m(u.height, u.width);
    if (hp_orient_u8c3_host(stored.data(), stored.cols, stored.rows, stored.cols * 3, o.code(), m.data(), u.width * 3) != HP_OK)
        std::exit(3);
    return m;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "host") == 0)
        return host_part();
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    int compared = 0;
    for (int keep_ratio = 0; keep_ratio < 2; ++keep_ratio) {
        hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 4, keep_ratio != 0);
        const std::vector<cv::Mat> stored = { random_mat(200, 120, 1), random_mat(96, 80, 2), random_mat(80, 96, 3) };
        // an I444 frame's BGR reading is what the engine makes of it: the reference of the yuv_frame overload is the cv::Mat overload on that
        std::vector<uint8_t> i444((size_t)64 * 48 * 3);
        unsigned s = 5;
        for (auto& b : i444)
            s = s * 1664525u + 1013904223u, b = (uint8_t)(s >> 24);
        const hp::yuv_frame yuv = hp::yuv_frame::packed(HP_YUV_I444, i444.data(), 64, 48);
        for (int code : { 1, 2, 6, 7 }) {
            const hp::orientation o = hp::orientation::from_code(code);
            std::vector<cv::Mat> upright;
            for (const auto& m : stored)
                upright.push_back(upright_of(m, o));
            engine.set_orientation(hp::orientation{});
            const auto want = engine.inference(upright);
            const cv::Size u0 = hp::oriented_size(cv::Size(200, 120), o);
            const std::vector<cv::Rect> regions = { cv::Rect(0, 0, u0.width, u0.height), cv::Rect(8, 4, 96, 80), cv::Rect(u0.width - 48, u0.height - 40, 48, 40) };
            const auto want_regions = engine.inference(upright[0], regions);
            engine.set_orientation(o);
            if (want.size() != 3 || !same_maps(engine.inference(stored), want))
                return 10 + keep_ratio;
            ++compared;
            if (!same_maps(engine.inference(stored[0], regions), want_regions))
                return 12 + keep_ratio;
            ++compared;
            // the yuv_frame overloads against themselves through the regions call: the whole upright frame as one region is the per-frame call
            const cv::Size uy = hp::oriented_size(cv::Size(64, 48), o);
            const auto a = engine.inference(std::vector<hp::yuv_frame>{ yuv });
            const auto b = engine.inference(yuv, std::vector<cv::Rect>{ cv::Rect(0, 0, uy.width, uy.height) });
            if (a.size() != 1 || !same_maps(a, b))
                return 14 + keep_ratio;
            ++compared;
        }
        engine.set_orientation(hp::orientation{});
    }
    std::printf("OK %d\n", compared);
    return 0;
}
