// Tiled inference through the C++ mirror.  Host half (`tiles.bin --host`, no device): hyperpose::plan_tiles, to_frame and merge_humans
// equal hp_tile_plan, hp_humans_to_frame and hp_humans_merge.  Device half: dnn::tensorrt::inference(frame, regions) returns, per region,
// the maps of inference() on that region cut out into a frame of its own, by memcmp - for a cv::Mat and for an NV12 yuv_frame whose
// cut-outs are views of its sub-planes - stretched and letter-boxed; more regions than max_batch_size throw.
// Prints "HOST_OK <checks>" / "OK <comparisons> <threw>"; run by tests/test_cpp_tiles.py.
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

namespace hp = hyperpose;

static unsigned lcg(unsigned& s) { return (s = s * 1664525u + 1013904223u) >> 8; }

static bool same_maps(const hp::internal_t& a, const hp::internal_t& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t k = 0; k < a.size(); ++k) {
        if (a[k].shape() != b[k].shape() || a[k].name() != b[k].name())
            return false;
        size_t n = sizeof(float);
        for (int d : a[k].shape())
            n *= (size_t)d;
        if (std::memcmp(a[k].view<float>(), b[k].view<float>(), n) != 0)
            return false;
    }
    return true;
}

static int host_half()
{
    int checks = 0;
    // the planner
    hp::tiling t;
    t.cols = 3, t.rows = 2, t.overlap_x = 33, t.overlap_y = 7, t.with_full = true;
    for (int format : { -1, (int)HP_YUV_NV12, (int)HP_YUV_YUY2 }) {
        int ax = 1, ay = 1;
        if (format >= 0)
            hp_yuv_roi_alignment(format, &ax, &ay);
        const hp_tiling c = t.c_form();
        hp_roi want[64];
        const int n = hp_tile_plan(&c, 1920, 1080, ax, ay, want, 64);
        const std::vector<cv::Rect> got = hp::plan_tiles(cv::Size(1920, 1080), t, format);
        if (n != 7 || (int)got.size() != n)
            return 10;
        for (int i = 0; i < n; ++i)
            if (!(got[i] == cv::Rect(want[i].x, want[i].y, want[i].w, want[i].h)))
                return 11;
        ++checks;
    }
    try {
        hp::plan_tiles(cv::Size(1921, 1080), t, HP_YUV_NV12);
        return 12;
    } catch (const std::invalid_argument&) {
        ++checks;
    }
    // seeded humans: two regions see the same people, the second with a small offset and fewer parts
    unsigned s = 99;
    std::vector<hp::human_t> humans;
    std::vector<int> region;
    for (int person = 0; person < 9; ++person) {
        const float cx = 0.1f + 0.09f * person, cy = 0.2f + 0.05f * (person % 4);
        for (int r = 0; r < 3; ++r) {
            hp::human_t h{};
            h.score = (float)(lcg(s) % 7);
            for (int k = 0; k < hp::COCO_N_PARTS; ++k)
                if (lcg(s) % 4 != 0)
                    h.parts[k] = hp::body_part_t{ true, cx + 0.002f * k + 0.0005f * r, cy + 0.006f * k, (float)(lcg(s) % 100) / 100.f };
            humans.push_back(h), region.push_back(r == 2 ? 0 : r); // two of the three share a region
        }
    }
    std::vector<hp_human> in(humans.size()), out(humans.size());
    std::memcpy((void*)in.data(), humans.data(), sizeof(hp_human) * humans.size()); // same 292-byte layout (bool in its 4-byte slot, padding zeroed by {})
    for (size_t i = 0; i < in.size(); ++i)
        for (auto& p : in[i].parts)
            p.has_value = p.has_value & 1;
    std::vector<int32_t> reg(region.begin(), region.end());
    const int n = hp_humans_merge(in.data(), reg.data(), (int)in.size(), 1280, 720, 3, 0.1, out.data(), (int)out.size());
    const std::vector<hp::human_t> merged = hp::merge_humans(humans, region, cv::Size(1280, 720), 3, 0.1);
    if (n <= 0 || n >= (int)humans.size() || (int)merged.size() != n)
        return 20;
    for (int i = 0; i < n; ++i) {
        if (merged[i].score != out[i].score)
            return 21;
        for (int k = 0; k < hp::COCO_N_PARTS; ++k) {
            const auto& a = merged[i].parts[k];
            const auto& b = out[i].parts[k];
            if (a.has_value != (b.has_value != 0) || std::memcmp(&a.x, &b.x, 4) || std::memcmp(&a.y, &b.y, 4) || std::memcmp(&a.score, &b.score, 4))
                return 22;
        }
    }
    ++checks;
    // the way back
    const hp_roi roi{ 320, 96, 704, 416 };
    std::vector<hp_human> back = in;
    hp_humans_to_frame(back.data(), (int)back.size(), &roi, 1280, 720);
    for (size_t i = 0; i < humans.size(); ++i) {
        hp::human_t h = humans[i];
        hp::to_frame(h, cv::Rect(roi.x, roi.y, roi.w, roi.h), cv::Size(1280, 720));
        for (int k = 0; k < hp::COCO_N_PARTS; ++k)
            if (std::memcmp(&h.parts[k].x, &back[i].parts[k].x, 4) || std::memcmp(&h.parts[k].y, &back[i].parts[k].y, 4))
                return 30;
        hp::human_t same = humans[i];
        hp::to_frame(same, cv::Rect(0, 0, 1280, 720), cv::Size(1280, 720));
        for (int k = 0; k < hp::COCO_N_PARTS; ++k)
            if (std::memcmp(&same.parts[k].x, &humans[i].parts[k].x, 4) || std::memcmp(&same.parts[k].y, &humans[i].parts[k].y, 4))
                return 31;
    }
    ++checks;
    std::printf("HOST_OK %d\n", checks);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0)
        return host_half();
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    const int W = 320, H = 180;
    unsigned s = 5;
    cv::Mat frame(H, W);
    for (size_t i = 0; i < (size_t)W * H * 3; ++i)
        frame.data()[i] = (uint8_t)lcg(s);
    std::vector<uint8_t> nv12((size_t)W * H * 3 / 2);
    for (auto& b : nv12)
        b = (uint8_t)lcg(s);
    int compared = 0, threw = 0;
    for (int keep_ratio = 0; keep_ratio < 2; ++keep_ratio) {
        hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 6, keep_ratio != 0);
        hp::tiling t;
        t.cols = 2, t.rows = 2, t.overlap_x = 32, t.overlap_y = 16, t.with_full = true;
        {   // BGR: the whole frame, four tiles and one region of the network's own size
            std::vector<cv::Rect> regions = hp::plan_tiles(frame.size(), t);
            regions.emplace_back(101, 33, 96, 80);
            const auto packets = engine.inference(frame, regions);
            if (packets.size() != regions.size())
                return 40;
            // (the packets stay valid: they copy themselves to the host when the engine's buffers are re-used by the next call)
            for (size_t i = 0; i < regions.size(); ++i) {
                const cv::Rect& r = regions[i];
                cv::Mat cut(r.height, r.width);
                for (int y = 0; y < r.height; ++y)
                    std::memcpy(cut.data() + (size_t)y * r.width * 3, frame.data() + ((size_t)(r.y + y) * W + r.x) * 3, (size_t)r.width * 3);
                const auto one = engine.inference(std::vector<cv::Mat>{ cut });
                if (one.size() != 1 || !same_maps(packets[i], one[0])) {
                    std::printf("BGR region %zu differs (keep_ratio %d)\n", i, keep_ratio);
                    return 41;
                }
                ++compared;
            }
        }
        {   // NV12 in host memory: the cut-outs are views of the frame's sub-planes
            const hp::yuv_frame whole = hp::yuv_frame::packed(HP_YUV_NV12, nv12.data(), W, H, HP_YUV_BT709, HP_YUV_LIMITED);
            const std::vector<cv::Rect> regions = hp::plan_tiles(cv::Size(W, H), t, HP_YUV_NV12);
            const auto packets = engine.inference(whole, regions);
            for (size_t i = 0; i < regions.size(); ++i) {
                const cv::Rect& r = regions[i];
                hp::yuv_frame cut = whole;
                cut.width = r.width, cut.height = r.height;
                cut.plane[0] = (const uint8_t*)whole.plane[0] + (size_t)r.y * whole.stride[0] + r.x;
                cut.plane[1] = (const uint8_t*)whole.plane[1] + (size_t)(r.y / 2) * whole.stride[1] + r.x;
                const auto one = engine.inference(std::vector<hp::yuv_frame>{ cut });
                if (one.size() != 1 || !same_maps(packets[i], one[0])) {
                    std::printf("NV12 region %zu differs (keep_ratio %d)\n", i, keep_ratio);
                    return 42;
                }
                ++compared;
            }
        }
        try {
            engine.inference(frame, std::vector<cv::Rect>(7, cv::Rect(0, 0, 32, 32)));
        } catch (const std::logic_error&) {
            ++threw;
        }
        try {
            engine.inference(frame, std::vector<cv::Rect>{ cv::Rect(300, 0, 32, 32) });
        } catch (const std::logic_error&) {
            ++threw;
        }
    }
    std::printf("OK %d %d\n", compared, threw);
    return 0;
}
