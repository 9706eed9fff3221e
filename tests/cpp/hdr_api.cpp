// The C++ mirror of "HDR video in": hyperpose::hdr, dnn::tensorrt::set_tonemap / clear_tonemap and draw_humans(yuv_frame&, humans, hdr).
//   hdr_api.bin host   no device: the description's defaults and C form; draw_humans with an hdr on a HOST P010 frame gives the bytes of
//                      hp_overlay_draw_yuv_host_hdr and not those of the SDR overload; on an 8-bit frame it gives the SDR overload's bytes.
//                      Prints "HOST_OK".
//   hdr_api.bin        on the GPU: with set_tonemap, inference(std::vector<yuv_frame>) and inference(yuv_frame, regions) of P010 frames (host and
//                      device-resident, stretched and letter-boxed) return the maps of the cv::Mat overloads on the frames converted by
//                      hp_tonemap_convert_host, by memcmp; an NV12 frame in the same batch keeps its SDR maps; clear_tonemap brings the SDR
//                      maps back; a description the C ABI refuses throws and changes nothing.  Prints "OK <comparisons> <threw>".
// Run by tests/test_cpp_hdr.py.
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

namespace hp = hyperpose;

struct p010_frame {
    int w, h, pitch;
    std::vector<uint8_t> y, uv;
    hp::yuv_frame view() const
    {
        hp::yuv_frame f;
        f.format = HP_YUV_P010, f.matrix = HP_YUV_BT2020, f.range = HP_YUV_LIMITED, f.width = w, f.height = h;
        f.plane[0] = y.data(), f.plane[1] = uv.data(), f.stride[0] = f.stride[1] = w * 2 + pitch;
        return f;
    }
    cv::Mat to_bgr(const hp::hdr& h_) const
    {
        cv::Mat m(h, w);
        const hp_yuv_image im = view().image();
        const hp_hdr_desc d = h_.c_form();
        if (hp_tonemap_convert_host(&im, &d, m.data(), w * 3) != HP_OK)
            std::exit(3);
        return m;
    }
};

static p010_frame make_frame(int w, int h, int pitch, unsigned seed)
{
    p010_frame f{ w, h, pitch, {}, {} };
    unsigned s = seed * 2654435761u + 12345u;
    auto fill = [&](std::vector<uint8_t>& p, size_t n) {
        p.resize(n);
        for (auto& b : p)
            s = s * 1664525u + 1013904223u, b = (uint8_t)(s >> 24);
    };
    fill(f.y, (size_t)(w * 2 + pitch) * h);
    fill(f.uv, (size_t)(w * 2 + pitch) * (h / 2));
    return f;
}

static bool same_packet(const hp::internal_t& a, const hp::internal_t& b)
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

static bool same_maps(const std::vector<hp::internal_t>& a, const std::vector<hp::internal_t>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!same_packet(a[i], b[i]))
            return false;
    return true;
}

static std::vector<hp::human_t> one_human()
{
    hp::human_t h{};
    const float pts[5][2] = { { 0.5f, 0.2f }, { 0.5f, 0.4f }, { 0.3f, 0.45f }, { 0.25f, 0.7f }, { 0.2f, 0.9f } };
    for (int k = 0; k < 5; ++k)
        h.parts[k].has_value = true, h.parts[k].x = pts[k][0], h.parts[k].y = pts[k][1], h.parts[k].score = 1.f;
    h.score = 1.f;
    return { h };
}

static int host_part()
{
    const hp::hdr def;
    const hp_hdr_desc c = def.c_form();
    if (c.transfer != HP_TRC_PQ || c.to_bt709 != 1 || c.peak_nits != HP_HDR_DEFAULT_PEAK || c.white_nits != HP_HDR_DEFAULT_WHITE)
        return 20;
    hp::hdr hlg;
    hlg.transfer = HP_TRC_HLG, hlg.to_bt709 = false, hlg.white_nits = 100.f;
    const auto humans = one_human();
    p010_frame a = make_frame(64, 48, 6, 1), b = a, s = a;
    hp::yuv_frame fa = a.view(), fb = b.view(), fs = s.view();
    hp::draw_humans(fa, humans, hlg, 0.5f);
    const hp_yuv_image ib = fb.image();
    const hp_hdr_desc d = hlg.c_form();
    const auto list = hp::detail::to_c_humans(humans);
    if (hp_overlay_draw_yuv_host_hdr(&ib, &d, list.data(), 1, 0.5f, 0) != HP_OK)
        return 21;
    hp::draw_humans(fs, humans, 0.5f);
    if (a.y != b.y || a.uv != b.uv || a.y == s.y)
        return 22;
    // an 8-bit frame is painted as the SDR overload paints it
    std::vector<uint8_t> n1((size_t)64 * 48 * 3 / 2, 90), n2 = n1;
    hp::yuv_frame f1 = hp::yuv_frame::packed(HP_YUV_NV12, n1.data(), 64, 48), f2 = hp::yuv_frame::packed(HP_YUV_NV12, n2.data(), 64, 48);
    hp::draw_humans(f1, humans, hlg);
    hp::draw_humans(f2, humans);
    if (n1 != n2 || n1 == std::vector<uint8_t>(n1.size(), 90))
        return 23;
    bool threw = false;
    try {
        hp::hdr bad;
        bad.white_nits = 5000.f;
        hp::draw_humans(fa, humans, bad);
    } catch (const std::logic_error&) {
        threw = true;
    }
    if (!threw)
        return 24;
    std::printf("HOST_OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "host") == 0)
        return host_part();
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    int compared = 0, threw = 0;
    hp::hdr pq, hlg;
    hlg.transfer = HP_TRC_HLG, hlg.to_bt709 = false;
    for (int keep_ratio = 0; keep_ratio < 2; ++keep_ratio) {
        hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 4, keep_ratio != 0);
        const std::vector<p010_frame> frames = { make_frame(320, 240, 0, 1), make_frame(192, 160, 0, 2), make_frame(96, 80, 0, 3), make_frame(200, 120, 26, 4) };
        std::vector<hp::yuv_frame> yuv;
        for (const auto& f : frames)
            yuv.push_back(f.view());
        for (const hp::hdr& h : { pq, hlg }) {
            std::vector<cv::Mat> bgr;
            for (const auto& f : frames)
                bgr.push_back(f.to_bgr(h));
            engine.set_tonemap(h);
            const auto a = engine.inference(yuv);
            if (a.size() != 4 || !same_maps(a, engine.inference(bgr)))
                return 10 + keep_ratio;
            ++compared;
            // regions of the first frame: one packet per region, each the cut-out's
            const std::vector<cv::Rect> regions = { cv::Rect(0, 0, 320, 240), cv::Rect(32, 16, 192, 160), cv::Rect(224, 160, 96, 80) };
            const auto r = engine.inference(yuv[0], regions);
            if (!same_maps(r, engine.inference(bgr[0], regions)))
                return 12 + keep_ratio;
            ++compared;
        }
        {   // a device-resident surface and an NV12 frame in one batch: the P010 frame is tone-mapped, the NV12 frame is not
            engine.set_tonemap(pq);
            void *dy = nullptr, *duv = nullptr;
            const p010_frame& f = frames[3];
            if (hp_malloc(&dy, f.y.size()) != HP_OK || hp_malloc(&duv, f.uv.size()) != HP_OK || hp_memcpy_h2d(dy, f.y.data(), f.y.size()) != HP_OK
                || hp_memcpy_h2d(duv, f.uv.data(), f.uv.size()) != HP_OK || hp_device_synchronize() != HP_OK)
                return 14;
            hp::yuv_frame dev = f.view();
            dev.plane[0] = dy, dev.plane[1] = duv, dev.on_device = true;
            std::vector<uint8_t> nv12((size_t)200 * 120 * 3 / 2);
            unsigned s = 99;
            for (auto& b : nv12)
                s = s * 1664525u + 1013904223u, b = (uint8_t)(s >> 24);
            const hp::yuv_frame n = hp::yuv_frame::packed(HP_YUV_NV12, nv12.data(), 200, 120);
            const auto mixed = engine.inference(std::vector<hp::yuv_frame>{ dev, n });
            engine.clear_tonemap();
            const auto plain = engine.inference(std::vector<hp::yuv_frame>{ n });
            const auto converted = engine.inference(std::vector<cv::Mat>{ f.to_bgr(pq) });
            const bool nv12_same = plain.size() == 1 && same_packet(mixed[1], plain[0]);
            const bool p010_same = converted.size() == 1 && same_packet(mixed[0], converted[0]);
            hp_free(dy), hp_free(duv);
            if (!nv12_same || !p010_same)
                return 16 + keep_ratio;
            ++compared;
        }
        {   // a refused description throws and the engine keeps the one it had; clear_tonemap brings the SDR maps back
            engine.set_tonemap(pq);
            try {
                hp::hdr bad;
                bad.transfer = 9;
                engine.set_tonemap(bad);
            } catch (const std::logic_error&) {
                ++threw;
            }
            std::vector<cv::Mat> bgr;
            for (const auto& f : frames)
                bgr.push_back(f.to_bgr(pq));
            if (!same_maps(engine.inference(yuv), engine.inference(bgr)))
                return 18;
            engine.clear_tonemap(); // the SDR reading of the same code values: other maps, tone-mapping is not a no-op
            const auto plain = engine.inference(yuv);
            engine.set_tonemap(pq);
            if (same_maps(plain, engine.inference(yuv)))
                return 19;
            engine.clear_tonemap();
            ++compared;
        }
    }
    std::printf("OK %d %d\n", compared, threw);
    return 0;
}
