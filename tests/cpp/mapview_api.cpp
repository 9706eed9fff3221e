// hyperpose::draw_maps (include/hyperpose/utility/map_view.hpp) on what an engine returned: a letter-boxing lw_openpose_mobilenet engine infers two
// P010 frames with padded pitch; the confidence maps (max) and the part-affinity fields (field) of frame 1 are drawn into the frame in DEVICE memory
// - read from the engine's output where it lies - and into the same frame in HOST memory from the host copy: the same bytes, padding included.
// After the engine's next inference the device view is gone and the device call goes through a staged copy: the same bytes again.  The device_bgr
// form equals the C ABI's host BGR twin; an opacity of 0 throws.  Prints "OK <comparisons> <threw>"; run by tests/test_cpp_mapview.py on the GPU box.
#include "frame_fixture.hpp"

#include <cstdio>
#include <cstring>

namespace hp = hyperpose;

int main()
{
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    int compared = 0, threw = 0;
    const int w = 200, h = 120, pitch = 26, s0 = w * 2 + pitch, s1 = w * 2 + pitch;
    hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_mobilenet", {}, 7 }, cv::Size(96, 80), 2, /*keep_ratio*/ true);
    const hp::map_cover cover = engine.map_cover(cv::Size(w, h));
    if (!(cover[0] == 1. && cover[1] > 0.5 && cover[1] < 1.))
        return 3;
    std::vector<std::vector<uint8_t>> y, uv;
    std::vector<hp::yuv_frame> frames;
    for (unsigned i = 0; i < 2; ++i) {
        y.push_back(noise((size_t)s0 * h, 1 + i, true)), uv.push_back(noise((size_t)s1 * (h / 2), 5 + i, true));
        hp::yuv_frame f;
        f.format = HP_YUV_P010, f.matrix = HP_YUV_BT709, f.range = HP_YUV_LIMITED, f.width = w, f.height = h;
        f.plane[0] = y[i].data(), f.plane[1] = uv[i].data(), f.stride[0] = s0, f.stride[1] = s1;
        frames.push_back(f);
    }
    auto maps = engine.inference(frames);
    if (maps.size() != 2 || maps[1].size() < 2)
        return 4;
    hp::map_view conf, paf;
    conf.gain = 40.f, conf.alpha = hp::map_view::scaled, conf.opacity = 1.f; // seeded weights give small maps
    paf.mode = hp::map_view::field, paf.palette = hp::map_view::heat, paf.gain = 40.f;
    for (int pass = 0; pass < 2; ++pass) { // pass 1: after another inference, the maps' device view is no longer valid
        for (const hp::map_view& v : { conf, paf }) {
            const hp::feature_map_t* map = nullptr;
            for (const auto& m : maps[1])
                if (m.shape().size() == 3 && m.shape()[0] == (v.mode == hp::map_view::field ? 38 : 19))
                    map = &m;
            if (!map || (pass == 0) != (map->device_batch() != nullptr))
                return 5;
            std::vector<uint8_t> p0 = y[1], p1 = uv[1];
            void *d0 = nullptr, *d1 = nullptr;
            if (hp_malloc(&d0, p0.size()) != HP_OK || hp_malloc(&d1, p1.size()) != HP_OK || hp_memcpy_h2d(d0, p0.data(), p0.size()) != HP_OK
                || hp_memcpy_h2d(d1, p1.data(), p1.size()) != HP_OK)
                return 10;
            hp::yuv_frame host = frames[1];
            host.plane[0] = p0.data(), host.plane[1] = p1.data();
            hp::yuv_frame dev = host;
            dev.plane[0] = d0, dev.plane[1] = d1, dev.on_device = true;
            hp::draw_maps(dev, *map, cover, v);
            hp::draw_maps(host, *map, cover, v);
            std::vector<uint8_t> g0(p0.size()), g1(p1.size());
            if (hp_device_synchronize() != HP_OK || hp_memcpy_d2h(g0.data(), d0, g0.size()) != HP_OK || hp_memcpy_d2h(g1.data(), d1, g1.size()) != HP_OK)
                return 11;
            hp_free(d0), hp_free(d1);
            if (g0 != p0 || g1 != p1)
                return 12;
            if (p0 == y[1] || p1 == uv[1])
                return 13; // nothing was painted
            ++compared;
            if (pass)
                continue;
            // 8-bit BGR in device memory, stored turned, against the host BGR twin of the C ABI on the host copy of the same map
            const int sb = w * 3 + 7;
            std::vector<uint8_t> bgr = noise((size_t)sb * h, 3, false), got(bgr.size());
            void* db = nullptr;
            if (hp_malloc(&db, bgr.size()) != HP_OK || hp_memcpy_h2d(db, bgr.data(), bgr.size()) != HP_OK)
                return 14;
            const hp::orientation turned{ 1, true };
            hp::draw_maps(hp::device_bgr{ (uint8_t*)db, w, h, sb }, *map, cover, turned, v);
            hp::detail::mapview_call c;
            hp::detail::mapview_prepare(c, *map, cover, v, turned.code(), false);
            if (hp_mapview_draw_u8c3_host(bgr.data(), w, h, sb, &c.d, c.palette, v.opacity) != HP_OK)
                return 15;
            if (hp_device_synchronize() != HP_OK || hp_memcpy_d2h(got.data(), db, got.size()) != HP_OK)
                return 16;
            hp_free(db);
            if (got != bgr)
                return 17;
            ++compared;
        }
        if (pass == 0)
            (void)engine.inference(frames); // the engine's buffers move on; `maps` keeps its host copy
    }
    try {
        hp::map_view bad;
        bad.opacity = 0.f;
        hp::draw_maps(frames[0], maps[0][0], cover, bad);
    } catch (const std::logic_error&) {
        ++threw;
    }
    std::printf("OK %d %d\n", compared, threw);
    return threw == 1 ? 0 : 4;
}
