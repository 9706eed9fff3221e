// hyperpose::redact_humans (include/hyperpose/utility/redact.hpp): a P010 BT.709 frame with padded pitch redacted in DEVICE memory and the same
// frame redacted in HOST memory give the same bytes, padding included, for heads pixelated and bodies blacked out; the device_bgr form equals the
// C ABI's host BGR twin on the library's region list; an odd cell throws.  Prints "OK <comparisons> <threw>"; run by tests/test_cpp_redact.py on
// the GPU box.
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
    const auto humans = some_humans(0.1f, 0.15f);
    int compared = 0, threw = 0;
    const int w = 200, h = 120, pitch = 26;
    hp::redaction heads, bodies;
    heads.margin = 0.5f;
    bodies.what = hp::redaction::body, bodies.effect = hp::redaction::black, bodies.cell = 6, bodies.margin = 0.25f;
    for (const hp::redaction& r : { heads, bodies }) {
        // P010, BT.709 limited range
        const int s0 = w * 2 + pitch, s1 = w * 2 + pitch;
        std::vector<uint8_t> p0 = noise((size_t)s0 * h, 1, true), p1 = noise((size_t)s1 * (h / 2), 2, true);
        const std::vector<uint8_t> before0 = p0;
        void *d0 = nullptr, *d1 = nullptr;
        if (hp_malloc(&d0, p0.size()) != HP_OK || hp_malloc(&d1, p1.size()) != HP_OK || hp_memcpy_h2d(d0, p0.data(), p0.size()) != HP_OK
            || hp_memcpy_h2d(d1, p1.data(), p1.size()) != HP_OK)
            return 10;
        hp::yuv_frame host;
        host.format = HP_YUV_P010, host.matrix = HP_YUV_BT709, host.range = HP_YUV_LIMITED, host.width = w, host.height = h;
        host.plane[0] = p0.data(), host.plane[1] = p1.data(), host.stride[0] = s0, host.stride[1] = s1;
        hp::yuv_frame dev = host;
        dev.plane[0] = d0, dev.plane[1] = d1, dev.on_device = true;
        hp::redact_humans(dev, humans, r);
        hp::redact_humans(host, humans, r);
        std::vector<uint8_t> g0(p0.size()), g1(p1.size());
        if (hp_device_synchronize() != HP_OK || hp_memcpy_d2h(g0.data(), d0, g0.size()) != HP_OK || hp_memcpy_d2h(g1.data(), d1, g1.size()) != HP_OK)
            return 11;
        hp_free(d0), hp_free(d1);
        if (g0 != p0 || g1 != p1)
            return 12;
        if (p0 == before0)
            return 13; // nothing was redacted
        size_t same = 0;
        for (size_t i = 0; i < p0.size(); ++i)
            same += p0[i] == before0[i];
        if (same < p0.size() / 4)
            return 18; // (nearly) everything was redacted
        ++compared;
        // 8-bit BGR in device memory against the host BGR twin of the C ABI
        const int sb = w * 3 + 7;
        std::vector<uint8_t> bgr = noise((size_t)sb * h, 3, false), got(bgr.size());
        void* db = nullptr;
        if (hp_malloc(&db, bgr.size()) != HP_OK || hp_memcpy_h2d(db, bgr.data(), bgr.size()) != HP_OK)
            return 14;
        hp::redact_humans(hp::device_bgr{ (uint8_t*)db, w, h, sb }, humans, r);
        const auto regions = hp::detail::redact_regions(humans, w, h, r);
        if (regions.empty() || hp_redact_u8c3_host(bgr.data(), w, h, sb, regions.data(), (int)regions.size(), r.effect, r.cell) != HP_OK)
            return 15;
        if (hp_device_synchronize() != HP_OK || hp_memcpy_d2h(got.data(), db, got.size()) != HP_OK)
            return 16;
        hp_free(db);
        if (got != bgr)
            return 17;
        ++compared;
    }
    std::vector<uint8_t> p((size_t)64 * 48 * 2);
    for (int what : { 0, 1 })
        try {
            hp::yuv_frame f = hp::yuv_frame::packed(HP_YUV_YUY2, p.data(), 64, 48);
            hp::redaction bad;
            if (what == 0)
                bad.cell = 15;
            else
                bad.margin = 0.f;
            hp::redact_humans(f, humans, bad);
        } catch (const std::logic_error&) {
            ++threw;
        }
    std::printf("OK %d %d\n", compared, threw);
    return threw == 2 ? 0 : 4;
}
