// rgb_formats.cpp — hyperpose_amd/csrc/rgb_formats.hpp as a stand-alone host program (plain C++, no HIP): the layout table against the rule as the
// header of the library states it ("memory order is as the name reads"), to_bgr on frames allocated with no slack - under -fsanitize=address a read
// outside width * pixel_bytes of a row or a write outside width * 3 of an output row aborts - and every refusal of check(), whose message must name
// the layout and the offending quantity.  Prints "OK <cases>".
#include "../../hyperpose_amd/csrc/rgb_formats.hpp"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int cases = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++cases;                                                          \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            return 1;                                                     \
        }                                                                 \
    } while (0)

// the channels of a pixel in memory order, read off the names; X: ignored, Y: grey
static const char* const ORDER[7] = { "BGR", "RGB", "BGRX", "RGBX", "XRGB", "XBGR", "Y" };
static const char* const NAME[7] = { "HP_RGB_BGR24", "HP_RGB_RGB24", "HP_RGB_BGRA32", "HP_RGB_RGBA32", "HP_RGB_ARGB32", "HP_RGB_ABGR32", "HP_RGB_GRAY8" };

static bool refused(const hp_rgb_image* im, bool kernel, const char* a, const char* b)
{
    char msg[256] = "";
    if (hp_rgb::check(im, "who", kernel, msg, sizeof msg) == 0)
        return false;
    return strncmp(msg, "who: ", 5) == 0 && strstr(msg, a) && strstr(msg, b);
}

int main()
{
    EXPECT(HP_RGB_BGR24 == 0 && HP_RGB_RGB24 == 1 && HP_RGB_BGRA32 == 2 && HP_RGB_RGBA32 == 3 && HP_RGB_ARGB32 == 4 && HP_RGB_ABGR32 == 5 && HP_RGB_GRAY8 == 6);
    EXPECT(!hp_rgb::layout_of(-1) && !hp_rgb::layout_of(7) && !hp_rgb::layout_of(9));
    EXPECT(hp_rgb::packed_bytes(7, 4, 4) == 0 && hp_rgb::packed_bytes(-1, 4, 4) == 0);
    unsigned seed = 12345;
    auto rnd = [&] { return (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24); };
    for (int f = 0; f < 7; ++f) {
        const hp_rgb::layout* l = hp_rgb::layout_of(f);
        EXPECT(l && strcmp(l->name, NAME[f]) == 0);
        const std::string o = ORDER[f];
        const int pb = (int)o.size();
        EXPECT(l->pixel_bytes == pb);
        if (o == "Y")
            EXPECT(l->b == 0 && l->g == 0 && l->r == 0);
        else
            EXPECT(l->b == (int)o.find('B') && l->g == (int)o.find('G') && l->r == (int)o.find('R'));
        EXPECT(hp_rgb::packed_bytes(f, 0, 3) == 0 && hp_rgb::packed_bytes(f, 3, -1) == 0 && hp_rgb::packed_bytes(f, 1920, 1080) == (size_t)1920 * 1080 * pb);

        const int sizes[3][2] = { { 1, 1 }, { 5, 3 }, { 97, 65 } };
        for (const auto& wh : sizes) {
            const int w = wh[0], h = wh[1];
            for (int pad = 0; pad < 2; ++pad) {
                // the last row ends where its pixels end: no slack behind the frame, and none behind the output
                const int stride = w * pb + (pad ? 5 : 0), ostride = w * 3 + (pad ? 7 : 0);
                std::vector<uint8_t> src((size_t)stride * (h - 1) + (size_t)w * pb), out((size_t)ostride * (h - 1) + (size_t)w * 3, 0x3C);
                for (auto& v : src)
                    v = rnd();
                const hp_rgb_image im{ f, w, h, src.data(), stride };
                char msg[256];
                EXPECT(hp_rgb::check(&im, "who", false, msg, sizeof msg) == 0);
                hp_rgb::to_bgr(im, out.data(), ostride);
                bool same = true, untouched = true;
                for (int y = 0; y < h; ++y) {
                    for (int x = 0; x < w; ++x) {
                        const uint8_t* s = &src[(size_t)y * stride + (size_t)x * pb];
                        const uint8_t* d = &out[(size_t)y * ostride + (size_t)x * 3];
                        for (int c = 0; c < 3; ++c)
                            same = same && d[c] == (o == "Y" ? s[0] : s[o.find("BGR"[c])]);
                    }
                    for (int k = w * 3; k < ostride && y + 1 < h; ++k)
                        untouched = untouched && out[(size_t)y * ostride + k] == 0x3C;
                }
                EXPECT(same);
                EXPECT(untouched);
            }
        }

        // refusals: the layout's name and the offending quantity
        alignas(4) static uint8_t buf[64 * 8];
        const hp_rgb_image ok{ f, 6, 4, buf, 32 };
        EXPECT(!refused(&ok, true, "", ""));
        hp_rgb_image im = ok;
        im.width = 0;
        EXPECT(refused(&im, false, NAME[f], "0 x 4"));
        im = ok, im.height = -3;
        EXPECT(refused(&im, false, NAME[f], "6 x -3"));
        im = ok, im.data = nullptr;
        EXPECT(refused(&im, false, NAME[f], "null"));
        im = ok, im.stride = 6 * pb - 1;
        EXPECT(refused(&im, false, NAME[f], ("stride " + std::to_string(6 * pb - 1)).c_str()));
        im = ok, im.stride = 6 * pb; // tight is fine
        EXPECT(!refused(&im, true, "", ""));
        // the alignment rule: 4-byte layouts, and only where a kernel reads the plane
        im = ok, im.stride = 30;
        EXPECT(refused(&im, true, NAME[f], "stride 30") == (pb == 4));
        EXPECT(!refused(&im, false, "", ""));
        for (int mis = 1; mis < 4; ++mis) {
            im = ok, im.data = buf + mis;
            EXPECT(refused(&im, true, NAME[f], ("address % 4 = " + std::to_string(mis)).c_str()) == (pb == 4));
            EXPECT(!refused(&im, false, "", ""));
        }
    }
    const hp_rgb_image bad{ 9, 6, 4, &seed, 32 };
    EXPECT(refused(&bad, false, "unknown format 9", "HP_RGB_GRAY8"));
    EXPECT(refused(nullptr, false, "null image", ""));
    printf("OK %d\n", cases);
    return 0;
}
