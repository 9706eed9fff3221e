// to_yuv_rules.cpp — the host side of hyperpose_amd/csrc/to_yuv.hpp (coefficients, pixel and chroma rules, padding, the host twin) as a stand-alone
// host program (plain C++, no HIP), built with -fsanitize=address,undefined by tests/test_cpp_to_yuv.py: every source and every plane is a heap block
// of exactly the bytes the call may touch - a source of height * stride - (stride - width * pixel bytes) bytes, planes of rows * stride - (stride -
// row bytes) - so a read outside width * pixel bytes of a row, a write outside a plane's samples or an overflow in the integer rules aborts.  The
// samples are checked against a per-pixel restatement that goes through the float64 coefficients itself, and the bytes between the rows must keep
// their fill.  Prints "OK <cases>".
#include "../../hyperpose_amd/csrc/to_yuv.hpp"

#include <cstdio>
#include <cstring>
#include <memory>
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

static int channel(const uint8_t* p, int format, char c)
{
    const char* o = ORDER[format];
    if (o[0] == 'Y')
        return p[0];
    return p[strchr(o, c) - o];
}

struct block { // a heap block of exactly n bytes
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit block(size_t n_, uint8_t fill) : p(new uint8_t[n_]), n(n_) { memset(p.get(), fill, n_); }
};

// one sample's code value where the layouts' names put it (restated: NV12 / NV16 / P010 hold (U, V) pairs, YUY2 is Y0 U Y1 V, UYVY is U Y0 V Y1)
static int sample_at(const hp_yuv_image& im, int which /* 0 Y, 1 U, 2 V */, int x, int y)
{
    const int f = im.format;
    const bool semi = f == HP_YUV_NV12 || f == HP_YUV_P010 || f == HP_YUV_NV16, packed = f == HP_YUV_YUY2 || f == HP_YUV_UYVY;
    const bool wide = f == HP_YUV_P010 || f == HP_YUV_I010;
    const int sx = f == HP_YUV_I444 ? 0 : 1, sy = (f == HP_YUV_NV12 || f == HP_YUV_I420 || f == HP_YUV_P010 || f == HP_YUV_I010) ? 1 : 0;
    const int sb = wide ? 2 : 1;
    const uint8_t* q;
    if (packed) {
        const uint8_t* row = (const uint8_t*)im.plane[0] + (size_t)y * im.stride[0];
        const int luma0 = f == HP_YUV_YUY2 ? 0 : 1;
        q = which == 0 ? row + 2 * x + luma0 : row + 4 * (x >> 1) + (1 - luma0) + (which == 2 ? 2 : 0);
    } else if (which == 0)
        q = (const uint8_t*)im.plane[0] + (size_t)y * im.stride[0] + (size_t)x * sb;
    else if (semi)
        q = (const uint8_t*)im.plane[1] + (size_t)(y >> sy) * im.stride[1] + (size_t)(x >> sx) * 2 * sb + (which == 2 ? sb : 0);
    else
        q = (const uint8_t*)im.plane[which] + (size_t)(y >> sy) * im.stride[which] + (size_t)(x >> sx) * sb;
    if (!wide)
        return q[0];
    const int word = q[0] | (q[1] << 8);
    if (f == HP_YUV_P010)
        return (word & 63) ? -1 : word >> 6; // the low six bits are stored as zero
    return (word & ~1023) ? -1 : word;
}

int main()
{
    // the table the issue of this unit quotes
    {
        int32_t k[11];
        hp_enc::forward_coefficients(HP_YUV_BT601, HP_YUV_LIMITED, 8, k);
        const int32_t want[11] = { 16, 128, 67315, 132155, 25665, -38856, -76282, 115138, 115138, -96414, -18724 };
        EXPECT(memcmp(k, want, sizeof want) == 0);
    }
    // padded sizes
    {
        int w = 0, h = 0;
        hp_enc::padded_size(*hp_yuv::layout_of(HP_YUV_NV12), 1920, 1080, 16, &w, &h);
        EXPECT(w == 1920 && h == 1088);
        hp_enc::padded_size(*hp_yuv::layout_of(HP_YUV_I444), 3, 5, 1, &w, &h);
        EXPECT(w == 3 && h == 5);
        hp_enc::padded_size(*hp_yuv::layout_of(HP_YUV_YUY2), 3, 5, 3, &w, &h);
        EXPECT(w == 6 && h == 6);
        hp_enc::padded_size(*hp_yuv::layout_of(HP_YUV_I420), 8191, 8191, 256, &w, &h);
        EXPECT(w == 8192 && h == 8192);
    }
    unsigned seed = 2024;
    auto rnd = [&] { return (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24); };
    const int sizes[][4] = { { 1, 1, 0, 0 }, { 2, 2, 2, 2 }, { 3, 5, 4, 6 }, { 31, 3, 32, 4 }, { 30, 20, 32, 32 } };
    for (int yf = HP_YUV_NV12; yf <= HP_YUV_I444; ++yf)
        for (int rf = HP_RGB_BGR24; rf <= HP_RGB_GRAY8; ++rf)
            for (const auto& sz : sizes) {
                const hp_yuv::layout& l = *hp_yuv::layout_of(yf);
                const hp_rgb::layout& in = *hp_rgb::layout_of(rf);
                const int matrix = (yf + rf) % 3, range = (yf + rf / 3) % 2, depth = l.sample_bytes == 2 ? 10 : 8, top = (1 << depth) - 1;
                hp_rgb_image src;
                src.format = rf, src.width = sz[0], src.height = sz[1], src.stride = sz[0] * in.pixel_bytes + 5;
                block sbuf((size_t)src.height * src.stride - 5, 0);
                for (size_t i = 0; i < sbuf.n; ++i)
                    sbuf.p[i] = rnd();
                if (sz[0] >= 3) // extremes in the first row
                    memset(sbuf.p.get(), 255, (size_t)in.pixel_bytes), memset(sbuf.p.get() + in.pixel_bytes, 0, (size_t)in.pixel_bytes);
                src.data = sbuf.p.get();
                hp_yuv_image dst;
                memset(&dst, 0, sizeof dst);
                dst.format = yf, dst.matrix = matrix, dst.range = range, dst.width = sz[2], dst.height = sz[3];
                if (!sz[2])
                    hp_enc::padded_size(l, 1, 1, 1, &dst.width, &dst.height);
                EXPECT(hp_yuv::size_ok(l, dst.width, dst.height));
                std::vector<block> planes;
                for (int k = 0; k < l.planes; ++k) {
                    const size_t row = hp_yuv::row_bytes(l, k, dst.width);
                    dst.stride[k] = (int)row + 3 + k; // odd and even pitches: host planes follow no alignment rule
                    planes.emplace_back((size_t)hp_yuv::rows(l, k, dst.height) * dst.stride[k] - (3 + k), 0xA5);
                    dst.plane[k] = planes.back().p.get();
                }
                char msg[256] = "";
                EXPECT(hp_enc::check_sizes(src, dst, "who", msg, sizeof msg) == 0);
                hp_enc::convert_host(src, dst);
                // every sample against the restatement; double arithmetic on the rounded coefficients is exact (all values are below 2^53)
                int32_t k11[11];
                hp_enc::forward_coefficients(matrix, range, depth, k11);
                EXPECT(k11[5] + k11[6] + k11[7] == 0 && k11[8] + k11[9] + k11[10] == 0);
                bool same = true;
                const int px = 1 << l.sx, py = 1 << l.sy, n = px * py;
                for (int by = 0; by < dst.height / py && same; ++by)
                    for (int bx = 0; bx < dst.width / px && same; ++bx) {
                        long long rs = 0, gs = 0, bs = 0;
                        for (int dy = 0; dy < py; ++dy)
                            for (int dx = 0; dx < px; ++dx) {
                                const int x = bx * px + dx, y = by * py + dy;
                                const uint8_t* p = sbuf.p.get() + (size_t)std::min(y, src.height - 1) * src.stride + (size_t)std::min(x, src.width - 1) * in.pixel_bytes;
                                const long long r = channel(p, rf, 'R'), g = channel(p, rf, 'G'), b = channel(p, rf, 'B');
                                rs += r, gs += g, bs += b;
                                long long yv = (k11[2] * r + k11[3] * g + k11[4] * b + ((long long)k11[0] << 18) + (1 << 17)) >> 18;
                                yv = std::min<long long>(top, std::max<long long>(0, yv));
                                same = same && sample_at(dst, 0, x, y) == (int)yv;
                            }
                        for (int c = 0; c < 2; ++c) {
                            const int32_t* row = k11 + 5 + 3 * c;
                            long long v = (row[0] * rs + row[1] * gs + row[2] * bs + n * (((long long)k11[1] << 18) + (1 << 17))) / ((long long)n << 18);
                            v = std::min<long long>(top, std::max<long long>(0, v)); // (the numerator is non-negative: the division floors)
                            same = same && sample_at(dst, 1 + c, bx * px, by * py) == (int)v;
                        }
                    }
                EXPECT(same);
                // the bytes between the rows keep their fill
                bool kept = true;
                for (int k = 0; k < l.planes; ++k) {
                    const size_t row = hp_yuv::row_bytes(l, k, dst.width);
                    for (int y = 0; y + 1 < hp_yuv::rows(l, k, dst.height); ++y)
                        for (size_t i = row; i < (size_t)dst.stride[k]; ++i)
                            kept = kept && planes[k].p[(size_t)y * dst.stride[k] + i] == 0xA5;
                }
                EXPECT(kept);
            }
    // a grey frame has neutral chroma in every table
    for (int matrix = 0; matrix < 3; ++matrix)
        for (int range = 0; range < 2; ++range)
            for (int depth = 8; depth <= 10; depth += 2) {
                const hp_enc::table t = hp_enc::table_of(matrix, range, depth);
                bool neutral = true;
                for (int v = 0; v < 256; ++v)
                    for (int log2n = 0; log2n <= 2; ++log2n)
                        neutral = neutral && hp_enc::chroma(t.u, t.c_off, v << log2n, v << log2n, v << log2n, log2n, (1 << depth) - 1) == t.c_off
                            && hp_enc::chroma(t.v, t.c_off, v << log2n, v << log2n, v << log2n, log2n, (1 << depth) - 1) == t.c_off;
                EXPECT(neutral);
            }
    // the size rules, by message
    {
        hp_rgb_image src = { HP_RGB_BGRA32, 10, 6, nullptr, 40 };
        hp_yuv_image dst;
        memset(&dst, 0, sizeof dst);
        dst.format = HP_YUV_P010, dst.width = 8, dst.height = 6;
        char msg[256] = "";
        EXPECT(hp_enc::check_sizes(src, dst, "who", msg, sizeof msg) != 0 && strstr(msg, "who: HP_YUV_P010") && strstr(msg, "width 8") && strstr(msg, "HP_RGB_BGRA32"));
        dst.width = 10, dst.height = 4;
        EXPECT(hp_enc::check_sizes(src, dst, "who", msg, sizeof msg) != 0 && strstr(msg, "height 4") && strstr(msg, "HP_RGB_BGRA32"));
        dst.width = 8194, dst.height = 6;
        EXPECT(hp_enc::check_sizes(src, dst, "who", msg, sizeof msg) != 0 && strstr(msg, "8194 x 6") && strstr(msg, "8192"));
        dst.width = 10, dst.height = 6;
        EXPECT(hp_enc::check_sizes(src, dst, "who", msg, sizeof msg) == 0);
    }
    printf("OK %d\n", cases);
    return 0;
}
