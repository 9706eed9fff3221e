// Host-only check of csrc/weight_pack.hpp: every layout gets a source of distinct non-zero values; each source element must sit at the index
// the layout's DEFINITION gives - written out here as tile / k-step / lane / element, never by calling the function under test - and every
// other element of the buffer must be zero (the non-zero count equals the source count).  Shapes cross each boundary: 24 -> 32 and 40 -> 48 / 64
// input channels, 33 and 72 outputs (a 32-row tile, the 64 / 128 pads), 1 and 9 taps, k on both sides of 8 and 16.
#include "../../hyperpose_amd/csrc/weight_pack.hpp"

#include <cstdio>
#include <cstring>

namespace wp = hp::wpack;

static int g_checks = 0, g_fail = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            if (++g_fail <= 20) {                                \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                        \
                std::printf("\n");                               \
            }                                                    \
        }                                                        \
    } while (0)

static int round_up(int a, int b) { return (a + b - 1) / b * b; }

// distinct non-zero floats; the fp16 form is exact in half precision and distinct for the first 48 912 indices: an odd integer below 2048
// (so no two of them differ by a power of two), a sign, and one of 24 powers of two that keep it a normal number
static float val32(size_t i) { return (float)(i + 1); }
static float val16(size_t i) { return (float)(2 * (i % 1019) + 1) * ((i / 1019) % 2 ? -1.f : 1.f) / (float)(1 << ((i / 2038) % 24)); }
static std::vector<float> source(size_t n, float (*val)(size_t))
{
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i)
        v[i] = val(i);
    return v;
}
static unsigned short bits(__half h)
{
    unsigned short u;
    std::memcpy(&u, &h, 2);
    return u;
}
static bool same(__half a, float want) { return bits(a) == bits(__float2half(want)) && __half2float(a) == want; }
template <typename T>
static size_t nonzero(const std::vector<T>& v)
{
    size_t n = 0;
    const T zero{};
    for (const T& x : v)
        n += std::memcmp(&x, &zero, sizeof(T)) != 0;
    return n;
}
// the fp16 MFMA fragment order: [32-row tile][16-wide k step][64 lanes][8 elements]
static size_t frag_at(size_t tile, size_t kstep, size_t lane, size_t elem, size_t ksteps) { return ((tile * ksteps + kstep) * 64 + lane) * 8 + elem; }

static void test_padded()
{
    const std::vector<float> src = source(33, val32);
    const std::vector<float> v = wp::padded(src.data(), 33, 64), z = wp::padded(nullptr, 33, 64);
    CHECK(v.size() == 64 && z.size() == 64 && nonzero(v) == 33 && nonzero(z) == 0, "padded: sizes / counts");
    for (int i = 0; i < 33; ++i)
        CHECK(v[i] == src[i], "padded: element %d", i);
}

static void test_depthwise(int C)
{
    const std::vector<float> w = source((size_t)C * 9, val16), bias = source(C, val32);
    const std::vector<float> p32 = wp::dw_taps32(w.data(), C), pb = wp::dw_taps32_bias(w.data(), bias.data(), C);
    const std::vector<__half> p16 = wp::dw_taps16(w.data(), C);
    CHECK(p32.size() == (size_t)9 * C && p16.size() == (size_t)9 * C && pb.size() == (size_t)10 * C, "depthwise %d: sizes", C);
    CHECK(nonzero(p32) == w.size() && nonzero(p16) == w.size() && nonzero(pb) == w.size() + C, "depthwise %d: counts", C);
    for (int c = 0; c < C; ++c) {
        for (int t = 0; t < 9; ++t) {
            const float x = w[(size_t)c * 9 + t];
            CHECK(p32[(size_t)t * C + c] == x && pb[(size_t)t * C + c] == x && same(p16[(size_t)t * C + c], x), "depthwise %d: channel %d tap %d", C, c, t);
        }
        CHECK(pb[(size_t)9 * C + c] == bias[c], "depthwise %d: bias %d is not row 9", C, c);
    }
}

static void test_dense32(int cout, int taps, int cin)
{
    const int cin_pad = round_up(cin, 16), cout_pad = round_up(cout, 64), cin_s = round_up(cin, taps == 1 ? 64 : 32);
    const std::vector<float> w = source((size_t)cout * taps * cin, val32);
    const std::vector<float> rows = wp::dense32_rows(w.data(), cout, taps, cin, cout_pad, cin_pad);
    const std::vector<float> wide = wp::restride32(rows, taps, cout_pad, cin_pad, cin_s);
    CHECK(rows.size() == (size_t)taps * cout_pad * cin_pad && wide.size() == (size_t)taps * cout_pad * cin_s, "dense32 %d/%d/%d: sizes", cout, taps, cin);
    CHECK(nonzero(rows) == w.size() && nonzero(wide) == w.size(), "dense32 %d/%d/%d: counts", cout, taps, cin);
    for (int co = 0; co < cout; ++co)
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < cin; ++ci) {
                const float x = w[((size_t)co * taps + t) * cin + ci];
                CHECK(rows[((size_t)t * cout_pad + co) * cin_pad + ci] == x, "dense32 rows: out %d tap %d in %d", co, t, ci);
                CHECK(wide[((size_t)t * cout_pad + co) * cin_s + ci] == x, "dense32 wide: out %d tap %d in %d", co, t, ci);
            }
}

static void test_dense16(int cout, int taps, int cin, int cout_pad, int cin_pad)
{
    const std::vector<float> w = source((size_t)cout * taps * cin, val16);
    const std::vector<__half> rows = wp::dense16(w.data(), cout, taps, cin, cout_pad, cin_pad, 0), frag = wp::dense16(w.data(), cout, taps, cin, cout_pad, cin_pad, 1);
    const size_t total = (size_t)taps * cout_pad * cin_pad, ksteps = cin_pad / 16, tiles_per_tap = cout_pad / 32;
    CHECK(rows.size() == total && frag.size() == total, "dense16 %d/%d/%d: sizes", cout, taps, cin);
    CHECK(nonzero(rows) == w.size() && nonzero(frag) == w.size(), "dense16 %d/%d/%d: counts %zu %zu of %zu", cout, taps, cin, nonzero(rows), nonzero(frag), w.size());
    for (int co = 0; co < cout; ++co)
        for (int t = 0; t < taps; ++t)
            for (int k = 0; k < cin; ++k) {
                const float x = w[((size_t)co * taps + t) * cin + k];
                CHECK(same(rows[((size_t)t * cout_pad + co) * cin_pad + k], x), "dense16 rows: out %d tap %d in %d", co, t, k);
                const size_t tile = t * tiles_per_tap + co / 32, kstep = k / 16, lane = (size_t)(k % 16 >= 8 ? 32 : 0) + co % 32, elem = k % 8;
                CHECK(same(frag[frag_at(tile, kstep, lane, elem, ksteps)], x), "dense16 fragments: out %d tap %d in %d", co, t, k);
            }
    CHECK(wp::frag16(cout - 1, cin - 1, ksteps, 3) == frag_at(3 + (cout - 1) / 32, (cin - 1) / 16, ((cin - 1) % 16 / 8) * 32 + (cout - 1) % 32, (cin - 1) % 8, ksteps), "frag16 itself");
}

// head_params::w2: the hidden channel c = 128 w + 32 i + 8 a + 4 h + b (a < 4, h < 2, b < 4) sits at K-step 8 w + 2 i + a / 2, in lane half h,
// at element 4 (a % 2) + b; rows padded to 64 (two 32-row tiles of 32 K-steps each)
static void test_head_w2(int cout2)
{
    const int HID = 512;
    const std::vector<float> w = source((size_t)cout2 * HID, val16);
    const std::vector<__half> p = wp::head_w2(w.data(), cout2, HID);
    CHECK(p.size() == (size_t)64 * HID && nonzero(p) == w.size(), "head w2 %d: size / count", cout2);
    for (int m = 0; m < cout2; ++m)
        for (int wv = 0; wv < HID / 128; ++wv)
            for (int i = 0; i < 4; ++i)
                for (int a = 0; a < 4; ++a)
                    for (int h = 0; h < 2; ++h)
                        for (int b = 0; b < 4; ++b) {
                            const int c = 128 * wv + 32 * i + 8 * a + 4 * h + b;
                            const size_t tile = m / 32, kstep = 8 * wv + 2 * i + a / 2, lane = 32 * h + m % 32, elem = 4 * (a % 2) + b;
                            CHECK(same(p[frag_at(tile, kstep, lane, elem, 32)], w[(size_t)m * HID + c]), "head w2 %d: row %d hidden %d", cout2, m, c);
                        }
}

// first_conv_f16_kernel: k' = ky * ROWP + kx * 3 + c with ROWP = the 3 KS row elements rounded up to 8, in 16-wide steps
static void test_first_conv(int KS, int cout, int rowp, int steps)
{
    const std::vector<float> w = source((size_t)cout * KS * KS * 3, val16);
    const std::vector<__half> p = wp::first_conv_frag16(w.data(), cout, KS);
    CHECK(p.size() == (size_t)(cout <= 32 ? 1 : 2) * steps * 64 * 8 && nonzero(p) == w.size(), "first conv %d x %d / %d: size / count", KS, KS, cout);
    for (int co = 0; co < cout; ++co)
        for (int ky = 0; ky < KS; ++ky)
            for (int kx = 0; kx < KS; ++kx)
                for (int c = 0; c < 3; ++c) {
                    const int k = ky * rowp + kx * 3 + c;
                    const size_t lane = (size_t)(k % 16 >= 8 ? 32 : 0) + co % 32;
                    CHECK(same(p[frag_at(co / 32, k / 16, lane, k % 8, steps)], w[(((size_t)co * KS + ky) * KS + kx) * 3 + c]), "first conv %d: out %d ky %d kx %d c %d", KS, co, ky, kx, c);
                }
}

static void test_int8_values()
{
    // 4 channels x 1 tap x 8 inputs.  0: all zero (scale 1).  1: extreme -127 -> scale 1, ties at +-0.5 / +-1.5 / 2.5 quanta.
    // 2: extreme +254 -> scale 2, the same ties at twice the size.  3: extreme -1e-3, every value a multiple of the quantum
    const float w[4][8] = { { 0, 0, 0, 0, 0, 0, 0, 0 }, { -127.f, 0.5f, -0.5f, 1.5f, -1.5f, 2.5f, 126.5f, -126.5f },
        { 254.f, 1.f, -1.f, 3.f, -3.f, 5.f, -253.f, 253.f }, { -1e-3f, 1e-3f, 0.f, 5e-4f, 0, 0, 0, 0 } };
    const int want[4][8] = { { 0, 0, 0, 0, 0, 0, 0, 0 }, { -127, 0, 0, 2, -2, 2, 126, -126 }, { 127, 0, 0, 2, -2, 2, -126, 126 }, { -127, 127, 0, 0, 0, 0, 0, 0 } };
    const wp::i8_rows r = wp::quantize_rows(&w[0][0], 4, 1, 8, 64, 32);
    CHECK(r.s_w.size() == 4 && r.s_w[0] == 1.f && r.s_w[1] == 1.f && r.s_w[2] == 2.f && r.s_w[3] == 1e-3f / 127.f, "int8 scales %g %g %g %g", r.s_w[0], r.s_w[1], r.s_w[2], r.s_w[3]);
    CHECK(r.q.size() == (size_t)64 * 32, "int8 rows: size");
    size_t expect_nonzero = 0;
    for (int c = 0; c < 4; ++c)
        for (int k = 0; k < 8; ++k) {
            if (c == 3 && k == 3) { // 63.5 quanta up to the rounding of the scale: 63 or 64, nothing else
                CHECK(r.q[c * 32 + k] == 63 || r.q[c * 32 + k] == 64, "int8 value: channel 3 input 3 = %d", r.q[c * 32 + k]);
                ++expect_nonzero;
                continue;
            }
            CHECK(r.q[c * 32 + k] == want[c][k], "int8 value: channel %d input %d = %d, want %d", c, k, r.q[c * 32 + k], want[c][k]);
            expect_nonzero += want[c][k] != 0;
        }
    CHECK(nonzero(r.q) == expect_nonzero, "int8 rows: padding not zero");
}

static void test_int8_rows(int cout, int taps, int cin, int cout_pad, int cin_pad)
{
    std::vector<float> w((size_t)cout * taps * cin);
    for (size_t i = 0; i < w.size(); ++i) // (every value at least 1 / 52 of its channel's extreme: no weight rounds to zero)
        w[i] = ((i / 2039) % 2 ? -1.f : 1.f) * (40.f + (float)(i % 2039));
    const wp::i8_rows r = wp::quantize_rows(w.data(), cout, taps, cin, cout_pad, cin_pad);
    CHECK(r.q.size() == (size_t)taps * cout_pad * cin_pad && nonzero(r.q) == w.size(), "int8 rows %d/%d/%d: size / count", cout, taps, cin);
    for (int co = 0; co < cout; ++co) {
        float m = 0.f;
        for (int k = 0; k < taps * cin; ++k)
            m = std::max(m, std::fabs(w[(size_t)co * taps * cin + k]));
        CHECK(r.s_w[co] == m / 127.f, "int8 rows: scale of channel %d", co);
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < cin; ++ci) {
                const float x = w[((size_t)co * taps + t) * cin + ci] / (m / 127.f);
                const int q = r.q[((size_t)t * cout_pad + co) * cin_pad + ci];
                CHECK(q >= -127 && q <= 127 && std::fabs((float)q - x) <= 0.5f, "int8 rows: out %d tap %d in %d: %d for %g quanta", co, t, ci, q, x);
            }
    }
    // conv_i8_direct_kernel's order: [tap][64-channel chunk][32-channel half][32-row tile][lane = 16-channel quarter * 32 + row][16 bytes]
    std::vector<int8_t> all(r.q.size());
    for (size_t i = 0; i < all.size(); ++i)
        all[i] = (int8_t)((int)(i % 251) - 125 >= 0 ? (int)(i % 251) - 124 : (int)(i % 251) - 125); // non-zero, period 251
    if (cin_pad % 64 == 0) {
        const std::vector<int8_t> d = wp::i8_direct(all, taps, cout_pad, cin_pad);
        CHECK(d.size() == all.size() && nonzero(d) == all.size(), "int8 direct %d/%d/%d: size / count", cout, taps, cin);
        for (int t = 0; t < taps; ++t)
            for (int m = 0; m < cout_pad; ++m)
                for (int c = 0; c < cin_pad; ++c) {
                    const size_t chunk = c / 64, half = c % 64 / 32, tile = m / 32, lane = (size_t)(c % 32 / 16) * 32 + m % 32, byte = c % 16;
                    const size_t at = (((((size_t)t * (cin_pad / 64) + chunk) * 2 + half) * (cout_pad / 32) + tile) * 64 + lane) * 16 + byte;
                    CHECK(d[at] == all[((size_t)t * cout_pad + m) * cin_pad + c], "int8 direct: tap %d row %d channel %d", t, m, c);
                }
    }
}

int main()
{
    test_padded();
    test_depthwise(24);
    test_depthwise(40);
    test_dense32(33, 1, 24); // 24 -> 32 (-> 64 for the direct kernel), 33 -> 64 rows
    test_dense32(72, 9, 40); // 40 -> 48 (-> 64), 72 -> 128 rows
    test_dense16(33, 1, 24, 64, 32);
    test_dense16(72, 9, 40, 128, 48);
    test_dense16(72, 9, 40, 128, 64);   // as the fp16 engine pads 40 input channels
    test_dense16(33, 1, 32, 128, 32);   // a separable block's pointwise half: [rows][K], one tap
    test_dense16(512, 1, 64, 512, 64);  // a head's first layer
    test_head_w2(19);
    test_head_w2(38);
    test_first_conv(3, 32, 16, 3);   // 9 -> 16 per kernel row, 48 = 3 steps
    test_first_conv(7, 64, 24, 11);  // 21 -> 24 per kernel row, 168 -> 11 steps, two 32-row tiles
    test_int8_values();
    test_int8_rows(33, 1, 24, 64, 32);
    test_int8_rows(72, 9, 40, 128, 64);
    if (g_fail) {
        std::printf("FAILED %d of %d checks\n", g_fail, g_checks);
        return 1;
    }
    std::printf("OK %d\n", g_checks);
    return 0;
}
