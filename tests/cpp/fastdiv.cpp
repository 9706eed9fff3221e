// fastdiv.hpp on the host: quotient and remainder against `/` and `%` over the header's stated range (1 <= d < 2^31, 0 <= n < 2^31), and the
// kernels' pixel decomposition against the carry loop it replaced.  No library, no device code.
//
// Divisors: everything an fp32 engine of the five BASELINE networks divides by - their inputs are 368 x 432 (configs[0], [1]), 432 x 768 ([2]),
// 384 x 384 ([3]) and 385 x 385 ([4]); a map is the input halved k = 0 .. 6 times, rounded up (SAME) or down (VALID) - so for every such (OH, OW):
// OW, OH, OH * OW, the depthwise kernel's row segments ceil(OH / run) and column-pair slots at dilation 1 and 2, and the channel groups C / 4 of
// every width a layer there has; then the issue's list 1, 2, 3, 7, 16, 17, 54, 2 484, 2^16 - 1, 2^16 + 1 and the range's ends.
#include "../../hyperpose_amd/csrc/fastdiv.hpp"

#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

using hp::fastdiv;

static long checks = 0, failures = 0;

static void check(uint32_t n, const fastdiv& f)
{
    uint32_t q, r;
    hp::fd_divmod(n, f, q, r);
    ++checks;
    if (q != n / f.d || r != n % f.d || hp::fd_div(n, f) != q) {
        if (failures++ < 10)
            std::printf("FAIL %u / %u: got %u rem %u, want %u rem %u\n", n, f.d, q, r, n / f.d, n % f.d);
    }
}

static void sweep(uint32_t d)
{
    const fastdiv f = hp::make_fastdiv(d);
    if (f.d != d || !hp::fastdiv_is(f, d)) {
        std::printf("FAIL make_fastdiv(%u)\n", d);
        ++failures;
        return;
    }
    const uint32_t top = 0x7fffffffu; // the last numerator of the range
    for (uint32_t n = 0; n < (1u << 24); ++n)
        check(n, f);
    for (uint32_t n = 1u << 24; n <= top - 9973; n += 9973) // a stride (a prime) through the rest ..
        check(n, f);
    for (uint32_t k = 0; k < 4096; ++k) // .. and the range's end
        check(top - k, f);
    // around every multiple of d near the end, and the multiples of d around 2^24, 2^30
    for (uint64_t base : { uint64_t(1) << 24, uint64_t(1) << 30, uint64_t(top) }) {
        const uint64_t m = base / d * d;
        for (int64_t k = -2; k <= 2; ++k) {
            const int64_t n = (int64_t)m + k * (int64_t)d;
            for (int64_t e = -1; e <= 1; ++e)
                if (n + e >= 0 && n + e <= (int64_t)top)
                    check((uint32_t)(n + e), f);
        }
    }
}

// the kernels' epilogues: pixel n + add of a B x OH x OW map from fd_pixel / fd_view_pixel against the carry loop from pixel n's coordinates
static void carries()
{
    for (int OW = 1; OW <= 40; ++OW)
        for (int OH : { 1, 2, 3, 7, 16, 17 }) {
            const fastdiv fow = hp::make_fastdiv(OW), fohw = hp::make_fastdiv((long)OH * OW);
            const int B = 5, npix = B * OH * OW, wp = OW + 4, img = (OH + 4) * wp + 3; // a view with a halo
            for (int n = 0; n < npix; ++n) {
                int b = n / (OH * OW), oy = (n - b * OH * OW) / OW, ox = n - b * OH * OW - oy * OW;
                for (int add = 0; add <= 160; add += 16) { // a t16 wavefront's tiles are 16 pixels apart; 64 x 64 rows 1 .. 32
                    if (add) {
                        ox += 16;
                        while (ox >= OW) {
                            ox -= OW;
                            if (++oy == OH)
                                oy = 0, ++b;
                        }
                    }
                    int fb, foy, frem;
                    hp::fd_pixel(n + add, fohw, fow, fb, foy, frem);
                    const long want = (long)b * img + (long)oy * wp + ox, got = hp::fd_view_pixel(n + add, fb, foy, fohw, fow, img, wp);
                    ++checks;
                    if (fb != b || foy != oy || frem != oy * OW + ox || got != want) {
                        if (failures++ < 10)
                            std::printf("FAIL carry OW %d OH %d n %d + %d: (%d, %d, %d) -> %ld, want (%d, %d, %d) -> %ld\n", OW, OH, n, add, fb, foy, frem - foy * OW, got, b, oy, ox, want);
                    }
                }
            }
        }
}

int main()
{
    std::set<uint32_t> ds = { 1, 2, 3, 7, 16, 17, 54, 2484, 65535, 65537, 0x7ffffffeu, 0x7fffffffu, 1u << 30, (1u << 30) + 1 };
    const int inputs[][2] = { { 368, 432 }, { 432, 768 }, { 384, 384 }, { 385, 385 } };
    for (const auto& in : inputs)
        for (int k = 0; k <= 6; ++k)
            for (int up = 0; up < 2; ++up) {
                const int OH = std::max(1, up ? (in[0] + (1 << k) - 1) >> k : in[0] >> k), OW = std::max(1, up ? (in[1] + (1 << k) - 1) >> k : in[1] >> k);
                ds.insert(OW), ds.insert(OH), ds.insert((uint32_t)OH * OW);
                const int run = OH >= 32 ? 8 : 4;
                ds.insert((OH + run - 1) / run);
                for (int dil : { 1, 2 })
                    ds.insert((OW + 2 * dil - 1) / (2 * dil) * dil);
            }
    for (int c : { 3, 8, 16, 19, 24, 32, 38, 48, 64, 96, 128, 144, 160, 192, 256, 320, 384, 512, 576, 960, 1024, 1280, 2048 })
        ds.insert(std::max(1, c / 4));
    if (hp::make_fastdiv(0).d != 0 || hp::make_fastdiv(1L << 31).d != 0 || hp::fastdiv_is(fastdiv{ 0, 0, 0 }, 0) || hp::fastdiv_is(hp::make_fastdiv(54), 46)) {
        std::printf("FAIL divisors outside the range / a stale constant must be refused\n");
        ++failures;
    }
    for (uint32_t d : ds)
        sweep(d);
    carries();
    std::printf("%zu divisors\n%s %ld\n", ds.size(), failures ? "FAILED" : "OK", checks);
    return failures ? 1 : 0;
}
