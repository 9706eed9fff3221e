// fastdiv.hpp — 32-bit unsigned division by a divisor that does not change from launch to launch (a layer's OW, OH * OW, channel groups ...):
// multiply-high, add, shift - three vector (or scalar) instructions where the runtime `/` of two registers is about 35.  Host + device, no HIP
// runtime call: the constants are made on the host where a layer's geometry is filled (engine.cpp), the kernels only apply them.
//
// The method is Granlund & Montgomery, "Division by Invariant Integers using Multiplication" (PLDI 1994), figure 4.1 with N = 32:
//   l = ceil(log2 d),  m = floor(2^32 (2^l - d) / d) + 1   (so that 2^32 + m = ceil(2^(32 + l) / d) for d no power of two, 2^32 + 1 for d = 2^l)
//   q = (mulhi(m, n) + n) >> l
// Proof of the range.  (2^32 + m) d = 2^(32 + l) + e with 0 < e <= d <= 2^l.  Then n (2^32 + m) / 2^(32 + l) = n / d + n e / (d 2^(32 + l)), and the
// second term is below n / (2^32 d) < 1 / d for n < 2^32: too small to carry n / d over the next integer, so the floor is floor(n / d) for EVERY
// 32-bit n.  What limits the range is the sum mulhi(m, n) + n in 32 bits: mulhi(m, n) <= n, so the sum stays below 2^32 for n < 2^31.
//   PROVEN RANGE: 1 <= d < 2^31, 0 <= n < 2^31 (every pixel / thread index a kernel forms as a non-negative int).  tests/cpp/fastdiv.cpp checks it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HP_FD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HP_FD_HD inline
#endif

namespace hp {

struct fastdiv {
    uint32_t d, m, s; // divisor, multiplier, shift; {0, 0, 0} = not filled (launchers refuse it: fastdiv_is)
};

// host side (engine build, launchers): the constants of divisor d, 1 <= d < 2^31
inline fastdiv make_fastdiv(long d)
{
    fastdiv f{ 0, 0, 0 };
    if (d < 1 || d >= (1L << 31))
        return f;
    uint32_t l = 0;
    while ((uint64_t(1) << l) < (uint64_t)d)
        ++l;
    f.d = (uint32_t)d, f.s = l;
    f.m = (uint32_t)(((uint64_t(1) << 32) * ((uint64_t(1) << l) - (uint64_t)d)) / (uint64_t)d + 1);
    return f;
}
// true where f holds the constants of divisor d (a launcher's guard: a params struct somebody filled without them must not reach a kernel)
inline bool fastdiv_is(const fastdiv& f, long d)
{
    const fastdiv g = make_fastdiv(d);
    return g.d != 0 && f.d == g.d && f.m == g.m && f.s == g.s;
}

HP_FD_HD uint32_t fd_mulhi(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
// n / d for 0 <= n < 2^31
HP_FD_HD uint32_t fd_div(uint32_t n, const fastdiv f) { return (fd_mulhi(f.m, n) + n) >> f.s; }
// n / d and n % d
HP_FD_HD void fd_divmod(uint32_t n, const fastdiv f, uint32_t& q, uint32_t& r)
{
    q = fd_div(n, f);
    r = n - q * f.d;
}

// Pixel index n of a B x OH x OW map (n = (b * OH + oy) * OW + ox) -> image b and row oy; ohw / ow = the constants of OH * OW and OW.
HP_FD_HD void fd_pixel(int n, const fastdiv ohw, const fastdiv ow, int& b, int& oy, int& rem)
{
    uint32_t q, r;
    fd_divmod((uint32_t)n, ohw, q, r);
    b = (int)q, rem = (int)r, oy = (int)fd_div(r, ow);
}
// The pixel's index in a view whose images are `img` pixels and whose rows are `wp` pixels apart: b * img + oy * wp + ox with ox = n - b OHW - oy OW,
// written without ox: n + b (img - OHW) + oy (wp - OW).
HP_FD_HD long fd_view_pixel(int n, int b, int oy, const fastdiv ohw, const fastdiv ow, int img, int wp)
{
    return n + (long)b * (img - (int)ohw.d) + (long)oy * (wp - (int)ow.d);
}
// The pixel `add` behind pixel n needs no carry loop (ox += add; while (ox >= OW) { ox -= OW; if (++oy == OH) oy = 0, ++b; }): fd_pixel(n + add)
// is eight instructions whatever the width, where the loop runs add / OW times per lane (sixteen on a one-pixel-wide map).

} // namespace hp
