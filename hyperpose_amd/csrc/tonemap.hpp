// tonemap.hpp — the ONE statement of how a PQ / HLG 10-bit video sample becomes an SDR sRGB byte (include/hp_hip.h, "HDR video in"; DESIGN.md
// 1.1): shared by the kernels of resize_yuv_hdr.hip, which convert a tap as they fetch it, and by the host twin hp_tonemap_convert_host
// (tonemap.cpp), which converts a whole frame; tests/hdr_ref.py restates it in numpy.  Everything a pixel goes through is integer arithmetic
// and table reads, so the three agree byte for byte; the floating point is confined to the tables, which are built once on the host
// (hp_tonemap_tables) and are the same array for everybody.
//
// Per source pixel, Y, U, V the 10-bit samples and k = hp_yuv_coefficients(matrix, range, 10):
//   1. non-linear R'G'B' at 10 bits:  u = U - c_off, v = V - c_off, yy = max(0, Y - y_off) * CY + (1 << 17),
//        E_B = sat10((yy + CUB*u) >> 18)   E_G = sat10((yy + CVG*v + CUG*u) >> 18)   E_R = sat10((yy + CVR*v) >> 18)
//      the products and sums of the 8-bit form (resize_yuv_device.hpp) shifted by 18 instead of 20: full scale is 255 * 4 = 1020
//   2. SDR linear light per channel:  L_c = A[E_c], A the 1024-entry uint16 table (PQ or HLG EOTF, then the tone curve, 65535 = SDR white)
//   3. primaries, when to_bt709:      (R, G, B) = clamp((M (L_R, L_G, L_B) + 2048) >> 12, 0, 65535), int32, arithmetic shift, M = rint(4096 M_2020->709)
//   4. sRGB bytes:                    c8 = O[value >> 4], O the 4096-entry uint8 table (sRGB OETF at the bin's centre)
// The largest |sum| of step 1 is 5.81e8 and of step 3 6.3e8 (6801 * 65535 + 2407 * 65535 + 298 * 65535 + 2048): inside int32.
#pragma once
#include <stdint.h>

#include "../../include/hp_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HP_HDR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HP_HDR_HD inline
#endif

namespace hp_hdr {

constexpr int LIN_N = 1024, OUT_N = 4096; // entries of A and O
constexpr int SHIFT10 = 18;               // step 1: the 2^20 coefficients of hp_yuv_coefficients give 10-bit R'G'B'
constexpr int M_SHIFT = 12;               // step 3: M is in units of 1 / 4096
constexpr size_t TABLE_BYTES = LIN_N * sizeof(uint16_t) + OUT_N; // A, then O: how the handle keeps them in device memory

HP_HDR_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the 24-bit multiply of yuv_taps::load where the device has one, exact for both uses: step 1 has coefficients below 2^23 and samples below
// 2^10, step 3 |M| <= 6801 < 2^13 and L < 2^16, and the low 32 bits of each product are the product
HP_HDR_HD int mul_coeff(int a, int b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// steps 1 - 4 for one pixel: u and v already have c_off subtracted.  k = { y_off, c_off, CY, CUB, CUG, CVG, CVR }; c = (B, G, R) bytes
HP_HDR_HD void convert(int Y, int u, int v, int y_off, int cy, int cub, int cug, int cvg, int cvr, const uint16_t* lin, const int32_t* m, bool primaries,
    const uint8_t* out, int (&c)[3])
{
    const int yy = mul_coeff(Y - y_off > 0 ? Y - y_off : 0, cy) + (1 << (SHIFT10 - 1));
    const int lb = lin[clampi((yy + mul_coeff(cub, u)) >> SHIFT10, 0, LIN_N - 1)];
    const int lg = lin[clampi((yy + mul_coeff(cvg, v) + mul_coeff(cug, u)) >> SHIFT10, 0, LIN_N - 1)];
    const int lr = lin[clampi((yy + mul_coeff(cvr, v)) >> SHIFT10, 0, LIN_N - 1)];
    int r = lr, g = lg, b = lb;
    if (primaries) {
        r = clampi((mul_coeff(m[0], lr) + mul_coeff(m[1], lg) + mul_coeff(m[2], lb) + (1 << (M_SHIFT - 1))) >> M_SHIFT, 0, 65535);
        g = clampi((mul_coeff(m[3], lr) + mul_coeff(m[4], lg) + mul_coeff(m[5], lb) + (1 << (M_SHIFT - 1))) >> M_SHIFT, 0, 65535);
        b = clampi((mul_coeff(m[6], lr) + mul_coeff(m[7], lg) + mul_coeff(m[8], lb) + (1 << (M_SHIFT - 1))) >> M_SHIFT, 0, 65535);
    }
    c[0] = out[b >> 4], c[1] = out[g >> 4], c[2] = out[r >> 4];
}

// host only (tonemap.cpp); `who` starts the message.  HP_OK or HP_ERR_INVALID (message set)
int check_desc(const hp_hdr_desc* d, const char* who);        // null, unknown transfer, non-finite or out-of-order peak / white
int check_frame(const hp_yuv_image* im, const char* who, bool kernel_access); // hp_yuv::validate, and the layout must be a 10-bit one

} // namespace hp_hdr

// the handle: the three tables of one hp_hdr_desc, immutable after hp_tonemap_create (resize_yuv_hdr.hip)
struct hp_tonemap {
    hp_hdr_desc desc;
    int32_t m[9];
    void* dev = nullptr; // TABLE_BYTES: A (uint16 [1024]), then O (uint8 [4096])
};
