// tonemap.cpp — the host side of "HDR video in" (include/hp_hip.h): hp_tonemap_tables, the ONE place where the transfer functions, the tone curve
// and the primaries matrix are evaluated (float64, then rounded to the three integer tables every pixel goes through); hp_tonemap_convert_host,
// the whole-frame twin of the kernels in resize_yuv_hdr.hip (the same csrc/tonemap.hpp convert(), so byte-equal); and hp_yuv_colours_hdr, the
// way back: draw_human's colours as HDR code values.  No device code, no device needed.
#include "tonemap.hpp"

#include "hp_common.hpp"
#include "overlay.hpp"
#include "yuv_formats.hpp"

#include <cmath>

namespace {

using namespace hp_hdr;

// SMPTE ST 2084
constexpr double PQ_M1 = 2610. / 16384., PQ_M2 = 128. * 2523. / 4096., PQ_C1 = 3424. / 4096., PQ_C2 = 32. * 2413. / 4096., PQ_C3 = 32. * 2392. / 4096.;
double pq_eotf(double e) // [0, 1] -> [0, 1] of 10 000 cd/m2
{
    const double p = std::pow(e, 1. / PQ_M2);
    return std::pow(std::max(p - PQ_C1, 0.) / (PQ_C2 - PQ_C3 * p), 1. / PQ_M1);
}
double pq_inverse_eotf(double y)
{
    const double p = std::pow(y, PQ_M1);
    return std::pow((PQ_C1 + PQ_C2 * p) / (1. + PQ_C3 * p), PQ_M2);
}

// BT.2100 HLG
constexpr double HLG_A = 0.17883277, HLG_B = 0.28466892, HLG_C = 0.55991073, HLG_GAMMA = 1.2, HLG_PEAK = 1000.;
double hlg_inverse_oetf(double e) { return e <= 0.5 ? e * e / 3. : (std::exp((e - HLG_C) / HLG_A) + HLG_B) / 12.; }
double hlg_oetf(double s) { return s <= 1. / 12. ? std::sqrt(3. * s) : HLG_A * std::log(12. * s - HLG_B) + HLG_C; }

double nits_of(int transfer, double e) { return transfer == HP_TRC_PQ ? 10000. * pq_eotf(e) : HLG_PEAK * std::pow(hlg_inverse_oetf(e), HLG_GAMMA); }
double signal_of(int transfer, double nits)
{
    return transfer == HP_TRC_PQ ? pq_inverse_eotf(nits / 10000.) : hlg_oetf(std::pow(nits / HLG_PEAK, 1. / HLG_GAMMA));
}

double srgb_oetf(double v) { return v <= 0.0031308 ? 12.92 * v : 1.055 * std::pow(v, 1. / 2.4) - 0.055; }
double srgb_eotf(double v) { return v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4); }

struct mat3 {
    double v[3][3];
};
mat3 mul(const mat3& a, const mat3& b)
{
    mat3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            r.v[i][j] = a.v[i][0] * b.v[0][j] + a.v[i][1] * b.v[1][j] + a.v[i][2] * b.v[2][j];
    return r;
}
mat3 inverse(const mat3& a)
{
    const double(*m)[3] = a.v;
    mat3 r;
    r.v[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1], r.v[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2], r.v[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    r.v[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2], r.v[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0], r.v[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    r.v[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0], r.v[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1], r.v[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    const double det = m[0][0] * r.v[0][0] + m[0][1] * r.v[1][0] + m[0][2] * r.v[2][0];
    for (auto& row : r.v)
        for (double& x : row)
            x /= det;
    return r;
}
// RGB -> XYZ of a set of primaries (x, y of R, G, B) with white D65: column i = S_i (x_i / y_i, 1, z_i / y_i), S = inv(P) W
mat3 rgb_to_xyz(const double xy[3][2])
{
    mat3 p;
    for (int i = 0; i < 3; ++i)
        p.v[0][i] = xy[i][0] / xy[i][1], p.v[1][i] = 1., p.v[2][i] = (1. - xy[i][0] - xy[i][1]) / xy[i][1];
    const double wx = 0.3127, wy = 0.3290, w[3] = { wx / wy, 1., (1. - wx - wy) / wy };
    const mat3 pi = inverse(p);
    for (int i = 0; i < 3; ++i) {
        const double s = pi.v[i][0] * w[0] + pi.v[i][1] * w[1] + pi.v[i][2] * w[2];
        for (int r = 0; r < 3; ++r)
            p.v[r][i] *= s;
    }
    return p;
}
mat3 bt2020_to_bt709()
{
    static const double P2020[3][2] = { { 0.708, 0.292 }, { 0.170, 0.797 }, { 0.131, 0.046 } }, P709[3][2] = { { 0.64, 0.33 }, { 0.30, 0.60 }, { 0.15, 0.06 } };
    return mul(inverse(rgb_to_xyz(P709)), rgb_to_xyz(P2020));
}

void tables(const hp_hdr_desc& d, uint16_t lin[LIN_N], int32_t m[9], uint8_t out[OUT_N])
{
    const double white = d.white_nits, p = (double)d.peak_nits / white;
    for (int i = 0; i < LIN_N; ++i) {
        const double x = nits_of(d.transfer, std::min(i, 1020) / 1020.) / white;
        lin[i] = (uint16_t)std::rint(65535. * std::min(1., x * (1. + x / (p * p)) / (1. + x)));
    }
    const mat3 M = bt2020_to_bt709();
    for (int i = 0; i < 9; ++i)
        m[i] = d.to_bt709 ? (int32_t)std::rint(4096. * M.v[i / 3][i % 3]) : (i % 4 == 0 ? 4096 : 0);
    for (int j = 0; j < OUT_N; ++j)
        out[j] = (uint8_t)std::rint(255. * srgb_oetf((16 * j + 7.5) / 65535.));
}

} // namespace

int hp_hdr::check_desc(const hp_hdr_desc* d, const char* who)
{
    HP_REQUIRE(d, HP_ERR_INVALID, "%s: null hp_hdr_desc", who);
    HP_REQUIRE(d->transfer == HP_TRC_PQ || d->transfer == HP_TRC_HLG, HP_ERR_INVALID, "%s: unknown transfer %d (HP_TRC_PQ, HP_TRC_HLG)", who, d->transfer);
    HP_REQUIRE(std::isfinite(d->peak_nits) && std::isfinite(d->white_nits), HP_ERR_INVALID, "%s: peak_nits %g / white_nits %g is not finite", who,
        (double)d->peak_nits, (double)d->white_nits);
    HP_REQUIRE(d->white_nits > 0.f && d->white_nits <= d->peak_nits && d->peak_nits <= 10000.f, HP_ERR_INVALID,
        "%s: white_nits %g, peak_nits %g: need 0 < white_nits <= peak_nits <= 10000", who, (double)d->white_nits, (double)d->peak_nits);
    return HP_OK;
}

int hp_hdr::check_frame(const hp_yuv_image* im, const char* who, bool kernel_access)
{
    HP_TRY(hp_yuv::validate(im, who, kernel_access));
    const hp_yuv::layout& l = *hp_yuv::layout_of(im->format);
    HP_REQUIRE(l.sample_bytes == 2, HP_ERR_INVALID, "%s: format %s is an 8-bit layout: the HDR path takes HP_YUV_P010 and HP_YUV_I010", who, l.name);
    return HP_OK;
}

extern "C" {

int hp_tonemap_tables(const hp_hdr_desc* d, uint16_t lin[1024], int32_t m[9], uint8_t out[4096])
{
    HP_TRY(hp_hdr::check_desc(d, "hp_tonemap_tables"));
    HP_REQUIRE(lin && m && out, HP_ERR_INVALID, "hp_tonemap_tables: null output (lin, m, out)");
    tables(*d, lin, m, out);
    return HP_OK;
}

int hp_tonemap_convert_host(const hp_yuv_image* f, const hp_hdr_desc* d, uint8_t* bgr, int stride)
{
    HP_TRY(hp_hdr::check_desc(d, "hp_tonemap_convert_host"));
    HP_TRY(hp_hdr::check_frame(f, "hp_tonemap_convert_host", false));
    HP_REQUIRE(bgr, HP_ERR_INVALID, "hp_tonemap_convert_host: null bgr");
    HP_REQUIRE((int64_t)stride >= (int64_t)f->width * 3, HP_ERR_INVALID, "hp_tonemap_convert_host: stride %d is smaller than a row (%lld bytes)", stride,
        (long long)f->width * 3);
    const hp_yuv::layout& l = *hp_yuv::layout_of(f->format);
    int32_t k[7], m[9];
    HP_TRY(hp_yuv_coefficients(f->matrix, f->range, 10, k));
    std::vector<uint16_t> lin(LIN_N);
    std::vector<uint8_t> out(OUT_N);
    tables(*d, lin.data(), m, out.data());
    const hp_yuv::sample_map s = hp_yuv::map_samples(*f, l);
    for (int y = 0; y < f->height; ++y)
        for (int x = 0; x < f->width; ++x) {
            const size_t at = (size_t)(y >> l.sy) * s.c_stride + (size_t)(x >> l.sx) * s.c_step;
            const int Y = hp_yuv::host_get(s.y + (size_t)y * s.y_stride + (size_t)x * s.y_step, 2, l.shift); // bytewise: any address
            const int U = hp_yuv::host_get(s.u + at, 2, l.shift), V = hp_yuv::host_get(s.v + at + (ptrdiff_t)(y >> l.sy) * s.v_extra, 2, l.shift);
            int c[3];
            convert(Y, U - k[1], V - k[1], k[0], k[2], k[3], k[4], k[5], k[6], lin.data(), m, d->to_bt709 != 0, out.data(), c);
            uint8_t* px = bgr + (size_t)y * stride + (size_t)x * 3;
            px[0] = (uint8_t)c[0], px[1] = (uint8_t)c[1], px[2] = (uint8_t)c[2];
        }
    return HP_OK;
}

int hp_yuv_colours_hdr(int matrix, int range, const hp_hdr_desc* d, int32_t out[19][3])
{
    HP_TRY(hp_hdr::check_desc(d, "hp_yuv_colours_hdr"));
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_yuv_colours_hdr: null output");
    HP_REQUIRE(matrix >= HP_YUV_BT601 && matrix <= HP_YUV_BT2020, HP_ERR_INVALID, "hp_yuv_colours_hdr: unknown matrix %d", matrix);
    HP_REQUIRE(range == HP_YUV_LIMITED || range == HP_YUV_FULL, HP_ERR_INVALID, "hp_yuv_colours_hdr: unknown range %d", range);
    static const double KR[3] = { 0.299, 0.2126, 0.2627 }, KB[3] = { 0.114, 0.0722, 0.0593 };
    const double kr = KR[matrix], kb = KB[matrix], kg = 1. - kr - kb;
    const mat3 back = inverse(bt2020_to_bt709());
    auto clip = [](double v) { return (int32_t)std::min(1023., std::max(0., std::nearbyint(v))); };
    for (int i = 0; i < 19; ++i) {
        double c[3], e[3];
        for (int j = 0; j < 3; ++j)
            c[j] = srgb_eotf(hp_ovl::COCO_COLOURS_RGB[i][j] / 255.);
        for (int j = 0; j < 3; ++j) {
            const double v = d->to_bt709 ? std::max(0., back.v[j][0] * c[0] + back.v[j][1] * c[1] + back.v[j][2] * c[2]) : c[j];
            e[j] = signal_of(d->transfer, v * (double)d->white_nits);
        }
        const double y = kr * e[0] + kg * e[1] + kb * e[2], cb = (e[2] - y) / (2. * (1. - kb)), cr = (e[0] - y) / (2. * (1. - kr));
        if (range == HP_YUV_LIMITED)
            out[i][0] = clip((16. + 219. * y) * 4.), out[i][1] = clip((128. + 224. * cb) * 4.), out[i][2] = clip((128. + 224. * cr) * 4.);
        else
            out[i][0] = clip(y * 1023.), out[i][1] = clip(512. + cb * 1023.), out[i][2] = clip(512. + cr * 1023.);
    }
    return HP_OK;
}

} // extern "C"
