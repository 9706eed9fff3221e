// to_yuv.hip — hp_rgb_to_yuv: a device-resident packed RGB or grey frame (hp_rgb_image) written as any hp_yuv_image layout in the target's matrix,
// range and bit depth, padded by edge replication to the size an encoder takes (include/hp_hip.h, "encoder hand-off").  The forward counterpart of
// hp_resize_yuv, and what lets the annotators (overlay.hip, redact.hip, mapview.hip) work on frames whose source was RGB.  WHAT is computed is stated
// once, in to_yuv.hpp (coefficients, pixel, chroma, padding, the host twin); this file holds the kernels and the C ABI.
//
// Kernels.  One launch per call, on the caller's stream; a pure streaming pass (4K BGRA -> NV12 reads 33 MB and writes 12 MB), shaped as the map
// view's painter is: one thread owns a horizontal run of RUN = 8 luma pixels, anchored at column 0, over one row of chroma blocks - 8 x 1 pixels
// (4:4:4, 4:2:2) or 8 x 2 (4:2:0) - and with it every byte of every plane those blocks own, so every byte has one writer: no atomics, no LDS.
//   loads    a run that lies whole inside the source is fetched as whole words - 32 bytes of a 4-byte layout (two dwordx4 where the address allows),
//            24 of a 3-byte one, 8 of grey - when its first byte is on a dword; a run that reaches over the source's right edge (padding repeats the
//            last pixel), or starts off a dword, goes pixel by pixel: one aligned word of a 4-byte layout, single bytes otherwise.  Either way no byte
//            outside width * pixel bytes of a row is read.  Rows below the source repeat its last row.
//   stores   a run that lies whole inside the output and whose row segment starts on a dword goes out as words: 8 Y bytes (dwordx2), 8 bytes of (U, V)
//            pairs or 4 + 4 of planar chroma on the 8-bit planes, 16 bytes (dwordx4) per row on the 16-bit planes and on packed 4:2:2.  The output's
//            last run when the width is no multiple of 8, and planes whose pointer or pitch is off a dword, go sample by sample.
// A block of 256 threads covers 64 runs x 4 block rows.  Variants follow mapview.hip's split: what changes the instructions of a store is a template
// parameter; the source layout is uniform over a launch and is branched on (scalar branches), so there is one kernel per kind of target:
//     to_yuv_planar8_kernel<PX, PY>        one byte per sample      NV12 I420 <2, 2>   NV16 I422 <2, 1>   I444 <1, 1>
//     to_yuv_word16_kernel                 16-bit words, << shift   P010 (6) I010 (0)
//     to_yuv_packed8_kernel                Y0 U Y1 V / U Y0 V Y1    YUY2 UYVY
// -Rpass-analysis=kernel-resource-usage (gfx950, the flags of hyperpose_amd/build.py): DESIGN.md 1.1 "Encoder hand-off".
#include "hp_common.hpp"
#include "to_yuv.hpp"

namespace {

using namespace hp_enc;

constexpr int RUN = 8, RUNS_X = 64, ROWS_Y = 4, THREADS = RUNS_X * ROWS_Y;

struct enc_src {
    const uint8_t* p;
    int stride, w, h;
    int pixel_bytes, b, g, r; // hp_rgb::layout
};

struct enc_geom {
    int dw, dh;      // the output's size
    int runs, brows; // runs of RUN luma pixels per row, rows of chroma blocks
    int top;         // 2^d - 1
    table t;
};

// ---- loads: the RUN pixels of one source row from column X0 on, each as R | G << 10 | B << 20 -------------------------------------------------------
// (ten bits a channel, so that the pixels of a chroma block are summed by adding such words: 4 * 255 < 1024)

template <int WORDS> __device__ __forceinline__ void load_words(const uint8_t* p, uint32_t (&v)[WORDS])
{
    const uintptr_t a = (uintptr_t)p;
    if constexpr (WORDS % 4 == 0) {
        if ((a & 15) == 0) {
#pragma unroll
            for (int k = 0; k < WORDS; k += 4) {
                const uint4 t = reinterpret_cast<const uint4*>(p)[k / 4];
                v[k] = t.x, v[k + 1] = t.y, v[k + 2] = t.z, v[k + 3] = t.w;
            }
            return;
        }
    }
    if constexpr (WORDS % 2 == 0) {
        if ((a & 7) == 0) {
#pragma unroll
            for (int k = 0; k < WORDS; k += 2) {
                const uint2 t = reinterpret_cast<const uint2*>(p)[k / 2];
                v[k] = t.x, v[k + 1] = t.y;
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < WORDS; ++k)
        v[k] = reinterpret_cast<const uint32_t*>(p)[k];
}

__device__ __forceinline__ uint32_t pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 10) | (b << 20); }

// byte j of a segment held as little-endian words
template <int WORDS> __device__ __forceinline__ uint32_t byte_of(const uint32_t (&v)[WORDS], int j) { return (v[j >> 2] >> (8 * (j & 3))) & 255u; }

__device__ __forceinline__ void load_run(const enc_src& s, int X0, int y, uint32_t (&px)[RUN])
{
    const uint8_t* row = s.p + (size_t)y * s.stride;
    const bool inside = X0 + RUN <= s.w; // else: the source's last pixel repeats
    const int last = s.w - 1;
    if (s.pixel_bytes == 4) {
        uint32_t v[RUN];
        if (inside)
            load_words<RUN>(row + (size_t)X0 * 4, v); // address and stride are multiples of 4 (hp_rgb::check)
        else {
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                v[i] = reinterpret_cast<const uint32_t*>(row)[min(X0 + i, last)];
        }
        const int sr = 8 * s.r, sg = 8 * s.g, sb = 8 * s.b;
#pragma unroll
        for (int i = 0; i < RUN; ++i)
            px[i] = pack_rgb((v[i] >> sr) & 255u, (v[i] >> sg) & 255u, (v[i] >> sb) & 255u);
    } else if (s.pixel_bytes == 3) {
        const uint8_t* at = row + (size_t)X0 * 3;
        const bool rgb = s.r == 0; // RGB24: R first
        if (inside && ((uintptr_t)at & 3) == 0) {
            uint32_t v[RUN * 3 / 4];
            load_words<RUN * 3 / 4>(at, v);
#pragma unroll
            for (int i = 0; i < RUN; ++i) {
                const uint32_t e0 = byte_of(v, 3 * i), e1 = byte_of(v, 3 * i + 1), e2 = byte_of(v, 3 * i + 2);
                px[i] = pack_rgb(rgb ? e0 : e2, e1, rgb ? e2 : e0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < RUN; ++i) {
                const uint8_t* q = row + (size_t)min(X0 + i, last) * 3;
                const uint32_t e0 = q[0], e1 = q[1], e2 = q[2];
                px[i] = pack_rgb(rgb ? e0 : e2, e1, rgb ? e2 : e0);
            }
        }
    } else {
        const uint8_t* at = row + X0;
        if (inside && ((uintptr_t)at & 3) == 0) {
            uint32_t v[RUN / 4];
            load_words<RUN / 4>(at, v);
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                px[i] = byte_of(v, i) * 0x100401u;
        } else {
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                px[i] = (uint32_t)row[min(X0 + i, last)] * 0x100401u;
        }
    }
}

// ---- stores ---------------------------------------------------------------------------------------------------------------------------------------

template <int WORDS> __device__ __forceinline__ void store_words(uint8_t* p, const uint32_t (&v)[WORDS])
{
    const uintptr_t a = (uintptr_t)p;
    if constexpr (WORDS == 4) {
        if ((a & 15) == 0) {
            *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
            return;
        }
    }
    if constexpr (WORDS % 2 == 0) {
        if ((a & 7) == 0) {
#pragma unroll
            for (int k = 0; k < WORDS; k += 2)
                reinterpret_cast<uint2*>(p)[k / 2] = make_uint2(v[k], v[k + 1]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < WORDS; ++k)
        reinterpret_cast<uint32_t*>(p)[k] = v[k];
}

// N samples of SB bytes each, contiguous from p, of which the first `valid` belong to the output: all of them on a dword go out as words, otherwise
// each of the first `valid` on its own.  16-bit samples are stored as value << shift.
template <int SB, int N> __device__ __forceinline__ void put_samples(uint8_t* p, const int (&c)[N], int valid, int shift)
{
    constexpr int WORDS = N * SB / 4, PER = 4 / SB, BITS = 8 * SB;
    static_assert(N * SB % 4 == 0, "a run's segment is whole dwords");
    if (valid == N && ((uintptr_t)p & 3) == 0) {
        uint32_t word[WORDS];
#pragma unroll
        for (int k = 0; k < WORDS; ++k) {
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j)
                out |= ((uint32_t)c[k * PER + j] << (SB == 2 ? shift : 0)) << (BITS * j);
            word[k] = out;
        }
        store_words<WORDS>(p, word);
        return;
    }
#pragma unroll
    for (int s = 0; s < N; ++s) {
        if (s >= valid)
            continue;
        if constexpr (SB == 2)
            reinterpret_cast<uint16_t*>(p)[s] = (uint16_t)(c[s] << shift); // planes and pitches of the 16-bit layouts are even (hp_yuv::validate)
        else
            p[s] = (uint8_t)c[s];
    }
}

template <int SB, int PX, int PY> struct planar_writer {
    static constexpr int NB = RUN / PX;
    uint8_t *y, *u, *v;
    int y_stride, c_stride, v_extra;
    int pairs; // the chroma plane holds (U, V) pairs
    int shift;
    // X0: the run's first luma column; `valid` luma pixels of the run belong to the output (a multiple of PX).  A luma row goes out as soon as it is
    // computed, so that a thread never holds two of them
    __device__ __forceinline__ void luma_row(int X0, int y_, const int (&yv)[RUN], int valid) const
    {
        put_samples<SB, RUN>(y + (size_t)y_ * y_stride + (size_t)X0 * SB, yv, valid, shift);
    }
    // by: the run's row of chroma blocks
    __device__ __forceinline__ void chroma_row(int X0, int by, const int (&)[RUN], const int (&cu)[NB], const int (&cv)[NB], int valid) const
    {
        const int bx = X0 / PX, blocks = valid / PX;
        if (pairs) {
            int c[NB * 2];
#pragma unroll
            for (int i = 0; i < NB; ++i)
                c[2 * i] = cu[i], c[2 * i + 1] = cv[i];
            put_samples<SB, NB * 2>(u + (size_t)by * c_stride + (size_t)bx * (2 * SB), c, blocks * 2, shift);
        } else {
            put_samples<SB, NB>(u + (size_t)by * c_stride + (size_t)bx * SB, cu, blocks, shift);
            put_samples<SB, NB>(v + (size_t)by * c_stride + (ptrdiff_t)by * v_extra + (size_t)bx * SB, cv, blocks, shift);
        }
    }
};

struct packed_writer {
    static constexpr int NB = RUN / 2;
    uint8_t* p;   // the macropixels' first byte
    int stride;
    int luma_odd; // UYVY: the luma samples are the odd bytes
    __device__ __forceinline__ void luma_row(int, int, const int (&)[RUN], int) const {} // luma and chroma share their words
    // yv: the luma samples of the block row's one pixel row
    __device__ __forceinline__ void chroma_row(int X0, int by, const int (&yv)[RUN], const int (&cu)[NB], const int (&cv)[NB], int valid) const
    {
        int c[RUN * 2];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int y0 = yv[2 * i], y1 = yv[2 * i + 1];
            c[4 * i] = luma_odd ? cu[i] : y0, c[4 * i + 1] = luma_odd ? y0 : cu[i], c[4 * i + 2] = luma_odd ? cv[i] : y1, c[4 * i + 3] = luma_odd ? y1 : cv[i];
        }
        put_samples<1, RUN * 2>(p + (size_t)by * stride + (size_t)X0 * 2, c, valid * 2, 0);
    }
};

template <int PX, int PY, class Writer> __device__ __forceinline__ void to_yuv_body(const enc_src& s, const enc_geom& g, const Writer& w)
{
    constexpr int NB = RUN / PX, LOG2N = (PX == 2) + (PY == 2);
    const int rx = (int)blockIdx.x * RUNS_X + (int)(threadIdx.x & (RUNS_X - 1)), by = (int)blockIdx.y * ROWS_Y + (int)(threadIdx.x / RUNS_X);
    if (rx >= g.runs || by >= g.brows)
        return;
    const int X0 = rx * RUN, valid = min(RUN, g.dw - X0);
    int yv[RUN];
    uint32_t sum[NB] = {}; // R, G and B of a block's pixels, summed in their ten-bit fields
#pragma unroll
    for (int dy = 0; dy < PY; ++dy) {
        uint32_t px[RUN];
        load_run(s, X0, min(by * PY + dy, s.h - 1), px);
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            yv[i] = luma(g.t, (int)(px[i] & 1023u), (int)((px[i] >> 10) & 1023u), (int)(px[i] >> 20), g.top);
            sum[i / PX] += px[i];
        }
        w.luma_row(X0, by * PY + dy, yv, valid);
    }
    int cu[NB], cv[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int rs = (int)(sum[i] & 1023u), gs = (int)((sum[i] >> 10) & 1023u), bs = (int)(sum[i] >> 20);
        cu[i] = chroma(g.t.u, g.t.c_off, rs, gs, bs, LOG2N, g.top);
        cv[i] = chroma(g.t.v, g.t.c_off, rs, gs, bs, LOG2N, g.top);
    }
    w.chroma_row(X0, by, yv, cu, cv, valid);
}

template <int PX, int PY> __global__ __launch_bounds__(THREADS) void to_yuv_planar8_kernel(const enc_src s, const enc_geom g, const planar_writer<1, PX, PY> w)
{
    to_yuv_body<PX, PY>(s, g, w);
}
__global__ __launch_bounds__(THREADS) void to_yuv_word16_kernel(const enc_src s, const enc_geom g, const planar_writer<2, 2, 2> w) { to_yuv_body<2, 2>(s, g, w); }
__global__ __launch_bounds__(THREADS) void to_yuv_packed8_kernel(const enc_src s, const enc_geom g, const packed_writer w) { to_yuv_body<2, 1>(s, g, w); }

// ---- the arguments of a call, checked ---------------------------------------------------------------------------------------------------------------

int check_call(const char* who, const hp_rgb_image* src, const hp_yuv_image* dst, bool kernel_access)
{
    HP_TRY(hp_yuv::validate(dst, who, kernel_access));
    HP_TRY(hp_rgb::validate(src, who, kernel_access));
    char msg[256];
    if (check_sizes(*src, *dst, who, msg, sizeof msg) != 0) {
        hp::set_error("%s", msg);
        return HP_ERR_INVALID;
    }
    return HP_OK;
}

template <int SB, int PX, int PY> planar_writer<SB, PX, PY> planar_of(const hp_yuv::sample_map& m, const hp_yuv::layout& l)
{
    planar_writer<SB, PX, PY> w;
    w.y = const_cast<uint8_t*>(m.y), w.u = const_cast<uint8_t*>(m.u), w.v = const_cast<uint8_t*>(m.v);
    w.y_stride = m.y_stride, w.c_stride = m.c_stride, w.v_extra = m.v_extra, w.pairs = l.planes == 2, w.shift = l.shift;
    return w;
}

} // namespace

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------------

extern "C" {

int hp_yuv_forward_coefficients(int matrix, int range, int depth, int32_t out[11])
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_yuv_forward_coefficients: null output");
    HP_REQUIRE(matrix >= HP_YUV_BT601 && matrix <= HP_YUV_BT2020, HP_ERR_INVALID, "hp_yuv_forward_coefficients: unknown matrix %d", matrix);
    HP_REQUIRE(range == HP_YUV_LIMITED || range == HP_YUV_FULL, HP_ERR_INVALID, "hp_yuv_forward_coefficients: unknown range %d", range);
    HP_REQUIRE(depth == 8 || depth == 10, HP_ERR_INVALID, "hp_yuv_forward_coefficients: depth %d (8 or 10)", depth);
    forward_coefficients(matrix, range, depth, out);
    return HP_OK;
}

int hp_yuv_padded_size(int format, int width, int height, int align, int* padded_width, int* padded_height)
{
    HP_REQUIRE(padded_width && padded_height, HP_ERR_INVALID, "hp_yuv_padded_size: null output");
    const hp_yuv::layout* l = hp_yuv::layout_of(format);
    HP_REQUIRE(l, HP_ERR_INVALID, "hp_yuv_padded_size: unknown format %d (HP_YUV_NV12 .. HP_YUV_I444)", format);
    HP_REQUIRE(width > 0 && height > 0 && width <= MAX_DIM && height <= MAX_DIM, HP_ERR_INVALID, "hp_yuv_padded_size: %s: a frame of %d x %d (1 .. %d)", l->name,
        width, height, MAX_DIM);
    HP_REQUIRE(align >= 1 && align <= MAX_ALIGN, HP_ERR_INVALID, "hp_yuv_padded_size: %s: align %d (1 .. %d)", l->name, align, MAX_ALIGN);
    padded_size(*l, width, height, align, padded_width, padded_height);
    return HP_OK;
}

int hp_rgb_to_yuv(const hp_rgb_image* src, const hp_yuv_image* dst, void* stream)
{
    HP_TRY(check_call("hp_rgb_to_yuv", src, dst, true));
    const hp_rgb::layout& in = *hp_rgb::layout_of(src->format);
    const hp_yuv::layout& l = *hp_yuv::layout_of(dst->format);
    const hp_yuv::sample_map m = hp_yuv::map_samples(*dst, l);
    const int depth = l.sample_bytes == 2 ? 10 : 8;
    const enc_src s { (const uint8_t*)src->data, src->stride, src->width, src->height, in.pixel_bytes, in.b, in.g, in.r };
    enc_geom g;
    g.dw = dst->width, g.dh = dst->height, g.runs = hp::ceil_div(dst->width, RUN), g.brows = dst->height >> l.sy, g.top = (1 << depth) - 1;
    g.t = table_of(dst->matrix, dst->range, depth);
    const dim3 grid(hp::ceil_div(g.runs, RUNS_X), hp::ceil_div(g.brows, ROWS_Y));
    const hipStream_t st = (hipStream_t)stream;
    if (l.sample_bytes == 2)
        hipLaunchKernelGGL(to_yuv_word16_kernel, grid, dim3(THREADS), 0, st, s, g, planar_of<2, 2, 2>(m, l));
    else if (l.planes == 1) {
        const uint8_t* first = m.y < m.u ? m.y : m.u;
        hipLaunchKernelGGL(to_yuv_packed8_kernel, grid, dim3(THREADS), 0, st, s, g, packed_writer{ const_cast<uint8_t*>(first), m.y_stride, m.y != first });
    } else if (l.sy == 1)
        hipLaunchKernelGGL((to_yuv_planar8_kernel<2, 2>), grid, dim3(THREADS), 0, st, s, g, planar_of<1, 2, 2>(m, l));
    else if (l.sx == 1)
        hipLaunchKernelGGL((to_yuv_planar8_kernel<2, 1>), grid, dim3(THREADS), 0, st, s, g, planar_of<1, 2, 1>(m, l));
    else
        hipLaunchKernelGGL((to_yuv_planar8_kernel<1, 1>), grid, dim3(THREADS), 0, st, s, g, planar_of<1, 1, 1>(m, l));
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

int hp_rgb_to_yuv_host(const hp_rgb_image* src, const hp_yuv_image* dst)
{
    HP_TRY(check_call("hp_rgb_to_yuv_host", src, dst, false));
    convert_host(*src, *dst);
    return HP_OK;
}

} // extern "C"
