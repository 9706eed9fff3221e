// conv_i8.hip — int8 matrix-pipe convolution of HP_DTYPE_I8 engines (post-training quantization, TensorRT's kINT8) and the
// calibration reduction.
//
//   conv_i8_kernel   dense k x k convolution as an implicit GEMM on v_mfma_i32_32x32x32_i8, modelled on conv_mfma_kernel:
//                    D[cout][pixel] = sum_{tap,cin} q_w[tap][cout][cin] * q_x[pixel@tap][cin], exact int32 sums.
//                    256 threads = 2 x 2 wavefronts, block tile BM (64 | 128 output channels) x 128 pixels x BK (32 | 64
//                    input channels of one tap).  The weights are int8 already (quantized on the host per output channel);
//                    the activation tile is read as fp16 and quantized while it is staged global -> LDS:
//                    q_x = clamp(rint(x * inv_a), -127, 127), round-half-even, exact fp32 product - the zero halo quantizes to 0.
//                    Two LDS buffers, one barrier per K-step, the global loads of step s + 1 in flight while step s computes.
//                    Epilogue: v = (float)acc * dq[c], then the fp16 engine's own epilogue (conv_epilogue.hpp) adds the bias and applies
//                    the activation, residual, concat offset, fp16 NHWC store and the fused fp32 NCHW output copy.
//   conv_i8_direct_kernel  K x K stride-1 layers (VGG19's 7 x 7 stages, the 3 x 3 backbones), modelled on conv_direct_kernel: a block owns
//                    128 output channels x an 8 x 16 output tile of one image; per 64-channel chunk the (8 + K - 1) x (16 + K - 1) input halo
//                    is read ONCE, quantized while it is staged and kept in LDS (64 bytes per pixel, half the fp16 tile), and all K * K taps
//                    read their B fragments from it - every input element is quantized once per chunk, not once per tap.  The weights
//                    stream from L2 in MFMA-fragment order (one coalesced 1 KB load per wavefront and K-step, prefetched a step ahead).
//                    Four wavefronts, each 32 output channels x 128 pixels.  Same integers, same sums, same epilogue: its results equal
//                    conv_i8_kernel's bit for bit.
//   absmax_kernel    max |x| of one layer's input channel range over [n, H, W] (calibration, TensorRT's MinMax rule): per-block
//                    maximum, then one vector atomic max on the float's bits.
//
// Both operands' fragments are read with the same lane map (row = lane & 31, 16 consecutive k at 16 * (lane >> 5)), so the k order
// the instruction uses inside a lane pair cancels out of the sum; the C/D layout is the one of every 32 x 32 MFMA on gfx950.
#include "conv_device.hpp"
#include "conv_epilogue.hpp"
#include "conv_i8.hpp"

namespace hp {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

namespace {

// 16-byte chunk `chunk` of LDS row `row` (BK bytes per row), XOR-swizzled so that the 16-lane groups of ds_read_b128 hit 16 distinct slots
template <int BK>
__device__ __forceinline__ int i8_lds_off(int row, int chunk)
{
    if (BK == 64)
        return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4);
    else
        return row * 32 + ((chunk ^ ((row >> 3) & 1)) << 4);
}

__device__ __forceinline__ unsigned quant1(_Float16 h, float inv_a)
{
    const float q = fminf(fmaxf(__builtin_rintf((float)h * inv_a), -127.f), 127.f);
    return (unsigned)(int)q & 0xffu;
}

// eight fp16 values (one 16-byte load) -> eight int8 (two dwords)
__device__ __forceinline__ uint2 quant8(u32x4 raw, float inv_a)
{
    const half8 h = __builtin_bit_cast(half8, raw);
    uint2 r;
    r.x = quant1(h[0], inv_a) | quant1(h[1], inv_a) << 8 | quant1(h[2], inv_a) << 16 | quant1(h[3], inv_a) << 24;
    r.y = quant1(h[4], inv_a) | quant1(h[5], inv_a) << 8 | quant1(h[6], inv_a) << 16 | quant1(h[7], inv_a) << 24;
    return r;
}

} // namespace

template <int BM, int BK, int EPI>
__global__ __launch_bounds__(256) void conv_i8_kernel(const conv_i8_params q)
{
    const conv_params& p = q.c;
    constexpr int BN = 128;
    constexpr int TM = BM / 64, TN = BN / 64; // 32 x 32 tiles per wavefront (wave tile BM / 2 x 64)
    constexpr int CH = BK / 16;               // 16-byte int8 chunks per LDS row
    constexpr int A_UNITS = BM * CH;          // 16-byte weight loads per K-step
    constexpr int A_LD = (A_UNITS + 255) / 256;
    constexpr int C8 = BK / 8;                // 8-channel fp16 loads per pixel row
    constexpr int B_LD = BN * C8 / 256;
    constexpr int A_BYTES = BM * BK, TILE_BYTES = (BM + BN) * BK;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * TILE_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int MB = p.Cout_pad / BM;
    const int m0 = (blockIdx.x % MB) * BM, n0 = (blockIdx.x / MB) * BN;
    const int KC = p.Cin / BK, steps = p.KH * p.KW * KC;
    const int OHW = p.OH * p.OW;
    const float inv_a = q.inv_a;

    // activation rows (pixels) this thread stages; rows past the end alias the last pixel (loaded, never stored)
    long rowoff[B_LD];
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
        const int u = tid + i * 256, row = u / C8, c8 = u % C8;
        const int n = min(n0 + row, p.npix - 1);
        const int b = n / OHW, rem = n - b * OHW;
        const int oy = rem / p.OW, ox = rem - oy * p.OW;
        rowoff[i] = tv_off(p.in, b, oy * p.stride - p.pad_t, ox * p.stride - p.pad_l) + c8 * 8;
    }
    const long w_tap_stride = (long)p.Cout_pad * p.Cin;

    u32x4 ra[A_LD], rb[B_LD];
    auto gload = [&](int t) {
        const int tap = t / KC, kc = t - tap * KC, ky = tap / p.KW, kx = tap - ky * p.KW;
        const long toff = ((long)(ky * p.dil) * p.in.wp + kx * p.dil) * p.in.cs + kc * BK;
        const int8_t* wb = q.w + tap * w_tap_stride + kc * BK;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int u = tid + i * 256;
            if (A_UNITS % 256 == 0 || u < A_UNITS)
                ra[i] = *reinterpret_cast<const u32x4*>(wb + (long)(m0 + u / CH) * p.Cin + (u % CH) * 16);
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i)
            rb[i] = *reinterpret_cast<const u32x4*>(p.in.p + rowoff[i] + toff);
    };
    auto lstore = [&](int buf) {
        unsigned char* a_ = lds + buf * TILE_BYTES;
        unsigned char* b_ = a_ + A_BYTES;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int u = tid + i * 256;
            if (A_UNITS % 256 == 0 || u < A_UNITS)
                *reinterpret_cast<u32x4*>(a_ + i8_lds_off<BK>(u / CH, u % CH)) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int u = tid + i * 256, row = u / C8, c8 = u % C8;
            *reinterpret_cast<uint2*>(b_ + i8_lds_off<BK>(row, c8 >> 1) + (c8 & 1) * 8) = quant8(rb[i], inv_a);
        }
    };

    i32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc[i][j][r] = 0;

    const int frow = lane & 31, fk = lane >> 5;
    gload(0);
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        lstore(buf);
        __syncthreads(); // (buffer buf was last read in step s - 2, before every thread passed the barrier of step s - 1)
        if (s + 1 < steps)
            gload(s + 1);
        const unsigned char* a_ = lds + buf * TILE_BYTES;
        const unsigned char* b_ = a_ + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            i32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                fa[i] = *reinterpret_cast<const i32x4*>(a_ + i8_lds_off<BK>(wm * (BM / 2) + i * 32 + frow, ks * 2 + fk));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                fb[j] = *reinterpret_cast<const i32x4*>(b_ + i8_lds_off<BK>(wn * (BN / 2) + j * 32 + frow, ks * 2 + fk));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }

    // dequantize: lane holds channels m_wave + i * 32 + 8 g + 4 (lane >> 5) + {0..3}
    const int m_wave = m0 + wm * (BM / 2);
    floatx16 facc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 d = *reinterpret_cast<const float4*>(q.dq + m_wave + i * 32 + 8 * g + 4 * (lane >> 5));
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                facc[i][j][4 * g + 0] = (float)acc[i][j][4 * g + 0] * d.x;
                facc[i][j][4 * g + 1] = (float)acc[i][j][4 * g + 1] * d.y;
                facc[i][j][4 * g + 2] = (float)acc[i][j][4 * g + 2] * d.z;
                facc[i][j][4 * g + 3] = (float)acc[i][j][4 * g + 3] * d.w;
            }
        }
    int pb[TN], py[TN], px[TN];
    bool pv[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
        pv[j] = n < p.npix;
        const int nn = min(n, p.npix - 1);
        pb[j] = nn / OHW;
        const int rem = nn - pb[j] * OHW;
        py[j] = rem / p.OW;
        px[j] = rem - py[j] * p.OW;
    }
    conv_epilogue<TM, TN, EPI>(p, facc, m_wave, lane, pb, py, px, pv);
}

template <int K, int EPI>
__global__ __launch_bounds__(256) void conv_i8_direct_kernel(const conv_i8_params q, int tiles_x, int tiles_y)
{
    const conv_params& p = q.c;
    constexpr int TH = 8, TW = 16, HTH = TH + K - 1, HTW = TW + K - 1, HP = HTH * HTW;
    constexpr int UNITS = HP * 8;                  // 8-channel fp16 loads per chunk
    constexpr int ITER = (UNITS + 255) / 256;
    __shared__ __attribute__((aligned(16))) unsigned char lds[HP * 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int MB = p.Cout_pad / 128;
    int t = blockIdx.x;
    const int mt = t % MB;
    t /= MB;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW, m0 = mt * 128;
    const int NC = p.Cin / 64, MT = p.Cout_pad / 32, steps = K * K * 2;
    const float inv_a = q.inv_a;
    const int frow = lane & 31, fk = lane >> 5;

    // this lane's B rows: pixel j * 32 + frow of the tile -> its halo pixel at tap (0, 0)
    int hp0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = j * 32 + frow;
        hp0[j] = (pix >> 4) * HTW + (pix & 15);
    }
    // weight fragments of this wavefront: 1 KB per (tap, chunk, k-step), lane-contiguous
    const int8_t* wbase = q.w_direct + ((size_t)(m0 / 32 + wave) * 64 + lane) * 16;
    auto wfrag = [&](int c, int s) {
        const int tap = s >> 1, ks = s & 1;
        return *reinterpret_cast<const i32x4*>(wbase + ((((size_t)tap * NC + c) * 2 + ks) * MT) * 1024);
    };

    i32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[j][r] = 0;

    for (int c = 0; c < NC; ++c) {
        // stage the halo of chunk c, quantized; pixels outside the image read as zero (what the zero halo holds)
        u32x4 raw[ITER];
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int u = tid + i * 256;
            raw[i] = u32x4{ 0, 0, 0, 0 };
            if (u < UNITS) {
                const int hp = u >> 3, c8 = u & 7, hy = hp / HTW, hx = hp - hy * HTW;
                const int iy = oy0 - p.pad_t + hy, ix = ox0 - p.pad_l + hx;
                if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                    raw[i] = *reinterpret_cast<const u32x4*>(p.in.p + tv_off(p.in, b, iy, ix) + c * 64 + c8 * 8);
            }
        }
        i32x4 a_cur = wfrag(c, 0);
        if (c > 0)
            __syncthreads(); // every wavefront is done reading the previous chunk's tile
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int u = tid + i * 256;
            if (u < UNITS) {
                const int hp = u >> 3, c8 = u & 7;
                *reinterpret_cast<uint2*>(lds + hp * 64 + (((c8 >> 1) ^ ((hp >> 2) & 3)) << 4) + (c8 & 1) * 8) = quant8(raw[i], inv_a);
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < steps; ++s) {
            const i32x4 a_next = wfrag(c, s + 1 < steps ? s + 1 : s);
            const int tap = s >> 1, ks = s & 1, ky = tap / K, kx = tap - ky * K;
            i32x4 fb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int hp = hp0[j] + ky * HTW + kx;
                fb[j] = *reinterpret_cast<const i32x4*>(lds + hp * 64 + (((ks * 2 + fk) ^ ((hp >> 2) & 3)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_cur, fb[j], acc[j], 0, 0, 0);
            a_cur = a_next;
        }
    }

    const int m_wave = m0 + wave * 32;
    floatx16 facc[1][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 d = *reinterpret_cast<const float4*>(q.dq + m_wave + 8 * g + 4 * (lane >> 5));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            facc[0][j][4 * g + 0] = (float)acc[j][4 * g + 0] * d.x;
            facc[0][j][4 * g + 1] = (float)acc[j][4 * g + 1] * d.y;
            facc[0][j][4 * g + 2] = (float)acc[j][4 * g + 2] * d.z;
            facc[0][j][4 * g + 3] = (float)acc[j][4 * g + 3] * d.w;
        }
    }
    int pb[4], py[4], px[4];
    bool pv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = j * 32 + frow;
        py[j] = oy0 + (pix >> 4), px[j] = ox0 + (pix & 15), pb[j] = b;
        pv[j] = py[j] < p.OH && px[j] < p.OW;
        py[j] = min(py[j], p.OH - 1), px[j] = min(px[j], p.OW - 1);
    }
    conv_epilogue<1, 4, EPI>(p, facc, m_wave, lane, pb, py, px, pv);
}

bool conv_i8_direct_ok(const conv_params& p)
{
    return p.KH == p.KW && (p.KH == 3 || p.KH == 7) && p.stride == 1 && p.dil == 1 && p.Cin % 64 == 0 && p.Cout_pad % 128 == 0;
}

bool conv_i8_ok(int kh, int kw, int stride, int dil)
{
    if (kh != kw)
        return false;
    if (kh == 1)
        return dil == 1 && (stride == 1 || stride == 2);
    if (kh == 3)
        return (stride == 1 || stride == 2) && (dil == 1 || dil == 2);
    if (kh == 7)
        return stride == 1 && dil == 1;
    return false;
}

namespace {
int pick_bm(const conv_params& p) { return p.Cout_pad % 128 == 0 ? 128 : 64; }
int pick_bk(const conv_params& p) { return p.Cin % 64 == 0 ? 64 : 32; }
} // namespace

int conv_i8_tile(const conv_params& p) { return conv_i8_direct_ok(p) ? 8900000 + p.KH : 8000000 + pick_bm(p) * 1000 + pick_bk(p); }

hipError_t launch_conv_i8(const conv_i8_params& q, hipStream_t s)
{
    const conv_params& p = q.c;
    if (!conv_i8_ok(p.KH, p.KW, p.stride, p.dil) || p.Cin % 32 || p.Cout_pad % 64 || p.npix < 1 || !q.w || !q.dq)
        return hipErrorInvalidValue;
    // (EPI 0's half4 stores need 8-byte aligned channel groups: out.coff % 4 == 0)
    const int epi = (p.out_f32 || !p.out.p || p.Cout % 4 || p.out.coff % 4) ? 1 : 0;
    if (q.w_direct && conv_i8_direct_ok(p)) {
        const int tiles_x = (p.OW + 15) / 16, tiles_y = (p.OH + 7) / 8;
        const dim3 grid((unsigned)(tiles_x * tiles_y * p.B * (p.Cout_pad / 128))), block(256);
#define HP_I8D_LAUNCH(K_)                                                                                   \
    if (p.KH == K_) {                                                                                       \
        if (epi == 0)                                                                                       \
            HP_LAUNCH((conv_i8_direct_kernel<K_, 0>), grid, block, 0, s, q, tiles_x, tiles_y);              \
        else                                                                                                \
            HP_LAUNCH((conv_i8_direct_kernel<K_, 1>), grid, block, 0, s, q, tiles_x, tiles_y);              \
        return hipGetLastError();                                                                           \
    }
        HP_I8D_LAUNCH(3)
        HP_I8D_LAUNCH(7)
#undef HP_I8D_LAUNCH
    }
    const int BM = pick_bm(p), BK = pick_bk(p);
    const int nb = (p.npix + 127) / 128;
    const dim3 grid((unsigned)(p.Cout_pad / BM * nb)), block(256);
    // EPI 0: aligned half4 stores, whole 4-channel groups; EPI 1: per-element stores and the fp32 NCHW output copy
#define HP_I8_LAUNCH(BM_, BK_)                                                              \
    if (BM == BM_ && BK == BK_) {                                                           \
        if (epi == 0)                                                                       \
            HP_LAUNCH((conv_i8_kernel<BM_, BK_, 0>), grid, block, 0, s, q);                 \
        else                                                                                \
            HP_LAUNCH((conv_i8_kernel<BM_, BK_, 1>), grid, block, 0, s, q);                 \
        return hipGetLastError();                                                           \
    }
    HP_I8_LAUNCH(128, 64)
    HP_I8_LAUNCH(128, 32)
    HP_I8_LAUNCH(64, 64)
    HP_I8_LAUNCH(64, 32)
#undef HP_I8_LAUNCH
    return hipErrorInvalidValue;
}

__global__ __launch_bounds__(256) void absmax_kernel(const tview t, int H, int W, int C, long total, unsigned* amax)
{
    __shared__ float red[4];
    float m = 0.f;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long pix = idx / C;
        const int c = (int)(idx - pix * C);
        const int b = (int)(pix / ((long)H * W)), rem = (int)(pix - (long)b * H * W);
        const int y = rem / W, x = rem - y * W;
        m = fmaxf(m, fabsf(__half2float(t.p[tv_off(t, b, y, x) + c])));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicMax(amax, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

hipError_t launch_absmax(const tview& t, int B, int H, int W, int C, unsigned* amax, hipStream_t s)
{
    const long total = (long)B * H * W * C;
    if (total <= 0)
        return hipSuccess;
    const long blocks = std::min<long>((total + 255) / 256, 4096);
    HP_LAUNCH(absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, H, W, C, total, amax);
    return hipGetLastError();
}

} // namespace hp
