// scale_ensemble.hip - the two kernels of the scale ensemble, their host twins and the bicubic tables (the definition: scale_ensemble.hpp).
//   scale_stage_kernel  n network-sized u8 HWC slots shrunk into (K - 1) * n slots, scale-major: resize_device.hpp's resize_pixel, fill behind
//   scale_merge_kernel  maps[f] = (maps[f] + bicubic(maps[n + f]) + ...) * (1 / K) in place, on every network output
// Both move well under 1 MB per frame at LW-OpenPose sizes and are bound by launch latency: one thread per pixel / per element, no tuning.
// Compiled with -ffp-contract=off -fno-slp-vectorize: the merge is fp32 vector code in the engines' streams and the tables are
// fp32 host code that tests/scale_ref.py restates.
#include "resize_device.hpp"
#include "scale_ensemble.hpp"

#include <climits>
#include <mutex>
#include <tuple>
#include <map>

namespace {

using namespace hp_resize;
using hp_scale::tap4;

struct stage_geoms {
    rz_geom g[hp_scale::MAX_EXTRA]; // dst = the first slot of the scale's n slots
};

// grid (ceil(w / 32), ceil(h / 8), (K - 1) * n), blocks of 32 x 8 pixels as rz_grid has them; slot z = (k - 1) * n + i reads slot i of src
__global__ __launch_bounds__(256) void scale_stage_kernel(const uint8_t* __restrict__ src, int n, size_t slot_bytes, stage_geoms gs)
{
    const int x = blockIdx.x * RZ_BLOCK_W + (threadIdx.x & 31), y = blockIdx.y * RZ_BLOCK_H + (threadIdx.x >> 5);
    const int k = blockIdx.z / n, i = blockIdx.z - k * n; // wave-uniform
    rz_geom g = k == 0 ? gs.g[0] : (k == 1 ? gs.g[1] : gs.g[2]);
    if (x >= g.dw || y >= g.dh)
        return;
    g.dst += (size_t)i * slot_bytes;
    const bgr_taps t{ src + (size_t)i * slot_bytes, g.sw * 3 };
    resize_pixel(g, t, x, y);
}

// grid (ceil(H * W / 256), C, n): one thread per element of the n merged maps; tables: x [K-1][W], then y [K-1][H]
__global__ __launch_bounds__(256) void scale_merge_kernel(float* maps, int n, int K, int C, int W, int H, int plane /* H * W */, float inv,
    const tap4* __restrict__ tables)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= plane)
        return;
    const int c = blockIdx.y, f = blockIdx.z;
    const int y = i / W, x = i - y * W;
    float* pa = maps + ((size_t)f * C + c) * plane + i;
    float acc = *pa;
    for (int k = 1; k < K; ++k) {
        const tap4 tx = tables[(k - 1) * W + x], ty = tables[(K - 1) * W + (k - 1) * H + y];
        const float* p = maps + ((size_t)(k * n + f) * C + c) * plane;
        float row[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* pr = p + (size_t)ty.idx[r] * W;
            row[r] = ((tx.wgt[0] * pr[tx.idx[0]] + tx.wgt[1] * pr[tx.idx[1]]) + tx.wgt[2] * pr[tx.idx[2]]) + tx.wgt[3] * pr[tx.idx[3]];
        }
        const float v = ((ty.wgt[0] * row[0] + ty.wgt[1] * row[1]) + ty.wgt[2] * row[2]) + ty.wgt[3] * row[3];
        acc = acc + v;
    }
    *pa = acc * inv;
}

// what the device call and its host twin refuse
int check_merge(const char* who, const void* maps, int n, int K, int C, int H, int W, const float* scales)
{
    HP_REQUIRE(maps, HP_ERR_INVALID, "%s: maps is null", who);
    HP_REQUIRE(K >= 2 && K <= hp_scale::MAX_EXTRA + 1, HP_ERR_INVALID, "%s: K %d (2 .. %d maps per frame)", who, K, hp_scale::MAX_EXTRA + 1);
    HP_TRY(hp_scale::check_scales(who, scales, K - 1));
    HP_REQUIRE(C >= 1 && C <= hp_scale::MAX_C, HP_ERR_INVALID, "%s: C %d (1 .. %d)", who, C, hp_scale::MAX_C);
    HP_REQUIRE(H >= 1, HP_ERR_INVALID, "%s: H %d (>= 1)", who, H);
    HP_REQUIRE(W >= 1, HP_ERR_INVALID, "%s: W %d (>= 1)", who, W);
    HP_REQUIRE((long long)H * W <= INT_MAX, HP_ERR_INVALID, "%s: H %d x W %d: a map of more than 2^31 - 1 elements", who, H, W);
    HP_REQUIRE(n >= 1 && n <= hp_scale::MAX_N, HP_ERR_INVALID, "%s: n %d (1 .. %d frames per call)", who, n, hp_scale::MAX_N);
    return HP_OK;
}

int check_stage(const char* who, const void* src, const void* dst, int w, int h, int n, int map_w, int map_h, const float* scales, int n_scales, int b,
    int g, int r)
{
    HP_REQUIRE(src && dst, HP_ERR_INVALID, "%s: null pointer", who);
    HP_REQUIRE(w >= 1 && h >= 1 && n >= 1, HP_ERR_INVALID, "%s: w %d, h %d, n %d (all >= 1)", who, w, h, n);
    HP_REQUIRE(map_w >= 1 && map_h >= 1, HP_ERR_INVALID, "%s: map_w %d, map_h %d (both >= 1)", who, map_w, map_h);
    HP_REQUIRE(w % map_w == 0 && h % map_h == 0, HP_ERR_INVALID, "%s: the input %d x %d is not a whole number of map cells of %d x %d", who, w, h,
        map_w, map_h);
    HP_TRY(hp_scale::check_scales(who, scales, n_scales));
    HP_REQUIRE(b >= 0 && b <= 255 && g >= 0 && g <= 255 && r >= 0 && r <= 255, HP_ERR_INVALID, "%s: fill (%d, %d, %d) is outside 0 .. 255", who, b,
        g, r);
    HP_REQUIRE((long long)n * n_scales <= hp_scale::MAX_N, HP_ERR_INVALID, "%s: n %d x %d scales: more than %d slots per call", who, n, n_scales,
        hp_scale::MAX_N);
    const long long slot = (long long)w * h * 3;
    HP_REQUIRE(slot <= INT_MAX, HP_ERR_INVALID, "%s: a %d x %d slot is more than 2^31 - 1 bytes", who, w, h);
    const size_t in = (size_t)n * slot, out = (size_t)n * n_scales * slot;
    const uint8_t *s = (const uint8_t*)src, *d = (const uint8_t*)dst;
    HP_REQUIRE(s + in <= d || d + out <= s, HP_ERR_INVALID, "%s: src and dst overlap", who);
    return HP_OK;
}

// the geometry of scale k's slots: rz_prepare's checks and mode, as every other feed
int stage_geom(rz_geom& g, uint8_t* dst, int w, int h, int map_w, int map_h, float s, const int bgr[3])
{
    const int iw = hp_scale::cells(s, map_w) * (w / map_w), ih = hp_scale::cells(s, map_h) * (h / map_h);
    return rz_prepare(g, w, h, dst, w, h, w * 3, iw, ih, bgr);
}

void tables_of(int W, int mw, tap4* out)
{
    const float A = -0.75f;
    for (int x = 0; x < W; ++x) {
        float fx = (float)((x + 0.5) * ((double)mw / W) - 0.5);
        const int sx = (int)floorf(fx);
        fx -= sx;
        const float c0 = ((A * (fx + 1) - 5 * A) * (fx + 1) + 8 * A) * (fx + 1) - 4 * A;
        const float c1 = ((A + 2) * fx - (A + 3)) * fx * fx + 1;
        const float c2 = ((A + 2) * (1 - fx) - (A + 3)) * (1 - fx) * (1 - fx) + 1;
        const float c3 = 1.f - c0 - c1 - c2;
        const float c[4] = { c0, c1, c2, c3 };
        for (int j = 0; j < 4; ++j) {
            out[x].idx[j] = std::min(std::max(sx - 1 + j, 0), mw - 1);
            out[x].wgt[j] = c[j];
        }
    }
}

// the stand-alone hp_scale_merge's tables: uploaded once per (device, geometry, scales) and never written again, so a later call on any stream
// reads them without waiting for anything
const tap4* cached_tables(const float* scales, int n_scales, int H, int W, int* rc)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, std::vector<float>>, void*> cache;
    int dev = 0;
    *rc = HP_OK;
    if (hipGetDevice(&dev) != hipSuccess) {
        hp::set_error("hp_scale_merge: hipGetDevice failed");
        *rc = HP_ERR_HIP;
        return nullptr;
    }
    const auto key = std::make_tuple(dev, H, W, std::vector<float>(scales, scales + n_scales));
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end())
        return (const tap4*)it->second;
    std::vector<tap4> host(hp_scale::tables_entries(n_scales, H, W));
    hp_scale::fill_tables(host.data(), scales, n_scales, H, W);
    void* p = nullptr;
    if (hipMalloc(&p, host.size() * sizeof(tap4)) != hipSuccess || hipMemcpy(p, host.data(), host.size() * sizeof(tap4), hipMemcpyHostToDevice) != hipSuccess) {
        if (p)
            (void)hipFree(p);
        hp::set_error("hp_scale_merge: uploading %zu table entries failed", host.size());
        *rc = HP_ERR_HIP;
        return nullptr;
    }
    cache[key] = p;
    return (const tap4*)p;
}

} // namespace

namespace hp_scale {

int fill_tables(tap4* out, const float* scales, int n_scales, int H, int W)
{
    for (int k = 0; k < n_scales; ++k) {
        tables_of(W, cells(scales[k], W), out + (size_t)k * W);
        tables_of(H, cells(scales[k], H), out + (size_t)n_scales * W + (size_t)k * H);
    }
    return HP_OK;
}

int launch_stage(const uint8_t* dev_src, uint8_t* dev_dst, int w, int h, int n, int map_w, int map_h, const float* scales, int n_scales, const int bgr[3],
    hipStream_t s)
{
    stage_geoms gs{};
    const size_t slot = (size_t)w * h * 3;
    for (int k = 0; k < n_scales; ++k)
        HP_TRY(stage_geom(gs.g[k], dev_dst + (size_t)k * n * slot, w, h, map_w, map_h, scales[k], bgr));
    for (int k = n_scales; k < MAX_EXTRA; ++k)
        gs.g[k] = gs.g[0]; // never read: blockIdx.z < n_scales * n
    hipLaunchKernelGGL(scale_stage_kernel, dim3(hp::ceil_div(w, RZ_BLOCK_W), hp::ceil_div(h, RZ_BLOCK_H), n_scales * n), dim3(256), 0, s, dev_src, n,
        slot, gs);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

int launch_merge(float* dev_maps, int n, int K, int C, int H, int W, const tap4* dev_tables, hipStream_t s)
{
    const int plane = H * W;
    hipLaunchKernelGGL(scale_merge_kernel, dim3(hp::ceil_div(plane, 256), C, n), dim3(256), 0, s, dev_maps, n, K, C, W, H, plane, 1.0f / (float)K,
        dev_tables);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

} // namespace hp_scale

extern "C" {

int hp_scale_tables(int W, int mw, int32_t idx[][4], float wgt[][4])
{
    HP_REQUIRE(idx && wgt, HP_ERR_INVALID, "hp_scale_tables: null argument");
    HP_REQUIRE(W >= 1, HP_ERR_INVALID, "hp_scale_tables: W %d (>= 1)", W);
    HP_REQUIRE(mw >= 1 && mw <= W, HP_ERR_INVALID, "hp_scale_tables: mw %d (1 .. W = %d)", mw, W);
    std::vector<tap4> t(W);
    tables_of(W, mw, t.data());
    for (int x = 0; x < W; ++x)
        for (int j = 0; j < 4; ++j)
            idx[x][j] = t[x].idx[j], wgt[x][j] = t[x].wgt[j];
    return HP_OK;
}

int hp_scale_stage_u8c3(const uint8_t* dev_src, uint8_t* dev_dst, int w, int h, int n, int map_w, int map_h, const float* scales, int n_scales, int b,
    int g, int r, void* stream)
{
    HP_TRY(check_stage("hp_scale_stage_u8c3", dev_src, dev_dst, w, h, n, map_w, map_h, scales, n_scales, b, g, r));
    const int bgr[3] = { b, g, r };
    return hp_scale::launch_stage(dev_src, dev_dst, w, h, n, map_w, map_h, scales, n_scales, bgr, (hipStream_t)stream);
}

int hp_scale_stage_u8c3_host(const uint8_t* src, uint8_t* dst, int w, int h, int n, int map_w, int map_h, const float* scales, int n_scales, int b, int g,
    int r)
{
    HP_TRY(check_stage("hp_scale_stage_u8c3_host", src, dst, w, h, n, map_w, map_h, scales, n_scales, b, g, r));
    const int bgr[3] = { b, g, r };
    const size_t slot = (size_t)w * h * 3;
    for (int k = 0; k < n_scales; ++k)
        for (int i = 0; i < n; ++i) {
            rz_geom geo;
            HP_TRY(stage_geom(geo, dst + ((size_t)k * n + i) * slot, w, h, map_w, map_h, scales[k], bgr));
            const bgr_taps t{ src + (size_t)i * slot, w * 3 };
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x)
                    resize_pixel(geo, t, x, y);
        }
    return HP_OK;
}

int hp_scale_merge(float* dev_maps, int n, int K, int C, int H, int W, const float* scales, void* stream)
{
    HP_TRY(check_merge("hp_scale_merge", dev_maps, n, K, C, H, W, scales));
    int rc = HP_OK;
    const tap4* t = cached_tables(scales, K - 1, H, W, &rc);
    HP_TRY(rc);
    return hp_scale::launch_merge(dev_maps, n, K, C, H, W, t, (hipStream_t)stream);
}

int hp_scale_merge_host(float* maps, int n, int K, int C, int H, int W, const float* scales)
{
    HP_TRY(check_merge("hp_scale_merge_host", maps, n, K, C, H, W, scales));
    std::vector<tap4> t(hp_scale::tables_entries(K - 1, H, W));
    hp_scale::fill_tables(t.data(), scales, K - 1, H, W);
    const tap4 *xt = t.data(), *yt = t.data() + (size_t)(K - 1) * W;
    const size_t plane = (size_t)H * W;
    const float inv = 1.0f / (float)K;
    for (int f = 0; f < n; ++f)
        for (int c = 0; c < C; ++c) {
            float* pa = maps + ((size_t)f * C + c) * plane;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    float acc = pa[(size_t)y * W + x];
                    for (int k = 1; k < K; ++k) {
                        const tap4 &tx = xt[(size_t)(k - 1) * W + x], &ty = yt[(size_t)(k - 1) * H + y];
                        const float* p = maps + ((size_t)(k * n + f) * C + c) * plane;
                        float row[4];
                        for (int r = 0; r < 4; ++r) {
                            const float* pr = p + (size_t)ty.idx[r] * W;
                            row[r] = ((tx.wgt[0] * pr[tx.idx[0]] + tx.wgt[1] * pr[tx.idx[1]]) + tx.wgt[2] * pr[tx.idx[2]]) + tx.wgt[3] * pr[tx.idx[3]];
                        }
                        const float v = ((ty.wgt[0] * row[0] + ty.wgt[1] * row[1]) + ty.wgt[2] * row[2]) + ty.wgt[3] * row[3];
                        acc = acc + v;
                    }
                    pa[(size_t)y * W + x] = acc * inv;
                }
        }
    return HP_OK;
}

} // extern "C"
