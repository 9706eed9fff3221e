// flip_ensemble.hip - the two kernels of the flip ensemble and their host twins (the definition: flip_ensemble.hpp).
//   hflip_u8c3_kernel   n packed u8 HWC frames flipped left-right into a second buffer: the engine's input for the flipped pass
//   flip_merge_kernel   maps[f] = 0.5f * (maps[f] +- flip-back(maps[n + f])) in place, on every network output
// Both move well under 1 MB per frame at LW-OpenPose sizes and are bound by launch latency: one thread per pixel / per element, no tuning.
// Compiled with -ffp-contract=off -fno-slp-vectorize: the merge is fp32 vector code in the engines' streams.
#include "flip_ensemble.hpp"
#include "hp_common.hpp"

#include <climits>

namespace {

// one thread per pixel: 3 byte loads, 3 byte stores - any width, any alignment
__global__ __launch_bounds__(256) void hflip_u8c3_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int total /* n * h * w */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total)
        return;
    const int row = i / w, x = i - row * w;
    const uint8_t* s = src + ((size_t)row * w + (w - 1 - x)) * 3;
    uint8_t* d = dst + (size_t)i * 3;
    const uint8_t b = s[0], g = s[1], r = s[2];
    d[0] = b, d[1] = g, d[2] = r;
}

struct merge_tables {
    uint8_t perm[hp_flip::MAX_C];
    uint32_t minus[hp_flip::MAX_C / 32]; // bit c set: sign[c] < 0
};

// grid (ceil(H * W / 256), C, n): one thread per element of the n merged maps
__global__ __launch_bounds__(256) void flip_merge_kernel(float* maps, int n, int C, int W, int plane /* H * W */, merge_tables t)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= plane)
        return;
    const int c = blockIdx.y, f = blockIdx.z;
    const int y = i / W, x = i - y * W;
    float* pa = maps + ((size_t)f * C + c) * plane + i;
    const float a = *pa;
    const float b = maps[((size_t)(n + f) * C + t.perm[c]) * plane + (size_t)y * W + (W - 1 - x)];
    *pa = (t.minus[c >> 5] >> (c & 31)) & 1u ? 0.5f * (a - b) : 0.5f * (a + b);
}

// what the device call and its host twin refuse
int check_merge(const char* who, const void* maps, int n, int C, int H, int W, const int32_t* perm, const int8_t* sign)
{
    HP_REQUIRE(maps && perm && sign, HP_ERR_INVALID, "%s: null argument", who);
    HP_REQUIRE(n >= 1, HP_ERR_INVALID, "%s: n %d (>= 1)", who, n);
    HP_REQUIRE(C >= 1 && C <= hp_flip::MAX_C, HP_ERR_INVALID, "%s: C %d (1 .. %d)", who, C, hp_flip::MAX_C);
    HP_REQUIRE(H >= 1, HP_ERR_INVALID, "%s: H %d (>= 1)", who, H);
    HP_REQUIRE(W >= 1, HP_ERR_INVALID, "%s: W %d (>= 1)", who, W);
    HP_REQUIRE((long long)H * W <= INT_MAX, HP_ERR_INVALID, "%s: H %d x W %d: a map of more than 2^31 - 1 elements", who, H, W);
    for (int c = 0; c < C; ++c) {
        HP_REQUIRE(perm[c] >= 0 && perm[c] < C, HP_ERR_INVALID, "%s: perm[%d] = %d is outside [0, %d)", who, c, perm[c], C);
        HP_REQUIRE(sign[c] == 1 || sign[c] == -1, HP_ERR_INVALID, "%s: sign[%d] = %d is neither -1 nor +1", who, c, (int)sign[c]);
    }
    return HP_OK;
}

int check_hflip(const char* who, const void* src, const void* dst, int w, int h, int n)
{
    HP_REQUIRE(src && dst, HP_ERR_INVALID, "%s: null pointer", who);
    HP_REQUIRE(w >= 1 && h >= 1 && n >= 1, HP_ERR_INVALID, "%s: w %d, h %d, n %d (all >= 1)", who, w, h, n);
    const long long bytes = (long long)n * h * w * 3;
    HP_REQUIRE(bytes <= INT_MAX, HP_ERR_INVALID, "%s: %d frames of %d x %d are more than 2^31 - 1 bytes", who, n, w, h);
    const uint8_t *s = (const uint8_t*)src, *d = (const uint8_t*)dst;
    HP_REQUIRE(s + bytes <= d || d + bytes <= s, HP_ERR_INVALID, "%s: src and dst overlap", who);
    return HP_OK;
}

} // namespace

extern "C" {

int hp_hflip_u8c3(const uint8_t* dev_src, uint8_t* dev_dst, int w, int h, int n, void* stream)
{
    HP_TRY(check_hflip("hp_hflip_u8c3", dev_src, dev_dst, w, h, n));
    const int total = n * h * w;
    hipLaunchKernelGGL(hflip_u8c3_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, dev_src, dev_dst, w, total);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

int hp_hflip_u8c3_host(const uint8_t* src, uint8_t* dst, int w, int h, int n)
{
    HP_TRY(check_hflip("hp_hflip_u8c3_host", src, dst, w, h, n));
    for (size_t row = 0; row < (size_t)n * h; ++row)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c)
                dst[(row * w + x) * 3 + c] = src[(row * w + (w - 1 - x)) * 3 + c];
    return HP_OK;
}

int hp_flip_merge(float* dev_maps, int n, int C, int H, int W, const int32_t* perm, const int8_t* sign, void* stream)
{
    HP_TRY(check_merge("hp_flip_merge", dev_maps, n, C, H, W, perm, sign));
    HP_REQUIRE(n <= 65535, HP_ERR_INVALID, "hp_flip_merge: n %d (<= 65535 frames per call)", n);
    merge_tables t{};
    for (int c = 0; c < C; ++c) {
        t.perm[c] = (uint8_t)perm[c];
        if (sign[c] < 0)
            t.minus[c >> 5] |= 1u << (c & 31);
    }
    const int plane = H * W;
    hipLaunchKernelGGL(flip_merge_kernel, dim3((plane + 255) / 256, C, n), dim3(256), 0, (hipStream_t)stream, dev_maps, n, C, W, plane, t);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

int hp_flip_merge_host(float* maps, int n, int C, int H, int W, const int32_t* perm, const int8_t* sign)
{
    HP_TRY(check_merge("hp_flip_merge_host", maps, n, C, H, W, perm, sign));
    const size_t plane = (size_t)H * W;
    for (int f = 0; f < n; ++f)
        for (int c = 0; c < C; ++c) {
            float* pa = maps + ((size_t)f * C + c) * plane;
            const float* pb = maps + ((size_t)(n + f) * C + perm[c]) * plane;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const float a = pa[(size_t)y * W + x], b = pb[(size_t)y * W + (W - 1 - x)];
                    pa[(size_t)y * W + x] = sign[c] < 0 ? 0.5f * (a - b) : 0.5f * (a + b);
                }
        }
    return HP_OK;
}

int hp_flip_tables_coco(int conf_channels, int32_t* conf_perm, int32_t paf_perm[38], int8_t paf_sign[38])
{
    using namespace hp_flip;
    HP_REQUIRE(conf_channels == HP_COCO_N_PARTS || conf_channels == HP_COCO_N_PARTS + 1, HP_ERR_INVALID,
        "hp_flip_tables_coco: conf_channels %d: a COCO confidence output has 18 parts, or 19 channels with the background", conf_channels);
    HP_REQUIRE(conf_perm && paf_perm && paf_sign, HP_ERR_INVALID, "hp_flip_tables_coco: null argument");
    for (int c = 0; c < conf_channels; ++c)
        conf_perm[c] = c < HP_COCO_N_PARTS ? COCO_PART_FLIP[c] : c; // (the background is its own mirror image)
    for (int k = 0; k < HP_COCO_N_PAIRS; ++k) {
        int m = -1; // the limb whose two parts are the mirrored parts of limb k
        for (int j = 0; j < HP_COCO_N_PAIRS; ++j)
            if (COCO_PAIRS[j][0] == COCO_PART_FLIP[COCO_PAIRS[k][0]] && COCO_PAIRS[j][1] == COCO_PART_FLIP[COCO_PAIRS[k][1]])
                m = j;
        HP_REQUIRE(m >= 0, HP_ERR_STATE, "hp_flip_tables_coco: limb %d has no mirror image in the limb table", k);
        paf_perm[COCO_PAIRS_NET[k][0]] = COCO_PAIRS_NET[m][0], paf_sign[COCO_PAIRS_NET[k][0]] = -1; // x component
        paf_perm[COCO_PAIRS_NET[k][1]] = COCO_PAIRS_NET[m][1], paf_sign[COCO_PAIRS_NET[k][1]] = 1;  // y component
    }
    return HP_OK;
}

} // extern "C"
