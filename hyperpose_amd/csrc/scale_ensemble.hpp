// scale_ensemble.hpp - the scale ensemble of PAF networks (include/hp_hip.h "scale ensemble"): the network runs on a frame and on
// K - 1 shrunken copies of it; the maps of every copy are resampled back to the map grid and the K sets of maps are averaged before parsing.  The
// ONE definition, for an engine with input in_w x in_h whose outputs all have H x W cells, in_w % W == 0 and in_h % H == 0:
//
//   scale s in (0, 1]:  mw = max(1, (int)floor((double)s * W + 0.5)),  mh likewise     (the valid map region: a whole number of cells)
//                       iw = mw * (in_w / W),  ih = mh * (in_h / H)                    (the shrunken slot's content, top-left)
//   stage   slot (k, i) = the network-sized slot i resized (resize_device.hpp, the mode cv::resize picks) into the top-left iw_k x ih_k, the rest
//           filled with (b, g, r); it lies at index (k - 1) * n + i of the destination, scale-major
//   tables  (hp_scale_tables) OpenCV's bicubic (A = -0.75) from the valid region mw to the W cells of a map, fp32, border replicate (parity
//           with OpenCV unpinned, as for the front-end resize: tests/scale_ref.py restates the coefficients)
//   merge   for f < n, in place, K maps [C][H][W] per frame scale-major (the n frames, then the n frames at scale 1, ...):
//               acc = maps[f][c][y][x]
//               for k = 1 .. K-1:  row_r = ((wx0 * p[r][0] + wx1 * p[r][1]) + wx2 * p[r][2]) + wx3 * p[r][3]     r = 0 .. 3
//                                  acc = acc + (((wy0 * row_0 + wy1 * row_1) + wy2 * row_2) + wy3 * row_3)
//               maps[f][c][y][x] = acc * (1.0f / (float)K)
//           p read from maps[k * n + f][c] at the tables' rows and columns: only the valid mh_k x mw_k region is addressed; no fused operation
//
// No perm and no sign: a confidence and a unit-vector field do not change under scaling (PifPaf's offsets and scales and PoseProposal's grid do,
// hence PAF pipelines only).
#pragma once
#include "hp_common.hpp"

#include <algorithm>
#include <cmath>

namespace hp_scale {

constexpr int MAX_EXTRA = 3;   // K - 1 <= 3: scales 0.5, 1 (the frame), 1.5 and 2 in the reference; here only scales up to 1 (above: tiles)
constexpr int MAX_C = 256;
constexpr int MAX_N = 65535;   // gridDim.z of the merge

// one destination column (or row): four source columns and their weights
struct tap4 {
    int32_t idx[4];
    float wgt[4];
};

// the valid map region of scale s over W cells (the caller has checked s)
inline int cells(float s, int W) { return std::max(1, (int)std::floor((double)s * W + 0.5)); }

// what every call that takes scales refuses: 1 .. 3 of them, each finite and in (0, 1]
inline int check_scales(const char* who, const float* scales, int n_scales)
{
    HP_REQUIRE(n_scales >= 1 && n_scales <= MAX_EXTRA, HP_ERR_INVALID, "%s: n_scales %d (1 .. %d extra scales, K = 2 .. %d)", who, n_scales, MAX_EXTRA,
        MAX_EXTRA + 1);
    HP_REQUIRE(scales, HP_ERR_INVALID, "%s: scales is null", who);
    for (int k = 0; k < n_scales; ++k)
        HP_REQUIRE(std::isfinite(scales[k]) && scales[k] > 0.f && scales[k] <= 1.f, HP_ERR_INVALID, "%s: scale %g (scales[%d]) is outside (0, 1]", who,
            (double)scales[k], k);
    return HP_OK;
}

// the device tables of K - 1 scales, one allocation: the x tables [K-1][W], then the y tables [K-1][H]
inline size_t tables_entries(int n_scales, int H, int W) { return (size_t)n_scales * (W + H); }
int fill_tables(tap4* out, const float* scales, int n_scales, int H, int W); // host; the layout above

// the engine's launches (scale_ensemble.hip): arguments already checked by the setter
int launch_stage(const uint8_t* dev_src, uint8_t* dev_dst, int w, int h, int n, int map_w, int map_h, const float* scales, int n_scales, const int bgr[3],
    hipStream_t s);
int launch_merge(float* dev_maps, int n, int K, int C, int H, int W, const tap4* dev_tables, hipStream_t s);

} // namespace hp_scale
