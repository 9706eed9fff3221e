// resize_rois_device.hpp — many regions of ONE frame per launch: the sorted region table, the by-value geometry of a launch and the kernel body that
// hands resize_device.hpp's resize_pixel() a region as a frame of its own.  Shared by resize_rois.hip (8-bit BGR and every SDR hp_yuv_image layout; the
// contract and the launch shape are stated at its top) and resize_yuv_hdr.hip (PQ / HLG 10-bit frames): what differs between them is the Taps type only.
#pragma once
#include "resize_yuv_device.hpp"

namespace hp_resize {

constexpr int ROIS_PER_LAUNCH = 16, ROIS_MAX = 64;

struct roi_geom {
    int x, y, sw, sh; // the region inside the source frame
    int iw, ih, mode; // as in rz_geom
    int slot;         // destination slot (the caller's index of this region)
    double scale_x, scale_y;
};

struct roi_batch {
    uint8_t* dst;
    size_t slot_stride;
    int dw, dh, dst_stride;
    int bg[3];
    roi_geom r[ROIS_PER_LAUNCH];
};

template <class Taps> __device__ __forceinline__ void resize_rois_body(const roi_batch& b, const Taps& t)
{
    const int x = blockIdx.x * RZ_BLOCK_W + (threadIdx.x & 31), y = blockIdx.y * RZ_BLOCK_H + (threadIdx.x >> 5);
    if (x >= b.dw || y >= b.dh)
        return;
    const roi_geom& r = b.r[blockIdx.z];
    rz_geom g;
    g.sw = r.sw, g.sh = r.sh;
    g.dst = b.dst + (size_t)r.slot * b.slot_stride;
    g.dw = b.dw, g.dh = b.dh, g.dst_stride = b.dst_stride;
    g.iw = r.iw, g.ih = r.ih, g.mode = r.mode;
    g.scale_x = r.scale_x, g.scale_y = r.scale_y;
    g.bg[0] = b.bg[0], g.bg[1] = b.bg[1], g.bg[2] = b.bg[2];
    resize_pixel(g, t.at(r.x, r.y), x, y);
}

// every check of a call and the geometry of its regions, in launch order (sorted by y, then x, then index); nothing is launched here
inline int prepare_rois(const char* who, const char* format, int sw, int sh, int ax, int ay, const hp_roi* rois, int n, int keep_ratio, uint8_t* dst,
    int dw, int dh, int dst_stride, size_t slot_stride, const int bg[3], roi_geom (&out)[ROIS_MAX])
{
    HP_REQUIRE(n >= 1 && n <= ROIS_MAX, HP_ERR_INVALID, "%s: %s: %d regions (1 .. %d)", who, format, n, ROIS_MAX);
    HP_REQUIRE(rois && dst, HP_ERR_INVALID, "%s: %s: null argument", who, format);
    HP_REQUIRE(dw > 0 && dh > 0 && dst_stride >= dw * 3, HP_ERR_INVALID, "%s: %s: bad destination (%d x %d, row stride %d)", who, format, dw, dh, dst_stride);
    HP_REQUIRE(slot_stride >= (size_t)dh * dst_stride, HP_ERR_INVALID, "%s: %s: slot stride %zu is smaller than a slot (%d rows of %d bytes)", who, format,
        slot_stride, dh, dst_stride);
    int order[ROIS_MAX];
    for (int i = 0; i < n; ++i) {
        const hp_roi& r = rois[i];
        HP_REQUIRE(r.w > 0 && r.h > 0 && r.x >= 0 && r.y >= 0 && (int64_t)r.x + r.w <= sw && (int64_t)r.y + r.h <= sh, HP_ERR_INVALID,
            "%s: %s: region %d (%d x %d at %d, %d) is empty or not inside the %d x %d frame", who, format, i, r.w, r.h, r.x, r.y, sw, sh);
        HP_REQUIRE(r.x % ax == 0 && r.w % ax == 0 && r.y % ay == 0 && r.h % ay == 0, HP_ERR_INVALID,
            "%s: %s: region %d (%d x %d at %d, %d): x and w must be multiples of %d, y and h of %d", who, format, i, r.w, r.h, r.x, r.y, ax, ay);
        int k = i; // insertion sort, stable: n <= 64
        for (; k > 0 && (rois[order[k - 1]].y > r.y || (rois[order[k - 1]].y == r.y && rois[order[k - 1]].x > r.x)); --k)
            order[k] = order[k - 1];
        order[k] = i;
    }
    for (int k = 0; k < n; ++k) {
        const hp_roi& r = rois[order[k]];
        int iw = dw, ih = dh;
        if (keep_ratio)
            hp_letterbox_inner(r.w, r.h, dw, dh, &iw, &ih);
        rz_geom g;
        HP_TRY(rz_prepare(g, r.w, r.h, dst, dw, dh, dst_stride, iw, ih, bg));
        out[k] = roi_geom{ r.x, r.y, r.w, r.h, g.iw, g.ih, g.mode, order[k], g.scale_x, g.scale_y };
    }
    return HP_OK;
}

template <class Kernel, class Taps>
int launch_rois(Kernel kernel, const Taps& t, const roi_geom (&geom)[ROIS_MAX], int n, uint8_t* dst, int dw, int dh, int dst_stride, size_t slot_stride,
    const int bg[3], hipStream_t s)
{
    roi_batch b;
    b.dst = dst, b.slot_stride = slot_stride, b.dw = dw, b.dh = dh, b.dst_stride = dst_stride;
    b.bg[0] = bg[0], b.bg[1] = bg[1], b.bg[2] = bg[2];
    for (int at = 0; at < n; at += ROIS_PER_LAUNCH) {
        const int m = std::min(ROIS_PER_LAUNCH, n - at);
        for (int k = 0; k < ROIS_PER_LAUNCH; ++k)
            b.r[k] = geom[at + std::min(k, m - 1)]; // the unused entries repeat the last one: no z-slice reads them
        hipLaunchKernelGGL(kernel, dim3(hp::ceil_div(dw, RZ_BLOCK_W), hp::ceil_div(dh, RZ_BLOCK_H), m), dim3(256), 0, s, b, t);
        HP_HIP_TRY(hipGetLastError());
    }
    return HP_OK;
}

} // namespace hp_resize
