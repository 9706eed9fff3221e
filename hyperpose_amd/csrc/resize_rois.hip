// resize_rois.hip — hp_resize_rois_u8c3 / hp_resize_rois_yuv: N regions of ONE source frame (8-bit BGR, or any hp_yuv_image layout read
// where it lies) to N network-sized slots of one destination buffer, for inference on overlapping tiles of a frame that is much larger
// than the network's input (tiles.cpp plans the regions and merges the humans).
//
// The parity contract: slot i holds, byte for byte, what hp_resize_u8c3 / hp_resize_yuv (keep_ratio == 0) or hp_letterbox_u8c3 /
// hp_letterbox_yuv (keep_ratio != 0) give on region i cut out into a frame of its own - the w x h sub-image, or the sub-planes of every
// plane with the same matrix, range and depth.  Nothing of the arithmetic is restated here: a region is a frame whose pixel (0, 0) is
// the source's (x, y), so the kernels hand resize_device.hpp's resize_pixel() an rz_geom with the REGION's size (taps clamp at the
// region's edges, a pixel outside the region is never read) and the frame's Taps moved to the region's origin (Taps::at).  Mode (linear
// / area 2 x 2 / copy) and letterbox inner size are picked per region by rz_prepare() and hp_letterbox_inner(), as for a frame.
//
// Launch shape: one thread = one output pixel, 32 x 8 pixels per block of 256 threads as in resize.hip, the region is blockIdx.z.  The
// per-region geometry (48 bytes) travels by value in the kernel arguments, 16 regions per launch (a call with n regions makes ceil(n / 16)
// launches); everything a block needs of its region is wave-uniform and is read with scalar loads from the argument segment.  Regions
// overlap, so several z-slices fetch the same source lines: the z order is the regions sorted by (y, x), not the caller's order, so that
// slices which share source rows are neighbours in launch order and find those rows in L2 while they are resident (each region keeps
// its own destination slot).  The call only enqueues: no allocation, no synchronisation, no copy.
#include "resize_yuv_device.hpp"

namespace {

using namespace hp_resize;

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

__global__ __launch_bounds__(256) void resize_rois_u8c3_kernel(const roi_batch b, const bgr_taps t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_yuv_planar8_kernel(const roi_batch b, const yuv_taps<1, 1> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_yuv_packed8_kernel(const roi_batch b, const yuv_taps<1, 2> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_yuv_word16_kernel(const roi_batch b, const yuv_taps<2, 1> t) { resize_rois_body(b, t); }

// every check of a call and the geometry of its regions, in launch order (sorted by y, then x, then index); nothing is launched here
int prepare_rois(const char* who, const char* format, int sw, int sh, int ax, int ay, const hp_roi* rois, int n, int keep_ratio, uint8_t* dst,
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

} // namespace

extern "C" {

int hp_yuv_roi_alignment(int format, int* ax, int* ay)
{
    const hp_yuv::layout* l = hp_yuv::layout_of(format);
    HP_REQUIRE(l, HP_ERR_INVALID, "hp_yuv_roi_alignment: unknown format %d (HP_YUV_NV12 .. HP_YUV_I444)", format);
    if (ax)
        *ax = 1 << l->sx;
    if (ay)
        *ay = 1 << l->sy;
    return HP_OK;
}

int hp_resize_rois_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, const hp_roi* rois, int n, int keep_ratio, int b, int g, int r,
    uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream)
{
    HP_REQUIRE(dev_src && sw > 0 && sh > 0, HP_ERR_INVALID, "hp_resize_rois_u8c3: BGR: empty source");
    HP_REQUIRE(src_stride >= sw * 3, HP_ERR_INVALID, "hp_resize_rois_u8c3: BGR: row stride smaller than a row");
    const int bg[3] = { b, g, r };
    roi_geom geom[ROIS_MAX];
    HP_TRY(prepare_rois("hp_resize_rois_u8c3", "BGR", sw, sh, 1, 1, rois, n, keep_ratio, dev_dst, dw, dh, dst_stride, slot_stride, bg, geom));
    const bgr_taps t{ dev_src, src_stride };
    return launch_rois(resize_rois_u8c3_kernel, t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, (hipStream_t)stream);
}

int hp_resize_rois_yuv(const hp_yuv_image* src, const hp_roi* rois, int n, int keep_ratio, int b, int g, int r, uint8_t* dev_dst, int dw, int dh,
    int dst_stride, size_t slot_stride, void* stream)
{
    HP_TRY(hp_yuv::validate(src, "hp_resize_rois_yuv"));
    const hp_yuv::layout& l = *hp_yuv::layout_of(src->format);
    int32_t k[7];
    HP_TRY(hp_yuv_coefficients(src->matrix, src->range, l.sample_bytes == 2 ? 10 : 8, k));
    const int bg[3] = { b, g, r };
    roi_geom geom[ROIS_MAX];
    HP_TRY(prepare_rois("hp_resize_rois_yuv", l.name, src->width, src->height, 1 << l.sx, 1 << l.sy, rois, n, keep_ratio, dev_dst, dw, dh, dst_stride,
        slot_stride, bg, geom));
    const hipStream_t s = (hipStream_t)stream;
    if (l.sample_bytes == 2) {
        yuv_taps<2, 1> t;
        fill_taps(t, *src, l, k);
        return launch_rois(resize_rois_yuv_word16_kernel, t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, s);
    }
    if (l.planes == 1) {
        yuv_taps<1, 2> t;
        fill_taps(t, *src, l, k);
        return launch_rois(resize_rois_yuv_packed8_kernel, t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, s);
    }
    yuv_taps<1, 1> t;
    fill_taps(t, *src, l, k);
    return launch_rois(resize_rois_yuv_planar8_kernel, t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, s);
}

} // extern "C"
