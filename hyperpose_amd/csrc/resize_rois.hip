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
#include "resize_rois_device.hpp"

namespace {

using namespace hp_resize;

__global__ __launch_bounds__(256) void resize_rois_u8c3_kernel(const roi_batch b, const bgr_taps t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_yuv_planar8_kernel(const roi_batch b, const yuv_taps<1, 1> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_yuv_packed8_kernel(const roi_batch b, const yuv_taps<1, 2> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_yuv_word16_kernel(const roi_batch b, const yuv_taps<2, 1> t) { resize_rois_body(b, t); }

// this unit's kernel for each Taps type that with_yuv_taps() hands out
auto kernel_of(const yuv_taps<2, 1>&) { return resize_rois_yuv_word16_kernel; }
auto kernel_of(const yuv_taps<1, 2>&) { return resize_rois_yuv_packed8_kernel; }
auto kernel_of(const yuv_taps<1, 1>&) { return resize_rois_yuv_planar8_kernel; }

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
    return with_yuv_taps("hp_resize_rois_yuv", src, [&](const auto& t) -> int {
        const hp_yuv::layout& l = *hp_yuv::layout_of(src->format);
        const int bg[3] = { b, g, r };
        roi_geom geom[ROIS_MAX];
        HP_TRY(prepare_rois("hp_resize_rois_yuv", l.name, src->width, src->height, 1 << l.sx, 1 << l.sy, rois, n, keep_ratio, dev_dst, dw, dh, dst_stride,
            slot_stride, bg, geom));
        return launch_rois(kernel_of(t), t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, (hipStream_t)stream);
    });
}

} // extern "C"
