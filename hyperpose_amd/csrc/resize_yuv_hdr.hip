// resize_yuv_hdr.hip — hp_resize_yuv_hdr / hp_letterbox_yuv_hdr / hp_resize_rois_yuv_hdr: a PQ or HLG 10-bit frame (P010 / I010, read where it
// lies) straight to the network's 8-bit sRGB BGR input, tone-mapped as each tap is fetched.  The rule is csrc/tonemap.hpp's convert() - the one the
// host twin (tonemap.cpp) runs - so the output equals "hp_tonemap_convert_host, then hp_resize_u8c3 / hp_letterbox_u8c3" byte for byte; the resize
// arithmetic is resize_device.hpp's resize_pixel(), the addressing is yuv_taps<2, 1>'s, the region table is resize_rois_device.hpp's.  The Taps type that
// ends in table reads instead of sat8 is resize_yuv_hdr_device.hpp's; this file adds the kernels and the handle that owns the tables.
//
// Two kernels, each the shape of its SDR twin (one thread = one output pixel, 32 x 8 pixels per block of 256 threads; regions: blockIdx.z):
//     resize_yuv_hdr_kernel        one frame per launch          (resize_yuv_word16_kernel)
//     resize_rois_yuv_hdr_kernel   up to 16 regions per launch   (resize_rois_yuv_word16_kernel)
// What is launch-uniform travels in the kernel arguments: geometry, plane addresses, the seven matrix integers, the nine of M and whether step 3
// runs at all (to_bt709 == 0 skips it by a uniform branch).
//
// Where the 6 KiB of tables live.  A linear-mode pixel loads 8 samples and makes 24 table reads (4 taps x 3 channels x (A, O)) at data-dependent
// indices, so the table reads, not the arithmetic, are the kernel's cost.  Both placements are built (template parameter LDS):
//     LDS      every block copies A and O into LDS first (768 8-byte loads and ds_write_b64, 3 per thread, then one barrier) and reads
//              them with ds_read_u16 / ds_read_u8: a wavefront's 64 indices spread over the banks, and equal indices broadcast
//     global   the reads go to device memory through the vector cache: the tables are hot in L1 after the first few wavefronts of a CU, but a
//              gather of 64 different addresses is served cache line by cache line
// The default is LDS; HP_HDR_TABLES=global (read at the first call) selects the other for measurements (tools/yuv_kernel_bench.py; DESIGN.md 1.1
// holds both figures).
#include "resize_yuv_hdr_device.hpp"

#include <cstdlib>
#include <memory>

namespace {

using namespace hp_resize;

// yuv_hdr_taps, stage_tables() and prepare_hdr(): resize_yuv_hdr_device.hpp, shared with the oriented kernels of resize_oriented.hip

template <bool LDS> __global__ __launch_bounds__(256) void resize_yuv_hdr_kernel(const rz_geom g, yuv_hdr_taps t)
{
    __shared__ uint2 tables[LDS ? hp_hdr::TABLE_BYTES / sizeof(uint2) : 1];
    stage_tables<LDS>(t, tables);
    const int x = blockIdx.x * RZ_BLOCK_W + (threadIdx.x & 31), y = blockIdx.y * RZ_BLOCK_H + (threadIdx.x >> 5);
    if (x >= g.dw || y >= g.dh)
        return;
    resize_pixel(g, t, x, y);
}

template <bool LDS> __global__ __launch_bounds__(256) void resize_rois_yuv_hdr_kernel(const roi_batch b, yuv_hdr_taps t)
{
    __shared__ uint2 tables[LDS ? hp_hdr::TABLE_BYTES / sizeof(uint2) : 1];
    stage_tables<LDS>(t, tables);
    resize_rois_body(b, t);
}

bool tables_in_lds()
{
    static const bool lds = [] {
        const char* e = getenv("HP_HDR_TABLES");
        return !(e && strcmp(e, "global") == 0);
    }();
    return lds;
}

int launch_frame(const char* who, const hp_yuv_image* im, const hp_tonemap* tm, uint8_t* dst, int dw, int dh, int dst_stride, bool letterbox, const int bg[3],
    hipStream_t s)
{
    yuv_hdr_taps t;
    HP_TRY(prepare_hdr(who, im, tm, t));
    int iw = dw, ih = dh;
    if (letterbox)
        hp_letterbox_inner(im->width, im->height, dw, dh, &iw, &ih);
    rz_geom g;
    HP_TRY(rz_prepare(g, im->width, im->height, dst, dw, dh, dst_stride, iw, ih, bg));
    if (tables_in_lds())
        hipLaunchKernelGGL(resize_yuv_hdr_kernel<true>, rz_grid(g), dim3(256), 0, s, g, t);
    else
        hipLaunchKernelGGL(resize_yuv_hdr_kernel<false>, rz_grid(g), dim3(256), 0, s, g, t);
    HP_HIP_TRY(hipGetLastError());
    return HP_OK;
}

} // namespace

extern "C" {

int hp_tonemap_create(hp_tonemap** out, const hp_hdr_desc* d)
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_tonemap_create: null output");
    HP_TRY(hp_hdr::check_desc(d, "hp_tonemap_create"));
    std::unique_ptr<hp_tonemap> t(new hp_tonemap());
    t->desc = *d;
    std::vector<uint8_t> host(hp_hdr::TABLE_BYTES);
    HP_TRY(hp_tonemap_tables(d, reinterpret_cast<uint16_t*>(host.data()), t->m, host.data() + hp_hdr::LIN_N * sizeof(uint16_t)));
    HP_HIP_TRY(hipMalloc(&t->dev, hp_hdr::TABLE_BYTES));
    if (hipMemcpy(t->dev, host.data(), hp_hdr::TABLE_BYTES, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(t->dev);
        hp::set_error("hp_tonemap_create: copying the tables to the device failed");
        return HP_ERR_HIP;
    }
    *out = t.release();
    return HP_OK;
}

void hp_tonemap_destroy(hp_tonemap* t)
{
    if (!t)
        return;
    (void)hipDeviceSynchronize(); // launches that read the tables may still be in flight on any stream
    (void)hipFree(t->dev);
    delete t;
}

int hp_resize_yuv_hdr(const hp_yuv_image* src, const hp_tonemap* t, uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream)
{
    const int bg[3] = { 0, 0, 0 };
    return launch_frame("hp_resize_yuv_hdr", src, t, dev_dst, dw, dh, dst_stride, false, bg, (hipStream_t)stream);
}

int hp_letterbox_yuv_hdr(const hp_yuv_image* src, const hp_tonemap* t, uint8_t* dev_dst, int dw, int dh, int dst_stride, int b, int g, int r, void* stream)
{
    const int bg[3] = { b, g, r };
    return launch_frame("hp_letterbox_yuv_hdr", src, t, dev_dst, dw, dh, dst_stride, true, bg, (hipStream_t)stream);
}

int hp_resize_rois_yuv_hdr(const hp_yuv_image* src, const hp_tonemap* tm, const hp_roi* rois, int n, int keep_ratio, int b, int g, int r, uint8_t* dev_dst,
    int dw, int dh, int dst_stride, size_t slot_stride, void* stream)
{
    yuv_hdr_taps t;
    HP_TRY(prepare_hdr("hp_resize_rois_yuv_hdr", src, tm, t));
    const hp_yuv::layout& l = *hp_yuv::layout_of(src->format);
    const int bg[3] = { b, g, r };
    roi_geom geom[ROIS_MAX];
    HP_TRY(prepare_rois("hp_resize_rois_yuv_hdr", l.name, src->width, src->height, 1 << l.sx, 1 << l.sy, rois, n, keep_ratio, dev_dst, dw, dh, dst_stride,
        slot_stride, bg, geom));
    if (tables_in_lds())
        return launch_rois(resize_rois_yuv_hdr_kernel<true>, t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, (hipStream_t)stream);
    return launch_rois(resize_rois_yuv_hdr_kernel<false>, t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, (hipStream_t)stream);
}

} // extern "C"
