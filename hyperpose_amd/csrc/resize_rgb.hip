// resize_rgb.hip — hp_resize_rgb / hp_resize_rois_rgb: the fused resize fed by the packed 8-bit layouts of hp_rgb_image (include/hp_hip.h, "packed RGB
// and grey frames": BGR24, RGB24, BGRA32, RGBA32, ARGB32, ABGR32, GRAY8), with any stride, any orientation code and many regions per launch, so that a
// 4-byte, an RGB-order or a grey frame is read where it lies instead of being repacked to BGR24 on the CPU.  The contract: the bytes written equal
// what hp_resize_oriented_u8c3 / hp_resize_rois_oriented_u8c3 give on hp_rgb_to_bgr_host(src).  Nothing of the arithmetic is restated: the kernels are
// resize_pixel() / resize_rois_body() over oriented_taps<Taps> with the Taps of resize_rgb_device.hpp (which also says why no byte outside a row's
// width * pixel_bytes is read), and the host side - thread map, geometry, region table, refusals - is resize_oriented_host.hpp's.
//
// Orientation 0 runs this unit's kernels too (the identity map, ROWS): there is no un-oriented twin to forward to.
//
// Kernels (256 threads, one thread = one output pixel):
//     resize_rgb_kernel<COLS>     every layout through rgb_taps (byte loads), both thread maps
//     resize_rois_rgb_kernel      up to 16 upright regions per launch
//     resize_rgb32_kernel<COLS>, resize_rois_rgb32_kernel   the same through rgb32_taps (one 32-bit load per tap) for the four 4-byte layouts
// HP_RGB_TAPS=bytes|words (read at the first call) forces one Taps for the 4-byte layouts for measurements (tools/rgb_input_bench.py; DESIGN.md 1.1
// "Packed RGB and grey frames" holds both columns); HP_ORIENT_MAP works as in resize_oriented.hip.
#include "resize_oriented_host.hpp"
#include "resize_rgb_device.hpp"

namespace {

using namespace hp_resize;

template <bool COLS, class Taps> __device__ __forceinline__ void resize_rgb_body(const rz_geom& g, const Taps& t)
{
    int x, y;
    oriented_pixel_of_thread<COLS>(x, y);
    if (x >= g.dw || y >= g.dh)
        return;
    resize_pixel(g, t, x, y);
}

template <bool COLS> __global__ __launch_bounds__(256) void resize_rgb_kernel(const rz_geom g, const oriented_taps<rgb_taps> t) { resize_rgb_body<COLS>(g, t); }
template <bool COLS> __global__ __launch_bounds__(256) void resize_rgb32_kernel(const rz_geom g, const oriented_taps<rgb32_taps> t)
{
    resize_rgb_body<COLS>(g, t);
}
__global__ __launch_bounds__(256) void resize_rois_rgb_kernel(const roi_batch b, const oriented_taps<rgb_taps> t) { resize_rois_body(b, t); }
__global__ __launch_bounds__(256) void resize_rois_rgb32_kernel(const roi_batch b, const oriented_taps<rgb32_taps> t) { resize_rois_body(b, t); }

auto frame_kernel(const oriented_taps<rgb_taps>&, bool cols) { return cols ? resize_rgb_kernel<true> : resize_rgb_kernel<false>; }
auto frame_kernel(const oriented_taps<rgb32_taps>&, bool cols) { return cols ? resize_rgb32_kernel<true> : resize_rgb32_kernel<false>; }
auto rois_kernel(const oriented_taps<rgb_taps>&) { return resize_rois_rgb_kernel; }
auto rois_kernel(const oriented_taps<rgb32_taps>&) { return resize_rois_rgb32_kernel; }

// 4-byte layouts: one 32-bit load per tap unless HP_RGB_TAPS=bytes
bool word_taps()
{
    static const bool words = [] {
        const char* e = getenv("HP_RGB_TAPS");
        return !(e && strcmp(e, "bytes") == 0);
    }();
    return words;
}

// The one statement of "image description -> Taps": every check of the description, then f(taps) with the Taps type the layout reads through
template <class F> int with_rgb_taps(const char* who, const hp_rgb_image* im, F&& f)
{
    HP_TRY(hp_rgb::validate(im, who));
    const hp_rgb::layout& l = *hp_rgb::layout_of(im->format);
    if (l.pixel_bytes == 4 && word_taps())
        return f(word_taps_of(*im, l));
    return f(byte_taps_of(*im, l));
}

} // namespace

int hp_rgb::validate(const hp_rgb_image* im, const char* who, bool kernel_access)
{
    char msg[256];
    if (hp_rgb::check(im, who, kernel_access, msg, sizeof msg) != 0) {
        hp::set_error("%s", msg);
        return HP_ERR_INVALID;
    }
    return HP_OK;
}

extern "C" {

int hp_rgb_pixel_bytes(int format)
{
    const hp_rgb::layout* l = hp_rgb::layout_of(format);
    return l ? l->pixel_bytes : 0;
}

size_t hp_rgb_packed_bytes(int format, int width, int height) { return hp_rgb::packed_bytes(format, width, height); }

int hp_rgb_to_bgr_host(const hp_rgb_image* src, uint8_t* bgr, int bgr_stride)
{
    const char* who = "hp_rgb_to_bgr_host";
    HP_TRY(hp_rgb::validate(src, who, false));
    HP_REQUIRE(bgr, HP_ERR_INVALID, "%s: %s: null output", who, hp_rgb::layout_of(src->format)->name);
    HP_REQUIRE((int64_t)bgr_stride >= (int64_t)src->width * 3, HP_ERR_INVALID, "%s: %s: output stride %d is smaller than a BGR row (%lld bytes)", who,
        hp_rgb::layout_of(src->format)->name, bgr_stride, (long long)src->width * 3);
    hp_rgb::to_bgr(*src, bgr, bgr_stride);
    return HP_OK;
}

int hp_resize_rgb(const hp_rgb_image* src, int orientation, int keep_ratio, int b, int g, int r, uint8_t* dev_dst, int dw, int dh, int dst_stride,
    void* stream)
{
    const char* who = "hp_resize_rgb";
    HP_CHECK_ORIENTATION(who, orientation);
    return with_rgb_taps(who, src, [&](const auto& in) -> int {
        const int bg[3] = { b, g, r };
        rz_geom geom;
        HP_TRY(prepare_frame(orientation, src->width, src->height, keep_ratio, bg, dev_dst, dw, dh, dst_stride, geom));
        const auto t = orient(in, orientation, src->width, src->height);
        const bool cols = oriented_cols(orientation);
        hipLaunchKernelGGL(frame_kernel(t, cols), oriented_grid(geom, cols), dim3(256), 0, (hipStream_t)stream, geom, t);
        HP_HIP_TRY(hipGetLastError());
        return HP_OK;
    });
}

int hp_resize_rois_rgb(const hp_rgb_image* src, int orientation, const hp_roi* rois, int n, int keep_ratio, int b, int g, int r, uint8_t* dev_dst, int dw,
    int dh, int dst_stride, size_t slot_stride, void* stream)
{
    const char* who = "hp_resize_rois_rgb";
    HP_CHECK_ORIENTATION(who, orientation);
    return with_rgb_taps(who, src, [&](const auto& in) -> int {
        const int bg[3] = { b, g, r };
        roi_geom geom[ROIS_MAX];
        HP_TRY(prepare_oriented_rois(who, hp_rgb::layout_of(src->format)->name, orientation, src->width, src->height, 1, 1, rois, n, keep_ratio, dev_dst,
            dw, dh, dst_stride, slot_stride, bg, geom));
        const oriented_taps<std::decay_t<decltype(in)>> t{ in, 0, 0, orientation }; // (the origin is each region's, from geom)
        return launch_rois(rois_kernel(t), t, geom, n, dev_dst, dw, dh, dst_stride, slot_stride, bg, (hipStream_t)stream);
    });
}

} // extern "C"
