// redact.hip — hp_redact_*: the heads or the whole persons of a frame pixelated or blacked out straight in a device-resident frame, 8-bit BGR
// or any hp_yuv_image layout, on the frame's own code values (include/hp_hip.h).  The write-back counterpart of overlay.hip: the frame never
// leaves the device.  WHAT is written is stated once, in redact.hpp (exact integer rules, the region list and the host painter included);
// this file holds the kernel, the handle and the C ABI.
//
// Kernel.  One launch per call.  The host computes the rectangle of cells the region list can reach, clipped to the frame; the grid covers those
// cells only: blockIdx.y is the cell row, one 64-lane wavefront owns one cell and a block holds four of them side by side.  A cell has exactly
// one owner, so a mean is never taken of half-rewritten samples, and there is no barrier, no LDS and no atomic.  The wavefront's index within the
// block goes through readfirstlane, which makes the cell and everything derived from it provably uniform: the loop over the region list (hits(),
// redact.hpp) runs on the scalar unit from scalar loads, and a wavefront whose cell no region reaches leaves at once.  In a hit cell the lanes
// walk each span's rows (redact.hpp, "spans"): a row of the cell is given to the smallest power of two of lanes that covers it (at most 64), the
// remaining lanes take the following rows, so consecutive lanes read consecutive samples and a 16-sample row keeps all 64 lanes busy on four
// rows.  Every lane keeps one int32 partial sum per channel; three __shfl_xor butterflies give every lane the sums, the counts come from the
// cell's geometry, and (sum + cnt / 2) / cnt is what the lanes then store over the same walk - every load of the cell precedes every store of it
// through that data dependence.  HP_REDACT_BLACK skips the loads.  The sample width (one byte, or 16-bit words with a shift) is the template
// parameter; addresses, strides, sub-sampling and the channel pattern are uniform and travel in the kernel arguments.
// Launch: grid = (ceil(cells across / 4), cells down), 256 threads.  -Rpass-analysis=kernel-resource-usage (gfx950, the flags of
// hyperpose_amd/build.py):
//     kernel                VGPRs  SGPRs  scratch  LDS bytes  waves / SIMD
//     redact_kernel<1>         16     41        0          0             8
//     redact_kernel<2>         16     43        0          0             8
//
// The list reaches the device through the handle (hp_redact), as for hp_overlay: an hp::staged_ring (annotate.hpp).  A call that has work takes
// the next slot, copies the regions into its pinned buffer, enqueues one hipMemcpyAsync and the kernel on the caller's stream and commits the
// slot; it waits (on the host) only if that slot's use SLOTS calls ago has not finished.  The frame checks both annotators make are there too.
#include "annotate.hpp"
#include "redact.hpp"

#include <algorithm>
#include <memory>

namespace {

using namespace hp_red;

constexpr int WAVES = 4, THREADS = WAVES * 64;

struct red_geom {
    const hp_redact_region* regs;
    int n_regs;
    int w, h, cell;
    int cx0, cy0, cx1; // first cell of the grid, last cell column of the list's rectangle (the grid's rows are exact)
    int effect;
    int n_spans, shift;
    span s[3];
    int black[3];
};

template <int SAMPLE_BYTES> __device__ __forceinline__ int load_sample(const uint8_t* q, int shift)
{
    if constexpr (SAMPLE_BYTES == 2)
        return (*reinterpret_cast<const uint16_t*>(q) >> shift) & 1023;
    else
        return *q;
}

template <int SAMPLE_BYTES> __device__ __forceinline__ void store_sample(uint8_t* q, int v, int shift)
{
    if constexpr (SAMPLE_BYTES == 2)
        *reinterpret_cast<uint16_t*>(q) = (uint16_t)(v << shift);
    else
        *q = (uint8_t)v;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off);
    return v;
}

// log2 of the lanes one row of `len` samples gets: the smallest power of two >= len, at most 64
__device__ __forceinline__ int lanes_log2(int len) { return len <= 1 ? 0 : min(6, 32 - __clz(len - 1)); }

template <int SAMPLE_BYTES> __global__ __launch_bounds__(THREADS) void redact_kernel(const red_geom g)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int ci = g.cx0 + (int)blockIdx.x * WAVES + wave, cj = g.cy0 + (int)blockIdx.y;
    if (ci > g.cx1)
        return;
    const int X0 = ci * g.cell, Y0 = cj * g.cell, X1 = min(X0 + g.cell, g.w) - 1, Y1 = min(Y0 + g.cell, g.h) - 1;
    bool hit = false;
    for (int i = 0; i < g.n_regs && !hit; ++i)
        hit = hits(g.regs[i], X0, Y0, X1, Y1);
    if (!hit)
        return;

    int value[3] = { g.black[0], g.black[1], g.black[2] };
    if (g.effect == HP_REDACT_PIXELATE) {
        int sum[3] = { 0, 0, 0 }, cnt[3] = { 0, 0, 0 };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k >= g.n_spans)
                break;
            const span s = g.s[k];
            int r0, r1, j0, j1;
            cell_of_span(s, X0, Y0, X1, Y1, r0, r1, j0, j1);
            const int blocks = ((X1 >> s.sx) - (X0 >> s.sx) + 1) * (r1 - r0 + 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (s.pat >> (2 * q)) & 3;
                if (q < s.k)
                    cnt[0] += c == 0 ? blocks : 0, cnt[1] += c == 1 ? blocks : 0, cnt[2] += c == 2 ? blocks : 0;
            }
            const int lg = lanes_log2(j1 - j0), per_row = 1 << lg;
            for (int r = r0 + (lane >> lg); r <= r1; r += 64 >> lg) {
                const uint8_t* row = s.base + (size_t)r * s.stride;
#pragma clang loop vectorize(disable)
                for (int j = j0 + (lane & (per_row - 1)); j < j1; j += per_row) {
                    const int v = load_sample<SAMPLE_BYTES>(row + (size_t)j * SAMPLE_BYTES, g.shift), c = channel_of(s, j);
                    sum[0] += c == 0 ? v : 0, sum[1] += c == 1 ? v : 0, sum[2] += c == 2 ? v : 0;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned total = (unsigned)wave_sum(sum[c]), count = (unsigned)cnt[c];
            value[c] = count ? (int)((total + count / 2) / count) : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.n_spans)
            break;
        const span s = g.s[k];
        int r0, r1, j0, j1;
        cell_of_span(s, X0, Y0, X1, Y1, r0, r1, j0, j1);
        const int lg = lanes_log2(j1 - j0), per_row = 1 << lg;
        for (int r = r0 + (lane >> lg); r <= r1; r += 64 >> lg) {
            uint8_t* row = s.base + (size_t)r * s.stride;
#pragma clang loop vectorize(disable)
            for (int j = j0 + (lane & (per_row - 1)); j < j1; j += per_row) {
                const int c = channel_of(s, j);
                store_sample<SAMPLE_BYTES>(row + (size_t)j * SAMPLE_BYTES, c == 0 ? value[0] : c == 1 ? value[1] : value[2], g.shift);
            }
        }
    }
}

} // namespace

// ---- the handle ---------------------------------------------------------------------------------------------------------------------------

struct hp_redact {
    int max_regions = 0;
    hp::staged_ring ring; // max_regions hp_redact_region per slot
};

namespace {

// ---- argument checks shared by the device and the host entry points ------------------------------------------------------------------------

int check_call(const char* who, const char* name, int w, int h, const hp_redact_region* regs, int n, int effect, int cell)
{
    HP_TRY(hp::check_max_dim(who, name, w, h));
    HP_REQUIRE(cell_ok(cell), HP_ERR_INVALID, "%s: %s: cell %d is not an even number in [%d, %d]", who, name, cell, MIN_CELL, MAX_CELL);
    HP_REQUIRE(effect == HP_REDACT_PIXELATE || effect == HP_REDACT_BLACK, HP_ERR_INVALID, "%s: %s: unknown effect %d", who, name, effect);
    HP_REQUIRE(n >= 0 && (n == 0 || regs), HP_ERR_INVALID, "%s: %s: %d regions at a null pointer or a negative count", who, name, n);
    for (int i = 0; i < n; ++i) {
        const char* fault = region_fault(regs[i]);
        HP_REQUIRE(!fault, HP_ERR_INVALID, "%s: %s: region %d (kind %d, %d, %d, %d, %d) is %s", who, name, i, regs[i].kind, regs[i].x0, regs[i].y0, regs[i].x1,
            regs[i].y1, fault);
    }
    return HP_OK;
}

int frame_bgr(frame& f, const char* who, uint8_t* bgr, int w, int h, int stride, const hp_redact_region* regs, int n, int effect, int cell)
{
    HP_TRY(hp::check_bgr_frame(who, bgr, w, h, stride));
    HP_TRY(check_call(who, "BGR", w, h, regs, n, effect, cell));
    describe_bgr(f, bgr, w, h, stride);
    return HP_OK;
}

int frame_yuv(frame& f, const char*& name, const char* who, const hp_yuv_image* im, bool kernel_access, const hp_redact_region* regs, int n, int effect, int cell)
{
    HP_TRY(hp_yuv::validate(im, who, kernel_access));
    const hp_yuv::layout& l = *hp_yuv::layout_of(im->format);
    name = l.name;
    HP_TRY(check_call(who, l.name, im->width, im->height, regs, n, effect, cell));
    describe_yuv(f, *im);
    return HP_OK;
}

int redact_device(hp_redact* r, const char* who, const char* name, const frame& f, const hp_redact_region* regs, int n, int effect, int cell, hipStream_t s)
{
    HP_REQUIRE(n <= r->max_regions, HP_ERR_INVALID, "%s: %s: %d regions, the handle was created for %d", who, name, n, r->max_regions);
    red_geom g;
    int cy1;
    if (n == 0 || !cell_rect(regs, n, f.w, f.h, cell, g.cx0, g.cy0, g.cx1, cy1))
        return HP_OK;
    hp_redact_region* staged;
    HP_TRY(r->ring.take(staged));
    std::copy(regs, regs + n, staged);
    HP_TRY(r->ring.upload((size_t)n * sizeof(hp_redact_region), s));
    g.regs = r->ring.device<hp_redact_region>(), g.n_regs = n, g.w = f.w, g.h = f.h, g.cell = cell, g.effect = effect;
    g.n_spans = f.n_spans, g.shift = f.shift;
    for (int k = 0; k < 3; ++k)
        g.s[k] = k < f.n_spans ? f.s[k] : span{}, g.black[k] = f.black[k];
    const dim3 grid(hp::ceil_div(g.cx1 - g.cx0 + 1, WAVES), cy1 - g.cy0 + 1);
    if (f.sample_bytes == 2)
        hipLaunchKernelGGL(redact_kernel<2>, grid, dim3(THREADS), 0, s, g);
    else
        hipLaunchKernelGGL(redact_kernel<1>, grid, dim3(THREADS), 0, s, g);
    return r->ring.commit(s);
}

} // namespace

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------

extern "C" {

int hp_redact_create(hp_redact** out, int max_regions)
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_redact_create: null output");
    *out = nullptr;
    HP_REQUIRE(max_regions > 0 && max_regions <= (1 << 20), HP_ERR_INVALID, "hp_redact_create: max_regions %d (1 .. 1048576)", max_regions);
    std::unique_ptr<hp_redact> r(new hp_redact); // a failed create frees what it allocated
    r->max_regions = max_regions;
    HP_TRY(r->ring.alloc((size_t)max_regions * sizeof(hp_redact_region), "hp_redact_create"));
    *out = r.release();
    return HP_OK;
}

void hp_redact_destroy(hp_redact* r) { delete r; } // the ring drains first

int hp_redact_regions(const hp_human* humans, int n, int w, int h, int what, float margin, hp_redact_region* out, int cap)
{
    HP_REQUIRE(w > 0 && h > 0 && w <= MAX_DIM && h <= MAX_DIM, HP_ERR_INVALID, "hp_redact_regions: frame %d x %d (1 .. %d)", w, h, MAX_DIM);
    HP_REQUIRE(n >= 0 && (n == 0 || humans) && cap >= 0 && (cap == 0 || out), HP_ERR_INVALID, "hp_redact_regions: null pointer or negative count");
    HP_REQUIRE(what == HP_REDACT_HEAD || what == HP_REDACT_BODY, HP_ERR_INVALID, "hp_redact_regions: unknown `what` %d (HP_REDACT_HEAD or HP_REDACT_BODY)", what);
    HP_REQUIRE(margin_ok(margin), HP_ERR_INVALID, "hp_redact_regions: margin %g is outside (0, 8]", (double)margin);
    return build_regions(humans, n, w, h, what, margin, out, cap);
}

int hp_redact_u8c3(hp_redact* r, uint8_t* dev_bgr, int w, int h, int stride, const hp_redact_region* regions, int n, int effect, int cell, void* stream)
{
    HP_REQUIRE(r, HP_ERR_INVALID, "hp_redact_u8c3: null handle");
    frame f;
    HP_TRY(frame_bgr(f, "hp_redact_u8c3", dev_bgr, w, h, stride, regions, n, effect, cell));
    return redact_device(r, "hp_redact_u8c3", "BGR", f, regions, n, effect, cell, (hipStream_t)stream);
}

int hp_redact_yuv(hp_redact* r, const hp_yuv_image* image, const hp_redact_region* regions, int n, int effect, int cell, void* stream)
{
    HP_REQUIRE(r, HP_ERR_INVALID, "hp_redact_yuv: null handle");
    frame f;
    const char* name = "";
    HP_TRY(frame_yuv(f, name, "hp_redact_yuv", image, true, regions, n, effect, cell));
    return redact_device(r, "hp_redact_yuv", name, f, regions, n, effect, cell, (hipStream_t)stream);
}

int hp_redact_u8c3_host(uint8_t* bgr, int w, int h, int stride, const hp_redact_region* regions, int n, int effect, int cell)
{
    frame f;
    HP_TRY(frame_bgr(f, "hp_redact_u8c3_host", bgr, w, h, stride, regions, n, effect, cell));
    paint_host(f, regions, n, effect, cell);
    return HP_OK;
}

int hp_redact_yuv_host(const hp_yuv_image* image, const hp_redact_region* regions, int n, int effect, int cell)
{
    frame f;
    const char* name = "";
    HP_TRY(frame_yuv(f, name, "hp_redact_yuv_host", image, false, regions, n, effect, cell));
    paint_host(f, regions, n, effect, cell);
    return HP_OK;
}

} // extern "C"
