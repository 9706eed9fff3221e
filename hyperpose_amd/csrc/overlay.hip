// overlay.hip — hp_overlay_*: the skeletons of a frame's humans painted straight into a device-resident frame, 8-bit BGR or any hp_yuv_image
// layout in the frame's own colour space and bit depth, optionally blended (include/hp_hip.h).  The output-side counterpart of
// resize_yuv_formats.hip: the last stage of the reference's stream, draw_human + writer (src/stream.cpp:114-147), without the frame ever
// leaving the device.  WHAT is painted is stated once, in overlay.hpp (exact integer rules); this file holds the primitive list (host),
// the kernels, the host twins (the same rules in plain C++ on host frames) and the C ABI.
//
// Kernels.  One thread owns one chroma block of pixels - 1 x 1 (BGR, I444), 2 x 1 (4:2:2) or 2 x 2 (4:2:0) - and with it every byte of the
// frame that block owns (its luma samples and its U and V sample), so every byte has exactly one writer and there are no atomics.  One block
// of 256 threads (four wavefronts) owns a tile of 32 x 8 chroma blocks; the grid covers only the bounding rectangle of the primitive list,
// clipped to the frame (no humans, or nothing inside the frame: no launch).  Each block walks the list 256 primitives at a time: a thread tests
// one primitive's reach (overlay.hpp) against the tile, the survivors are compacted IN ORDER into an LDS list (wave64 __ballot + prefix count
// over the four wavefronts' totals), and when the next 256 would not fit the list is painted first and restarted - a tile that more
// primitives touch than the list holds is processed in chunks in list order, never truncated; "later chunk wins" is painter's order because
// every thread carries the winning colour of its pixels across chunks in registers.  Painting = every thread runs the LDS list front to back
// (all lanes read the same entry: a broadcast) and keeps the last colour that covers each of its pixels, and the last that covers any of
// them for the chroma sample.  Only after the whole list does a thread touch the frame, and only the samples that were covered; a block whose
// list stayed empty never touches it.
// Variants follow the front end's split (resize_yuv_formats.hip): what changes the instructions of a store is a template parameter,
// everything else (addresses, strides, chroma shifts) is uniform and travels in the kernel arguments:
//     overlay_bgr_kernel        3 bytes per pixel
//     overlay_planar8_kernel    one byte per sample, luma at byte x            NV12 I420 NV16 I422 I444
//     overlay_packed8_kernel    one byte per sample, luma at byte 2x (+1)      YUY2 UYVY
//     overlay_word16_kernel     16-bit words, value << shift                   P010 (6) I010 (0)
// Launch: grid = (ceil(rect width in chroma blocks / 32), ceil(rect height in chroma blocks / 8)), 256 threads.  LDS: 256 entries of 32 bytes
// + 4 wavefront counts = 8208 bytes.  -Rpass-analysis=kernel-resource-usage (gfx950, the flags of hyperpose_amd/build.py):
//     kernel                    VGPRs  SGPRs  scratch  LDS bytes  waves / SIMD
//     overlay_bgr_kernel           29     64        0       8208             8
//     overlay_planar8_kernel       38     94        0       8208             8
//     overlay_packed8_kernel       33     88        0       8208             8
//     overlay_word16_kernel        38     94        0       8208             8
//
// The list reaches the device through the handle (hp_overlay): an hp::staged_ring (annotate.hpp), SLOTS pinned staging buffers and as many
// device lists, used in turn.  A call takes the next slot, builds the list in its pinned buffer, enqueues one hipMemcpyAsync and the kernel on
// the caller's stream and commits the slot; it waits (on the host) only if that slot's use SLOTS calls ago has not finished.  Where a part lies
// (part_points.hpp), the frame checks (annotate.hpp) and the bytewise host sample access (yuv_formats.hpp) are shared with redact.hip.
#include "annotate.hpp"
#include "overlay.hpp"
#include "tonemap.hpp"
#include "yuv_colour.hpp"
#include "yuv_formats.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace {

using namespace hp_ovl;

constexpr int TILE_W = 32, TILE_H = 8, THREADS = TILE_W * TILE_H, LIST_CAP = 256;

// ---- host: primitive list and colour tables -------------------------------------------------------------------------------------------

int build_primitives(const hp_human* humans, int n, int w, int h, int thickness, hp_overlay_prim* out, int cap)
{
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const hp_human& hm = humans[i];
        int t = thickness;
        if (t <= 0) { // over the PRESENT parts, whether or not their pixel is in range
            float nn = 1, s = 0, ww = 1, e = 0;
            for (const auto& p : hm.parts)
                if (hp_pts::present(p))
                    nn = std::min(nn, p.y), s = std::max(s, p.y), ww = std::min(ww, p.x), e = std::max(e, p.x);
            const float area = (e - ww) * (s - nn);
            float root = std::sqrt(area * (float)(w * h));
            if (!(root < 32.f * MAX_T))
                root = 32.f * MAX_T;
            t = std::max(1, (int)root / 32);
        }
        int32_t px[HP_COCO_N_PARTS], py[HP_COCO_N_PARTS];
        bool ok[HP_COCO_N_PARTS];
        hp_pts::part_points(hm, w, h, px, py, ok);
        auto emit = [&](int kind, int a, int b, int colour) {
            if (count < cap)
                out[count] = hp_overlay_prim{ kind, px[a], py[a], px[b], py[b], t, colour, i };
            ++count;
        };
        for (int k = 0; k < HP_COCO_N_PAIRS; ++k)
            if (ok[COCO_PAIRS[k][0]] && ok[COCO_PAIRS[k][1]])
                emit(KIND_CAPSULE, COCO_PAIRS[k][0], COCO_PAIRS[k][1], k);
        for (int k = 0; k < HP_COCO_N_PARTS; ++k)
            if (ok[k])
                emit(KIND_DISC, k, k, k);
    }
    return count;
}

int yuv_colours(int matrix, int range, int depth, int32_t out[19][3])
{
    for (int i = 0; i < 19; ++i) // the formulas: yuv_colour.hpp
        hp_yuv::colour_of(COCO_COLOURS_RGB[i][0], COCO_COLOURS_RGB[i][1], COCO_COLOURS_RGB[i][2], matrix, range, depth, out[i]);
    return HP_OK;
}

void bgr_colours(int32_t out[19][3])
{
    for (int i = 0; i < 19; ++i)
        out[i][0] = COCO_COLOURS_RGB[i][2], out[i][1] = COCO_COLOURS_RGB[i][1], out[i][2] = COCO_COLOURS_RGB[i][0];
}

// the rectangle of the frame the list can touch: false when there is none
bool list_rect(const hp_overlay_prim* prims, int n, int w, int h, int& x0, int& y0, int& x1, int& y1)
{
    x0 = w, y0 = h, x1 = -1, y1 = -1;
    for (int i = 0; i < n; ++i) {
        int lx, ly, hx, hy;
        reach(prims[i].x0, prims[i].y0, prims[i].x1, prims[i].y1, prims[i].t, lx, ly, hx, hy);
        if (hx < 0 || hy < 0 || lx >= w || ly >= h)
            continue;
        x0 = std::min(x0, std::max(lx, 0)), y0 = std::min(y0, std::max(ly, 0));
        x1 = std::max(x1, std::min(hx, w - 1)), y1 = std::max(y1, std::min(hy, h - 1));
    }
    return x1 >= x0 && y1 >= y0;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------

struct ovl_geom {
    const hp_overlay_prim* prims; // `colour` holds the three samples, 10 bits each (first sample in the low bits)
    int n_prims;
    int w, h;     // frame, pixels
    int bx0, by0; // first chroma block of the grid
    int bx1, by1; // last chroma block of the list's rectangle (inclusive)
    int sx, sy;   // a chroma block is (1 << sx) x (1 << sy) pixels
    int weight;   // 0 .. 256 (overlay.hpp)
};

__device__ __forceinline__ int mix(int c, int old, int w) { return blend(c, old, w); }

struct bgr_target {
    uint8_t* p;
    int stride;
    __device__ __forceinline__ void write(int bx, int by, const int (&col)[1][1], int, int w) const
    {
        if (col[0][0] < 0)
            return;
        uint8_t* q = p + (size_t)by * stride + (size_t)bx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int v = (col[0][0] >> (10 * c)) & 1023;
            q[c] = (uint8_t)(w == 256 ? v : mix(v, q[c], w));
        }
    }
};

template <int SAMPLE_BYTES, int Y_STEP, int PY> struct yuv_target {
    uint8_t *y, *u, *v;
    int y_stride, c_stride, v_extra, c_step;
    int sx, sy, shift;
    __device__ __forceinline__ void put(uint8_t* q, int c, int w) const
    {
        if constexpr (SAMPLE_BYTES == 2) {
            uint16_t* s = reinterpret_cast<uint16_t*>(q);
            *s = (uint16_t)((w == 256 ? c : mix(c, (*s >> shift) & 1023, w)) << shift);
        } else
            *q = (uint8_t)(w == 256 ? c : mix(c, *q, w));
    }
    __device__ __forceinline__ void write(int bx, int by, const int (&col)[PY][2], int ccol, int w) const
    {
#pragma unroll
        for (int dy = 0; dy < PY; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
                if (col[dy][dx] >= 0)
                    put(y + (size_t)((by << sy) + dy) * y_stride + (size_t)((bx << sx) + dx) * (Y_STEP * SAMPLE_BYTES), col[dy][dx] & 1023, w);
        if (ccol >= 0) {
            const size_t at = (size_t)by * c_stride + (size_t)bx * c_step;
            put(u + at, (ccol >> 10) & 1023, w);
            put(v + at + (ptrdiff_t)by * v_extra, (ccol >> 20) & 1023, w);
        }
    }
};

template <int PX, int PY, class Target> __device__ __forceinline__ void overlay_body(const ovl_geom& g, const Target& t)
{
    __shared__ hp_overlay_prim list[LIST_CAP];
    __shared__ int wave_count[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tbx = g.bx0 + blockIdx.x * TILE_W, tby = g.by0 + blockIdx.y * TILE_H;
    const int bx = tbx + (tid & (TILE_W - 1)), by = tby + tid / TILE_W;
    // the tile in pixels (inclusive), clipped to the list's rectangle: what a primitive must reach to be kept
    const int tx0 = tbx << g.sx, ty0 = tby << g.sy;
    const int tx1 = ((min(tbx + TILE_W - 1, g.bx1) + 1) << g.sx) - 1, ty1 = ((min(tby + TILE_H - 1, g.by1) + 1) << g.sy) - 1;
    const bool inside = bx <= g.bx1 && by <= g.by1;
    const int x = bx << g.sx, y = by << g.sy; // this thread's first pixel; its block spans nx x ny
    const int nx = PX == 1 ? 1 : 1 << g.sx, ny = PY == 1 ? 1 : 1 << g.sy;

    int col[PY][PX], ccol = -1;
#pragma unroll
    for (int dy = 0; dy < PY; ++dy)
#pragma unroll
        for (int dx = 0; dx < PX; ++dx)
            col[dy][dx] = -1;

    auto paint = [&](int count) {
        if (!inside)
            return;
        for (int k = 0; k < count; ++k) {
            const hp_overlay_prim p = list[k];
            int lx, ly, hx, hy;
            reach(p.x0, p.y0, p.x1, p.y1, p.t, lx, ly, hx, hy);
            if (hx < x || hy < y || lx > x + nx - 1 || ly > y + ny - 1)
                continue;
#pragma unroll
            for (int dy = 0; dy < PY; ++dy)
#pragma unroll
                for (int dx = 0; dx < PX; ++dx)
                    if (dx < nx && dy < ny && covers(p.kind, p.x0, p.y0, p.x1, p.y1, p.t, x + dx, y + dy))
                        col[dy][dx] = p.colour, ccol = p.colour;
        }
    };

    int fill = 0; // entries in the LDS list (uniform)
    for (int base = 0; base < g.n_prims; base += THREADS) {
        const int i = base + tid;
        hp_overlay_prim p = {};
        bool keep = false;
        if (i < g.n_prims) {
            p = g.prims[i];
            int lx, ly, hx, hy;
            reach(p.x0, p.y0, p.x1, p.y1, p.t, lx, ly, hx, hy);
            keep = hx >= tx0 && hy >= ty0 && lx <= tx1 && ly <= ty1;
        }
        const unsigned long long kept = __ballot(keep);
        if (lane == 0)
            wave_count[wave] = __popcll(kept);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < THREADS / 64; ++k) {
            const int c = wave_count[k];
            before += k < wave ? c : 0;
            total += c;
        }
        if (fill + total > LIST_CAP) { // paint what is there, in order, then start the list again: total <= THREADS = LIST_CAP always fits
            paint(fill);
            fill = 0;
            __syncthreads();
        }
        if (keep)
            list[fill + before + __popcll(kept & ((1ull << lane) - 1))] = p;
        fill += total;
        __syncthreads();
    }
    paint(fill);
    if (inside)
        t.write(bx, by, col, ccol, g.weight);
}

__global__ __launch_bounds__(THREADS) void overlay_bgr_kernel(const ovl_geom g, const bgr_target t) { overlay_body<1, 1>(g, t); }
__global__ __launch_bounds__(THREADS) void overlay_planar8_kernel(const ovl_geom g, const yuv_target<1, 1, 2> t) { overlay_body<2, 2>(g, t); }
__global__ __launch_bounds__(THREADS) void overlay_packed8_kernel(const ovl_geom g, const yuv_target<1, 2, 1> t) { overlay_body<2, 1>(g, t); }
__global__ __launch_bounds__(THREADS) void overlay_word16_kernel(const ovl_geom g, const yuv_target<2, 1, 2> t) { overlay_body<2, 2>(g, t); }

} // namespace

// ---- the handle ---------------------------------------------------------------------------------------------------------------------------

struct hp_overlay {
    int max_humans = 0, cap = 0; // cap = max_humans * PRIMS_PER_HUMAN primitives per list
    hp::staged_ring ring;        // cap hp_overlay_prim per slot
    bool hdr = false;       // hp_overlay_set_transfer: 10-bit frames are PQ / HLG and take hp_yuv_colours_hdr's table
    hp_hdr_desc transfer {};
};

namespace {

// ---- the frame a call paints, as both the device and the host path see it -------------------------------------------------------------

struct frame_desc {
    bool bgr = true;
    const char* name = "BGR";
    int w = 0, h = 0, sx = 0, sy = 0;
    int sample_bytes = 1, shift = 0, planes = 1;
    uint8_t* base = nullptr; // BGR
    int stride = 0;
    hp_yuv::sample_map map {};
    int32_t colours[19][3];
};

int check_common(const char* who, const char* name, int w, int h, const hp_human* humans, int n, float opacity, int thickness)
{
    HP_TRY(hp::check_max_dim(who, name, w, h));
    HP_REQUIRE(opacity > 0.f && opacity <= 1.f, HP_ERR_INVALID, "%s: %s: opacity %g is outside (0, 1]", who, name, (double)opacity);
    HP_REQUIRE(n >= 0 && (n == 0 || humans), HP_ERR_INVALID, "%s: %s: %d humans at a null pointer or a negative count", who, name, n);
    HP_REQUIRE(thickness <= MAX_T, HP_ERR_INVALID, "%s: %s: thickness %d is beyond %d", who, name, thickness, MAX_T);
    return HP_OK;
}

int describe_bgr(frame_desc& f, const char* who, uint8_t* bgr, int w, int h, int stride, const hp_human* humans, int n, float opacity, int thickness)
{
    HP_TRY(hp::check_bgr_frame(who, bgr, w, h, stride));
    HP_TRY(check_common(who, "BGR", w, h, humans, n, opacity, thickness));
    f.bgr = true, f.w = w, f.h = h, f.base = bgr, f.stride = stride;
    bgr_colours(f.colours);
    return HP_OK;
}

int describe_yuv(frame_desc& f, const char* who, const hp_yuv_image* im, bool kernel_access, const hp_human* humans, int n, float opacity, int thickness,
    const hp_hdr_desc* transfer = nullptr)
{
    HP_TRY(hp_yuv::validate(im, who, kernel_access));
    const hp_yuv::layout& l = *hp_yuv::layout_of(im->format);
    HP_TRY(check_common(who, l.name, im->width, im->height, humans, n, opacity, thickness));
    f.bgr = false, f.name = l.name, f.w = im->width, f.h = im->height, f.sx = l.sx, f.sy = l.sy;
    f.sample_bytes = l.sample_bytes, f.shift = l.shift, f.planes = l.planes;
    f.map = hp_yuv::map_samples(*im, l);
    if (transfer && l.sample_bytes == 2) // an HDR frame: graphics white at white_nits instead of full-scale code values
        return hp_yuv_colours_hdr(im->matrix, im->range, transfer, f.colours);
    return yuv_colours(im->matrix, im->range, l.sample_bytes == 2 ? 10 : 8, f.colours);
}

int weight_of(float opacity) { return (int)std::nearbyint((double)opacity * 256.); }

int pack_colour(const int32_t c[3]) { return c[0] | (c[1] << 10) | (c[2] << 20); }

template <class Target> void fill_target(Target& t, const frame_desc& f)
{
    t.y = const_cast<uint8_t*>(f.map.y), t.u = const_cast<uint8_t*>(f.map.u), t.v = const_cast<uint8_t*>(f.map.v);
    t.y_stride = f.map.y_stride, t.c_stride = f.map.c_stride, t.v_extra = f.map.v_extra, t.c_step = f.map.c_step;
    t.sx = f.sx, t.sy = f.sy, t.shift = f.shift;
}

int draw_device(hp_overlay* o, const char* who, const frame_desc& f, const hp_human* humans, int n, float opacity, int thickness, hipStream_t s)
{
    HP_REQUIRE(n <= o->max_humans, HP_ERR_INVALID, "%s: %s: %d humans, the handle was created for %d", who, f.name, n, o->max_humans);
    if (n == 0)
        return HP_OK;
    hp_overlay_prim* prims; // built in the slot's pinned buffer: the slot is taken before there is a list
    HP_TRY(o->ring.take(prims));
    const int count = build_primitives(humans, n, f.w, f.h, thickness, prims, o->cap);
    int x0, y0, x1, y1;
    if (count == 0 || !list_rect(prims, count, f.w, f.h, x0, y0, x1, y1))
        return HP_OK;
    for (int i = 0; i < count; ++i)
        prims[i].colour = pack_colour(f.colours[prims[i].colour]);
    HP_TRY(o->ring.upload((size_t)count * sizeof(hp_overlay_prim), s));
    ovl_geom g;
    g.prims = o->ring.device<hp_overlay_prim>(), g.n_prims = count, g.w = f.w, g.h = f.h, g.sx = f.sx, g.sy = f.sy;
    g.bx0 = x0 >> f.sx, g.by0 = y0 >> f.sy, g.bx1 = x1 >> f.sx, g.by1 = y1 >> f.sy;
    g.weight = weight_of(opacity);
    const dim3 grid(hp::ceil_div(g.bx1 - g.bx0 + 1, TILE_W), hp::ceil_div(g.by1 - g.by0 + 1, TILE_H));
    if (f.bgr) {
        bgr_target t { f.base, f.stride };
        hipLaunchKernelGGL(overlay_bgr_kernel, grid, dim3(THREADS), 0, s, g, t);
    } else if (f.sample_bytes == 2) {
        yuv_target<2, 1, 2> t;
        fill_target(t, f);
        hipLaunchKernelGGL(overlay_word16_kernel, grid, dim3(THREADS), 0, s, g, t);
    } else if (f.planes == 1) {
        yuv_target<1, 2, 1> t;
        fill_target(t, f);
        hipLaunchKernelGGL(overlay_packed8_kernel, grid, dim3(THREADS), 0, s, g, t);
    } else {
        yuv_target<1, 1, 2> t;
        fill_target(t, f);
        hipLaunchKernelGGL(overlay_planar8_kernel, grid, dim3(THREADS), 0, s, g, t);
    }
    return o->ring.commit(s);
}

// ---- host twin: the rules of overlay.hpp on a frame in host memory -------------------------------------------------------------------------

void host_put(const frame_desc& f, uint8_t* q, int c, int w)
{
    hp_yuv::host_put(q, f.sample_bytes, f.shift, w == 256 ? c : blend(c, hp_yuv::host_get(q, f.sample_bytes, f.shift), w));
}

int draw_host(const frame_desc& f, const hp_human* humans, int n, float opacity, int thickness)
{
    if (n == 0)
        return HP_OK;
    std::vector<hp_overlay_prim> prims((size_t)n * PRIMS_PER_HUMAN);
    const int count = build_primitives(humans, n, f.w, f.h, thickness, prims.data(), (int)prims.size());
    int x0, y0, x1, y1;
    if (count == 0 || !list_rect(prims.data(), count, f.w, f.h, x0, y0, x1, y1))
        return HP_OK;
    const int nx = 1 << f.sx, ny = 1 << f.sy, w = weight_of(opacity);
    x0 &= ~(nx - 1), y0 &= ~(ny - 1), x1 |= nx - 1, y1 |= ny - 1; // whole chroma blocks (the frame's size is a multiple of them)
    const int rw = x1 - x0 + 1, rh = y1 - y0 + 1;
    std::vector<int32_t> last((size_t)rw * rh, -1); // index of the last primitive that covers the pixel
    for (int k = 0; k < count; ++k) {
        const hp_overlay_prim& p = prims[k];
        int lx, ly, hx, hy;
        reach(p.x0, p.y0, p.x1, p.y1, p.t, lx, ly, hx, hy);
        for (int y = std::max(ly, y0); y <= std::min(hy, y1); ++y)
            for (int x = std::max(lx, x0); x <= std::min(hx, x1); ++x)
                if (covers(p.kind, p.x0, p.y0, p.x1, p.y1, p.t, x, y))
                    last[(size_t)(y - y0) * rw + (x - x0)] = k;
    }
    for (int y = y0; y <= y1; y += ny)
        for (int x = x0; x <= x1; x += nx) {
            int best = -1;
            for (int dy = 0; dy < ny; ++dy)
                for (int dx = 0; dx < nx; ++dx) {
                    const int k = last[(size_t)(y + dy - y0) * rw + (x + dx - x0)];
                    if (k < 0)
                        continue;
                    best = std::max(best, k);
                    const int32_t* c = f.colours[prims[k].colour];
                    if (f.bgr) {
                        uint8_t* q = f.base + (size_t)(y + dy) * f.stride + (size_t)(x + dx) * 3;
                        for (int ch = 0; ch < 3; ++ch)
                            host_put(f, q + ch, c[ch], w);
                    } else
                        host_put(f, const_cast<uint8_t*>(f.map.y) + (size_t)(y + dy) * f.map.y_stride + (size_t)(x + dx) * f.map.y_step, c[0], w);
                }
            if (best < 0 || f.bgr)
                continue;
            const int32_t* c = f.colours[prims[best].colour];
            const int cy = y >> f.sy;
            const size_t at = (size_t)cy * f.map.c_stride + (size_t)(x >> f.sx) * f.map.c_step;
            host_put(f, const_cast<uint8_t*>(f.map.u) + at, c[1], w);
            host_put(f, const_cast<uint8_t*>(f.map.v) + at + (ptrdiff_t)cy * f.map.v_extra, c[2], w);
        }
    return HP_OK;
}

} // namespace

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------

extern "C" {

int hp_overlay_create(hp_overlay** out, int max_humans)
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_overlay_create: null output");
    *out = nullptr;
    HP_REQUIRE(max_humans > 0 && max_humans <= (1 << 16), HP_ERR_INVALID, "hp_overlay_create: max_humans %d (1 .. 65536)", max_humans);
    std::unique_ptr<hp_overlay> o(new hp_overlay); // a failed create frees what it allocated
    o->max_humans = max_humans, o->cap = max_humans * PRIMS_PER_HUMAN;
    HP_TRY(o->ring.alloc((size_t)o->cap * sizeof(hp_overlay_prim), "hp_overlay_create"));
    *out = o.release();
    return HP_OK;
}

void hp_overlay_destroy(hp_overlay* o) { delete o; } // the ring drains first

int hp_overlay_primitives(const hp_human* humans, int n, int w, int h, int thickness, hp_overlay_prim* out, int cap)
{
    HP_REQUIRE(w > 0 && h > 0 && w <= MAX_DIM && h <= MAX_DIM, HP_ERR_INVALID, "hp_overlay_primitives: frame %d x %d (1 .. %d)", w, h, MAX_DIM);
    HP_REQUIRE(n >= 0 && (n == 0 || humans) && cap >= 0 && (cap == 0 || out), HP_ERR_INVALID, "hp_overlay_primitives: null pointer or negative count");
    HP_REQUIRE(thickness <= MAX_T, HP_ERR_INVALID, "hp_overlay_primitives: thickness %d is beyond %d", thickness, MAX_T);
    return build_primitives(humans, n, w, h, thickness, out, cap);
}

int hp_yuv_colours(int matrix, int range, int depth, int32_t out[19][3])
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_yuv_colours: null output");
    HP_REQUIRE(matrix >= HP_YUV_BT601 && matrix <= HP_YUV_BT2020, HP_ERR_INVALID, "hp_yuv_colours: unknown matrix %d", matrix);
    HP_REQUIRE(range == HP_YUV_LIMITED || range == HP_YUV_FULL, HP_ERR_INVALID, "hp_yuv_colours: unknown range %d", range);
    HP_REQUIRE(depth == 8 || depth == 10, HP_ERR_INVALID, "hp_yuv_colours: depth %d (8 or 10)", depth);
    return yuv_colours(matrix, range, depth, out);
}

int hp_overlay_draw_u8c3(hp_overlay* o, uint8_t* dev_bgr, int w, int h, int stride, const hp_human* humans, int n, float opacity, int thickness, void* stream)
{
    HP_REQUIRE(o, HP_ERR_INVALID, "hp_overlay_draw_u8c3: null handle");
    frame_desc f;
    HP_TRY(describe_bgr(f, "hp_overlay_draw_u8c3", dev_bgr, w, h, stride, humans, n, opacity, thickness));
    return draw_device(o, "hp_overlay_draw_u8c3", f, humans, n, opacity, thickness, (hipStream_t)stream);
}

int hp_overlay_draw_yuv(hp_overlay* o, const hp_yuv_image* frame, const hp_human* humans, int n, float opacity, int thickness, void* stream)
{
    HP_REQUIRE(o, HP_ERR_INVALID, "hp_overlay_draw_yuv: null handle");
    frame_desc f;
    HP_TRY(describe_yuv(f, "hp_overlay_draw_yuv", frame, true, humans, n, opacity, thickness, o->hdr ? &o->transfer : nullptr));
    return draw_device(o, "hp_overlay_draw_yuv", f, humans, n, opacity, thickness, (hipStream_t)stream);
}

int hp_overlay_draw_u8c3_host(uint8_t* bgr, int w, int h, int stride, const hp_human* humans, int n, float opacity, int thickness)
{
    frame_desc f;
    HP_TRY(describe_bgr(f, "hp_overlay_draw_u8c3_host", bgr, w, h, stride, humans, n, opacity, thickness));
    return draw_host(f, humans, n, opacity, thickness);
}

int hp_overlay_draw_yuv_host(const hp_yuv_image* frame, const hp_human* humans, int n, float opacity, int thickness)
{
    frame_desc f;
    HP_TRY(describe_yuv(f, "hp_overlay_draw_yuv_host", frame, false, humans, n, opacity, thickness));
    return draw_host(f, humans, n, opacity, thickness);
}

int hp_overlay_set_transfer(hp_overlay* o, const hp_hdr_desc* d)
{
    HP_REQUIRE(o, HP_ERR_INVALID, "hp_overlay_set_transfer: null handle");
    if (d)
        HP_TRY(hp_hdr::check_desc(d, "hp_overlay_set_transfer"));
    o->hdr = d != nullptr;
    if (d)
        o->transfer = *d;
    return HP_OK;
}

int hp_overlay_draw_yuv_host_hdr(const hp_yuv_image* frame, const hp_hdr_desc* d, const hp_human* humans, int n, float opacity, int thickness)
{
    frame_desc f;
    HP_TRY(describe_yuv(f, "hp_overlay_draw_yuv_host_hdr", frame, false, humans, n, opacity, thickness, d));
    return draw_host(f, humans, n, opacity, thickness);
}

} // extern "C"
