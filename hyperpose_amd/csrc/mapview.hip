// mapview.hip — hp_mapview_*: a colour-mapped, up-sampled view of the network's own maps blended straight into a device-resident frame, 8-bit BGR or
// any hp_yuv_image layout in the frame's own matrix, range and bit depth (include/hp_hip.h).  The third annotator after overlay.hip and redact.hip
// and the dense one: it reads and rewrites every sample of the region, so it is bound by memory, not by launches.  WHAT is painted is stated once,
// in mapview.hpp (the index plane in fp32, host taps, exact integer rules after them, the host painter included); this file holds the two kernels,
// the handle and the C ABI.
//
// Kernels.  Two launches per call, on the caller's stream.
//   reduce   one thread per map cell: the channel choice of the frame's maps -> one byte of the index plane (hp_mv::index_of), written into the ring
//            slot's device buffer.  The plane is a few KB and stays in cache for the painter.
//   paint    one thread owns a horizontal RUN = 4 of chroma blocks - 1 x 1 (BGR, I444), 2 x 1 (4:2:2) or 2 x 2 (4:2:0) pixels each - and with it every
//            byte of the frame those blocks own, so every byte has one writer.  Runs are anchored at the frame's column 0, so a run's samples start at
//            a multiple of 8, 12 or 16 bytes from the row's first byte.  A run that lies whole inside the roi and whose row segment starts on a dword
//            is read, blended and written as whole words (one dwordx4 or dwordx2 where the address allows, else dwords): 12 bytes per lane on BGR, 8
//            per luma row and 8 (UV pairs) or 4 + 4 per chroma row on the 8-bit planes, 16 per row on the 16-bit planes and on packed 4:2:2.  Any
//            other run - the roi's unaligned head and tail, a row whose pitch puts it off a dword - goes sample by sample and touches only samples
//            inside the roi with a weight above 0.  A block of 256 threads covers 64 runs x 4 block rows; the palette (256 entries of 8 bytes: three
//            10-bit samples and the weight) is copied to LDS once per block; the tap tables and the index plane are read through the cache.
// Variants follow overlay.hip's split: what changes the instructions of a store is a template parameter, everything else is uniform and travels
// in the kernel arguments.  -Rpass-analysis=kernel-resource-usage (gfx950, the flags of hyperpose_amd/build.py): DESIGN.md 1.1 "Map view".
//     mapview_bgr_kernel                    3 bytes per pixel
//     mapview_planar8_kernel<PX, PY>        one byte per sample      NV12 I420 <2, 2>   NV16 I422 <2, 1>   I444 <1, 1>
//     mapview_word16_kernel                 16-bit words, << shift   P010 (6) I010 (0)
//     mapview_packed8_kernel                Y0 U Y1 V / U Y0 V Y1    YUY2 UYVY
//
// The handle (hp_mapview) holds one hp::staged_ring (annotate.hpp); a slot carries the palette entries, the x table, the y table (uploaded by one
// hipMemcpyAsync) and the index plane (device only).  The tap tables of the last (pixels, cells, cover) per axis are kept, so a stream of frames of
// one size computes them once.  A call enqueues the copy, the two launches and the slot's event; it waits on the host only for the slot's use
// SLOTS calls ago.
#include "annotate.hpp"
#include "mapview.hpp"

#include <cmath>
#include <memory>
#include <vector>

namespace {

using namespace hp_mv;

constexpr int RUN = 4, RUNS_X = 64, ROWS_Y = 4, THREADS = RUNS_X * ROWS_Y;
static_assert(THREADS == 256, "one thread copies one palette entry to LDS");
constexpr size_t OFF_TABS = 256 * sizeof(entry), OFF_PLANE = OFF_TABS + 2 * (size_t)MAX_DIM * sizeof(uint32_t);

// ---- reduce -----------------------------------------------------------------------------------------------------------------------------------

struct mv_reduce {
    const float* maps; // the frame's [C][cells]
    uint8_t* plane;
    int cells, c0, cn, c_step, mode;
    float gain;
};

__global__ __launch_bounds__(THREADS) void mapview_reduce_kernel(const mv_reduce r)
{
    const int cell = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (cell < r.cells)
        r.plane[cell] = (uint8_t)index_of(r.maps, r.cells, cell, r.c0, r.cn, r.c_step, r.mode, r.gain);
}

// ---- paint ------------------------------------------------------------------------------------------------------------------------------------

struct mv_grid {
    int run0, by0;    // first run of RUN chroma blocks (counted from the frame's column 0) and first block row of the roi
    int runs, brows;  // how many of each the roi touches
};

template <int WORDS> __device__ __forceinline__ void load_words(const uint8_t* p, uint32_t (&v)[WORDS])
{
    const uintptr_t a = (uintptr_t)p;
    if constexpr (WORDS == 4) {
        if ((a & 15) == 0) {
            const uint4 t = *reinterpret_cast<const uint4*>(p);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
            return;
        }
    }
    if constexpr (WORDS % 2 == 0) {
        if ((a & 7) == 0) {
#pragma unroll
            for (int k = 0; k < WORDS; k += 2) {
                const uint2 t = reinterpret_cast<const uint2*>(p)[k / 2];
                v[k] = t.x, v[k + 1] = t.y;
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < WORDS; ++k)
        v[k] = reinterpret_cast<const uint32_t*>(p)[k];
}

template <int WORDS> __device__ __forceinline__ void store_words(uint8_t* p, const uint32_t (&v)[WORDS])
{
    const uintptr_t a = (uintptr_t)p;
    if constexpr (WORDS == 4) {
        if ((a & 15) == 0) {
            *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
            return;
        }
    }
    if constexpr (WORDS % 2 == 0) {
        if ((a & 7) == 0) {
#pragma unroll
            for (int k = 0; k < WORDS; k += 2)
                reinterpret_cast<uint2*>(p)[k / 2] = make_uint2(v[k], v[k + 1]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < WORDS; ++k)
        reinterpret_cast<uint32_t*>(p)[k] = v[k];
}

// N samples of SB bytes each, contiguous from p: sample s becomes the blend of c[s] at weight w[s]; weight 0 keeps it.  `whole`: every sample belongs
// to the roi, so the segment may be read and written as words; otherwise only the samples with a weight are touched.
template <int SB, int N> __device__ __forceinline__ void put_segment(uint8_t* p, const int (&c)[N], const int (&w)[N], bool whole, int shift)
{
    constexpr int WORDS = N * SB / 4, PER = 4 / SB, BITS = 8 * SB;
    static_assert(N * SB % 4 == 0, "a run's segment is whole dwords");
    if (whole && ((uintptr_t)p & 3) == 0) {
        uint32_t word[WORDS];
        load_words<WORDS>(p, word);
#pragma unroll
        for (int k = 0; k < WORDS; ++k) {
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int s = k * PER + j;
                const uint32_t raw = (word[k] >> (BITS * j)) & ((1u << BITS) - 1u);
                uint32_t nv = raw;
                if (w[s] > 0)
                    nv = SB == 2 ? (uint32_t)blend(c[s], (int)((raw >> shift) & 1023u), w[s]) << shift : (uint32_t)blend(c[s], (int)raw, w[s]);
                out |= nv << (BITS * j);
            }
            word[k] = out;
        }
        store_words<WORDS>(p, word);
        return;
    }
#pragma unroll
    for (int s = 0; s < N; ++s) {
        if (w[s] <= 0)
            continue;
        if constexpr (SB == 2) {
            uint16_t* q = reinterpret_cast<uint16_t*>(p) + s;
            *q = (uint16_t)(blend(c[s], (*q >> shift) & 1023, w[s]) << shift);
        } else
            p[s] = (uint8_t)blend(c[s], p[s], w[s]);
    }
}

// the palette entry of a pixel's index; a pixel outside the roi (q < 0) has weight 0
__device__ __forceinline__ entry look(const entry* pal, int q)
{
    entry e = pal[q < 0 ? 0 : q];
    e.w = q < 0 ? 0u : e.w;
    return e;
}

struct bgr_writer {
    uint8_t* p;
    int stride;
    __device__ __forceinline__ void write(const entry* pal, int bx, int by, const int (&q)[1][RUN], bool whole) const
    {
        int c[RUN * 3], w[RUN * 3];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            const entry e = look(pal, q[0][i]);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                c[3 * i + ch] = (int)((e.c >> (10 * ch)) & 1023u), w[3 * i + ch] = (int)e.w;
        }
        put_segment<1, RUN * 3>(p + (size_t)by * stride + (size_t)bx * 3, c, w, whole, 0);
    }
};

// the largest index among the pixels of chroma block i of the run
template <int PX, int PY> __device__ __forceinline__ int block_index(const int (&q)[PY][RUN * PX], int i)
{
    int best = -1;
#pragma unroll
    for (int dy = 0; dy < PY; ++dy)
#pragma unroll
        for (int dx = 0; dx < PX; ++dx)
            best = max(best, q[dy][i * PX + dx]);
    return best;
}

template <int SB, int PX, int PY> struct planar_writer {
    uint8_t *y, *u, *v;
    int y_stride, c_stride, v_extra;
    int pairs; // the chroma plane holds (U, V) pairs
    int shift;
    __device__ __forceinline__ void write(const entry* pal, int bx, int by, const int (&q)[PY][RUN * PX], bool whole) const
    {
#pragma unroll
        for (int dy = 0; dy < PY; ++dy) {
            int c[RUN * PX], w[RUN * PX];
#pragma unroll
            for (int i = 0; i < RUN * PX; ++i) {
                const entry e = look(pal, q[dy][i]);
                c[i] = (int)(e.c & 1023u), w[i] = (int)e.w;
            }
            put_segment<SB, RUN * PX>(y + (size_t)(by * PY + dy) * y_stride + (size_t)bx * (PX * SB), c, w, whole, shift);
        }
        int cu[RUN], cv[RUN], cw[RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            const entry e = look(pal, block_index<PX, PY>(q, i));
            cu[i] = (int)((e.c >> 10) & 1023u), cv[i] = (int)(e.c >> 20), cw[i] = (int)e.w;
        }
        if (pairs) {
            int c[RUN * 2], w[RUN * 2];
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                c[2 * i] = cu[i], c[2 * i + 1] = cv[i], w[2 * i] = w[2 * i + 1] = cw[i];
            put_segment<SB, RUN * 2>(u + (size_t)by * c_stride + (size_t)bx * (2 * SB), c, w, whole, shift);
        } else {
            put_segment<SB, RUN>(u + (size_t)by * c_stride + (size_t)bx * SB, cu, cw, whole, shift);
            put_segment<SB, RUN>(v + (size_t)by * c_stride + (ptrdiff_t)by * v_extra + (size_t)bx * SB, cv, cw, whole, shift);
        }
    }
};

struct packed_writer {
    uint8_t* p;   // the macropixels' first byte
    int stride;
    int luma_odd; // UYVY: the luma samples are the odd bytes
    __device__ __forceinline__ void write(const entry* pal, int bx, int by, const int (&q)[1][RUN * 2], bool whole) const
    {
        int c[RUN * 4], w[RUN * 4];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            const entry e0 = look(pal, q[0][2 * i]), e1 = look(pal, q[0][2 * i + 1]), ec = look(pal, block_index<2, 1>(q, i));
            const int y0 = (int)(e0.c & 1023u), y1 = (int)(e1.c & 1023u), cu = (int)((ec.c >> 10) & 1023u), cv = (int)(ec.c >> 20);
            c[4 * i] = luma_odd ? cu : y0, c[4 * i + 1] = luma_odd ? y0 : cu, c[4 * i + 2] = luma_odd ? cv : y1, c[4 * i + 3] = luma_odd ? y1 : cv;
            w[4 * i] = (int)(luma_odd ? ec.w : e0.w), w[4 * i + 1] = (int)(luma_odd ? e0.w : ec.w);
            w[4 * i + 2] = (int)(luma_odd ? ec.w : e1.w), w[4 * i + 3] = (int)(luma_odd ? e1.w : ec.w);
        }
        put_segment<1, RUN * 4>(p + (size_t)by * stride + (size_t)bx * 4, c, w, whole, 0);
    }
};

template <int PX, int PY, class Writer> __device__ __forceinline__ void paint_body(const view& v, const mv_grid& g, const Writer& t)
{
    __shared__ entry pal[256];
    pal[threadIdx.x] = v.pal[threadIdx.x];
    __syncthreads();
    const int rx_ = (int)blockIdx.x * RUNS_X + (int)(threadIdx.x & (RUNS_X - 1)), ry_ = (int)blockIdx.y * ROWS_Y + (int)(threadIdx.x / RUNS_X);
    if (rx_ >= g.runs || ry_ >= g.brows)
        return;
    const int bx = (g.run0 + rx_) * RUN, by = g.by0 + ry_; // this thread's first chroma block
    const int X0 = bx * PX, Y0 = by * PY, x_end = v.rx + v.rw, y_end = v.ry + v.rh;
    const bool whole = X0 >= v.rx && X0 + RUN * PX <= x_end && Y0 >= v.ry && Y0 + PY <= y_end;
    int q[PY][RUN * PX];
#pragma unroll
    for (int dy = 0; dy < PY; ++dy)
#pragma unroll
        for (int i = 0; i < RUN * PX; ++i) {
            const int x = X0 + i, y = Y0 + dy;
            q[dy][i] = -1;
            if (whole || (x >= v.rx && x < x_end && y >= v.ry && y < y_end))
                q[dy][i] = index_at(v, x, y);
        }
    t.write(pal, bx, by, q, whole);
}

__global__ __launch_bounds__(THREADS) void mapview_bgr_kernel(const view v, const mv_grid g, const bgr_writer t) { paint_body<1, 1>(v, g, t); }
template <int PX, int PY> __global__ __launch_bounds__(THREADS) void mapview_planar8_kernel(const view v, const mv_grid g, const planar_writer<1, PX, PY> t)
{
    paint_body<PX, PY>(v, g, t);
}
__global__ __launch_bounds__(THREADS) void mapview_word16_kernel(const view v, const mv_grid g, const planar_writer<2, 2, 2> t) { paint_body<2, 2>(v, g, t); }
__global__ __launch_bounds__(THREADS) void mapview_packed8_kernel(const view v, const mv_grid g, const packed_writer t) { paint_body<2, 1>(v, g, t); }

} // namespace

// ---- the handle ---------------------------------------------------------------------------------------------------------------------------

struct hp_mapview {
    int max_cells = 0;
    hp::staged_ring ring; // per slot: 256 entries, the x and the y table (uploaded), then the index plane (device only)
    struct axis {         // the table of the last (pixels, cells, cover) of one axis
        int U = 0, m = 0;
        double cover = 0;
        std::vector<uint32_t> taps;
    } x, y;
    const uint8_t* last_plane = nullptr; // hp_mapview_debug_plane
    int last_cells = 0;
};

namespace {

// ---- the arguments of a call, checked, as both the device and the host path use them -------------------------------------------------------------

struct call {
    const char* name = "BGR";
    target f {};
    const hp_yuv_image* image = nullptr; // YUV frames
    int w = 0, h = 0;
    hp_roi roi {};
    hp_orient::axes ax {};
    int nx = 0, ny = 0; // upright pixels of the roi
    int W = 0;          // nearbyint(opacity * 256)
};

int check_maps(const char* who, const char* name, const hp_mapview_desc* d)
{
    HP_REQUIRE(d, HP_ERR_INVALID, "%s: %s: null description", who, name);
    HP_REQUIRE(d->maps, HP_ERR_INVALID, "%s: %s: null maps", who, name);
    HP_REQUIRE(d->C > 0 && d->mh > 0 && d->mw > 0 && d->mh <= MAX_MAP_SIDE && d->mw <= MAX_MAP_SIDE && (int64_t)d->mh * d->mw <= MAX_MAP_CELLS, HP_ERR_INVALID,
        "%s: %s: maps of %d x %d x %d (channels x rows x columns)", who, name, d->C, d->mh, d->mw);
    HP_REQUIRE(d->frame >= 0, HP_ERR_INVALID, "%s: %s: frame %d is negative", who, name, d->frame);
    HP_REQUIRE(d->mode == HP_MAPVIEW_MAX || d->mode == HP_MAPVIEW_FIELD, HP_ERR_INVALID, "%s: %s: unknown mode %d", who, name, d->mode);
    HP_REQUIRE(d->cn >= 1, HP_ERR_INVALID, "%s: %s: cn %d is below 1", who, name, d->cn);
    HP_REQUIRE(d->c_step >= 1, HP_ERR_INVALID, "%s: %s: c_step %d is below 1", who, name, d->c_step);
    const int64_t last = (int64_t)d->c0 + (int64_t)(d->cn - 1) * d->c_step + (d->mode == HP_MAPVIEW_FIELD ? 1 : 0);
    HP_REQUIRE(d->c0 >= 0 && last < d->C, HP_ERR_INVALID, "%s: %s: channels %d .. %lld of %d", who, name, d->c0, (long long)last, d->C);
    HP_REQUIRE(std::isfinite(d->gain) && d->gain > 0.f, HP_ERR_INVALID, "%s: %s: gain %g is not a finite number above 0", who, name, (double)d->gain);
    return HP_OK;
}

int check_call(call& c, const char* who, const hp_mapview_desc* d, const int32_t (*palette)[4], float opacity)
{
    HP_TRY(hp::check_max_dim(who, c.name, c.w, c.h));
    HP_REQUIRE(opacity > 0.f && opacity <= 1.f, HP_ERR_INVALID, "%s: %s: opacity %g is outside (0, 1]", who, c.name, (double)opacity);
    HP_TRY(check_maps(who, c.name, d));
    HP_REQUIRE(d->cover_x > 0. && d->cover_x <= 1. && d->cover_y > 0. && d->cover_y <= 1., HP_ERR_INVALID, "%s: %s: cover (%g, %g) is outside (0, 1]", who, c.name,
        d->cover_x, d->cover_y);
    HP_REQUIRE(hp_orient::valid(d->orientation), HP_ERR_INVALID, "%s: %s: unknown orientation %d", who, c.name, d->orientation);
    c.roi = d->has_roi ? d->roi : hp_roi{ 0, 0, c.w, c.h };
    const hp_roi& r = c.roi;
    HP_REQUIRE(r.w > 0 && r.h > 0 && r.x >= 0 && r.y >= 0 && (int64_t)r.x + r.w <= c.w && (int64_t)r.y + r.h <= c.h, HP_ERR_INVALID,
        "%s: %s: roi (%d, %d, %d x %d) is empty or not inside the %d x %d frame", who, c.name, r.x, r.y, r.w, r.h, c.w, c.h);
    HP_REQUIRE(palette, HP_ERR_INVALID, "%s: %s: null palette", who, c.name);
    for (int i = 0; i < 256; ++i)
        for (int k = 0; k < 4; ++k)
            HP_REQUIRE(palette[i][k] >= 0 && palette[i][k] <= 255, HP_ERR_INVALID, "%s: %s: palette entry %d holds %d, outside [0, 255]", who, c.name, i, palette[i][k]);
    c.ax = hp_orient::axes_of(d->orientation);
    c.nx = c.ax.swap ? r.h : r.w, c.ny = c.ax.swap ? r.w : r.h;
    c.W = opacity_weight(opacity);
    return HP_OK;
}

int call_bgr(call& c, const char* who, uint8_t* bgr, int w, int h, int stride, const hp_mapview_desc* d, const int32_t (*palette)[4], float opacity)
{
    HP_TRY(hp::check_bgr_frame(who, bgr, w, h, stride));
    c.w = w, c.h = h;
    describe_bgr(c.f, bgr, stride);
    return check_call(c, who, d, palette, opacity);
}

int call_yuv(call& c, const char* who, const hp_yuv_image* im, bool kernel_access, const hp_mapview_desc* d, const int32_t (*palette)[4], float opacity)
{
    HP_TRY(hp_yuv::validate(im, who, kernel_access));
    const hp_yuv::layout& l = *hp_yuv::layout_of(im->format);
    c.name = l.name, c.w = im->width, c.h = im->height, c.image = im;
    describe_yuv(c.f, *im);
    return check_call(c, who, d, palette, opacity);
}

const float* frame_maps(const hp_mapview_desc* d) { return d->maps + (size_t)d->frame * d->C * d->mh * d->mw; }

view make_view(const call& c, const hp_mapview_desc* d, const entry* pal, const uint32_t* xtab, const uint32_t* ytab, const uint8_t* plane)
{
    return view{ pal, xtab, ytab, plane, d->mw, c.roi.x, c.roi.y, c.roi.w, c.roi.h, c.ax.swap, c.ax.flip_x, c.ax.flip_y };
}

template <int SB, int PX, int PY> planar_writer<SB, PX, PY> planar_of(const target& f)
{
    planar_writer<SB, PX, PY> t;
    t.y = const_cast<uint8_t*>(f.map.y), t.u = const_cast<uint8_t*>(f.map.u), t.v = const_cast<uint8_t*>(f.map.v);
    t.y_stride = f.map.y_stride, t.c_stride = f.map.c_stride, t.v_extra = f.map.v_extra, t.pairs = f.planes == 2, t.shift = f.shift;
    return t;
}

const std::vector<uint32_t>& cached_taps(hp_mapview::axis& a, int U, int m, double cover)
{
    if (a.U != U || a.m != m || a.cover != cover) {
        a.taps.resize((size_t)U);
        build_taps(U, m, cover, a.taps.data());
        a.U = U, a.m = m, a.cover = cover;
    }
    return a.taps;
}

int draw_device(hp_mapview* mv, const char* who, const call& c, const hp_mapview_desc* d, const int32_t (*palette)[4], hipStream_t s)
{
    const int cells = d->mh * d->mw;
    HP_REQUIRE(cells <= mv->max_cells, HP_ERR_INVALID, "%s: %s: maps of %d x %d = %d cells, the handle was created for %d", who, c.name, d->mh, d->mw, cells,
        mv->max_cells);
    uint8_t* stage;
    HP_TRY(mv->ring.take(stage));
    build_entries(c.image, palette, c.W, reinterpret_cast<entry*>(stage));
    uint32_t* tabs = reinterpret_cast<uint32_t*>(stage + OFF_TABS);
    const std::vector<uint32_t>&tx = cached_taps(mv->x, c.nx, d->mw, d->cover_x), &ty = cached_taps(mv->y, c.ny, d->mh, d->cover_y);
    std::copy(tx.begin(), tx.end(), tabs);
    std::copy(ty.begin(), ty.end(), tabs + c.nx);
    HP_TRY(mv->ring.upload(OFF_TABS + (size_t)(c.nx + c.ny) * sizeof(uint32_t), s));
    const uint8_t* dev = mv->ring.device<uint8_t>();
    uint8_t* plane = const_cast<uint8_t*>(dev) + OFF_PLANE;
    const uint32_t* dev_tabs = reinterpret_cast<const uint32_t*>(dev + OFF_TABS);
    const view v = make_view(c, d, reinterpret_cast<const entry*>(dev), dev_tabs, dev_tabs + c.nx, plane);

    const mv_reduce r { frame_maps(d), plane, cells, d->c0, d->cn, d->c_step, d->mode, d->gain };
    hipLaunchKernelGGL(mapview_reduce_kernel, dim3(hp::ceil_div(cells, THREADS)), dim3(THREADS), 0, s, r);

    const target& f = c.f;
    mv_grid g;
    g.run0 = (c.roi.x >> f.sx) / RUN, g.by0 = c.roi.y >> f.sy;
    g.runs = ((c.roi.x + c.roi.w - 1) >> f.sx) / RUN - g.run0 + 1, g.brows = ((c.roi.y + c.roi.h - 1) >> f.sy) - g.by0 + 1;
    const dim3 grid(hp::ceil_div(g.runs, RUNS_X), hp::ceil_div(g.brows, ROWS_Y));
    if (f.bgr)
        hipLaunchKernelGGL(mapview_bgr_kernel, grid, dim3(THREADS), 0, s, v, g, bgr_writer{ f.base, f.stride });
    else if (f.sample_bytes == 2)
        hipLaunchKernelGGL(mapview_word16_kernel, grid, dim3(THREADS), 0, s, v, g, planar_of<2, 2, 2>(f));
    else if (f.planes == 1) {
        const uint8_t* first = f.map.y < f.map.u ? f.map.y : f.map.u;
        hipLaunchKernelGGL(mapview_packed8_kernel, grid, dim3(THREADS), 0, s, v, g, packed_writer{ const_cast<uint8_t*>(first), f.map.y_stride, f.map.y != first });
    } else if (f.sy == 1)
        hipLaunchKernelGGL((mapview_planar8_kernel<2, 2>), grid, dim3(THREADS), 0, s, v, g, planar_of<1, 2, 2>(f));
    else if (f.sx == 1)
        hipLaunchKernelGGL((mapview_planar8_kernel<2, 1>), grid, dim3(THREADS), 0, s, v, g, planar_of<1, 2, 1>(f));
    else
        hipLaunchKernelGGL((mapview_planar8_kernel<1, 1>), grid, dim3(THREADS), 0, s, v, g, planar_of<1, 1, 1>(f));
    mv->last_plane = plane, mv->last_cells = cells;
    return mv->ring.commit(s);
}

// ---- host twin: maps and frame in host memory -----------------------------------------------------------------------------------------------------

void index_host(const hp_mapview_desc* d, uint8_t* out)
{
    const int cells = d->mh * d->mw;
    const float* maps = frame_maps(d);
    for (int cell = 0; cell < cells; ++cell)
        out[cell] = (uint8_t)index_of(maps, cells, cell, d->c0, d->cn, d->c_step, d->mode, d->gain);
}

int draw_host(const call& c, const hp_mapview_desc* d, const int32_t (*palette)[4])
{
    std::vector<uint8_t> plane((size_t)d->mh * d->mw);
    index_host(d, plane.data());
    std::vector<entry> pal(256);
    build_entries(c.image, palette, c.W, pal.data());
    std::vector<uint32_t> tx((size_t)c.nx), ty((size_t)c.ny);
    build_taps(c.nx, d->mw, d->cover_x, tx.data());
    build_taps(c.ny, d->mh, d->cover_y, ty.data());
    paint_host(c.f, make_view(c, d, pal.data(), tx.data(), ty.data(), plane.data()));
    return HP_OK;
}

} // namespace

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------

extern "C" {

int hp_mapview_create(hp_mapview** out, int max_map_cells)
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_mapview_create: null output");
    *out = nullptr;
    HP_REQUIRE(max_map_cells > 0 && max_map_cells <= MAX_MAP_CELLS, HP_ERR_INVALID, "hp_mapview_create: max_map_cells %d (1 .. %d)", max_map_cells, MAX_MAP_CELLS);
    std::unique_ptr<hp_mapview> v(new hp_mapview); // a failed create frees what it allocated
    v->max_cells = max_map_cells;
    HP_TRY(v->ring.alloc(OFF_PLANE + (size_t)max_map_cells, "hp_mapview_create"));
    *out = v.release();
    return HP_OK;
}

void hp_mapview_destroy(hp_mapview* v) { delete v; } // the ring drains first

int hp_mapview_cover(int frame_w, int frame_h, int in_w, int in_h, int keep_ratio, double cover[2])
{
    HP_REQUIRE(cover, HP_ERR_INVALID, "hp_mapview_cover: null output");
    HP_REQUIRE(frame_w > 0 && frame_h > 0 && in_w > 0 && in_h > 0, HP_ERR_INVALID, "hp_mapview_cover: sizes %d x %d -> %d x %d", frame_w, frame_h, in_w, in_h);
    cover[0] = cover[1] = 1.;
    if (keep_ratio) {
        int iw = 0, ih = 0;
        hp_letterbox_inner(frame_w, frame_h, in_w, in_h, &iw, &ih);
        cover[0] = iw / (double)in_w, cover[1] = ih / (double)in_h;
    }
    return HP_OK;
}

int hp_mapview_taps(int U, int m, double cover, int32_t (*out)[3])
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_mapview_taps: null output");
    HP_REQUIRE(U > 0 && U <= MAX_DIM, HP_ERR_INVALID, "hp_mapview_taps: %d pixels (1 .. %d)", U, MAX_DIM);
    HP_REQUIRE(m > 0 && m <= MAX_MAP_SIDE, HP_ERR_INVALID, "hp_mapview_taps: %d cells (1 .. %d)", m, MAX_MAP_SIDE);
    HP_REQUIRE(cover > 0. && cover <= 1., HP_ERR_INVALID, "hp_mapview_taps: cover %g is outside (0, 1]", cover);
    for (int u = 0; u < U; ++u) {
        const tap t = tap_of(u, U, m, cover);
        out[u][0] = t.i0, out[u][1] = t.i1, out[u][2] = t.w;
    }
    return HP_OK;
}

int hp_mapview_palette(int kind, int alpha_mode, int32_t out[256][4])
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_mapview_palette: null output");
    HP_REQUIRE(kind == HP_MAPVIEW_JET || kind == HP_MAPVIEW_HEAT || kind == HP_MAPVIEW_GREY, HP_ERR_INVALID, "hp_mapview_palette: unknown kind %d", kind);
    HP_REQUIRE(alpha_mode == HP_MAPVIEW_ALPHA_CONSTANT || alpha_mode == HP_MAPVIEW_ALPHA_SCALED, HP_ERR_INVALID, "hp_mapview_palette: unknown alpha mode %d", alpha_mode);
    for (int i = 0; i < 256; ++i)
        palette_entry(kind, alpha_mode, i, out[i]);
    return HP_OK;
}

int hp_mapview_palette_yuv(const int32_t rgba[256][4], int matrix, int range, int depth, int32_t out[256][4])
{
    HP_REQUIRE(rgba && out, HP_ERR_INVALID, "hp_mapview_palette_yuv: null pointer");
    HP_REQUIRE(matrix >= HP_YUV_BT601 && matrix <= HP_YUV_BT2020, HP_ERR_INVALID, "hp_mapview_palette_yuv: unknown matrix %d", matrix);
    HP_REQUIRE(range == HP_YUV_LIMITED || range == HP_YUV_FULL, HP_ERR_INVALID, "hp_mapview_palette_yuv: unknown range %d", range);
    HP_REQUIRE(depth == 8 || depth == 10, HP_ERR_INVALID, "hp_mapview_palette_yuv: depth %d (8 or 10)", depth);
    for (int i = 0; i < 256; ++i) {
        for (int k = 0; k < 4; ++k)
            HP_REQUIRE(rgba[i][k] >= 0 && rgba[i][k] <= 255, HP_ERR_INVALID, "hp_mapview_palette_yuv: palette entry %d holds %d, outside [0, 255]", i, rgba[i][k]);
        hp_yuv::colour_of(rgba[i][0], rgba[i][1], rgba[i][2], matrix, range, depth, out[i]);
        out[i][3] = rgba[i][3];
    }
    return HP_OK;
}

int hp_mapview_draw_u8c3(hp_mapview* v, uint8_t* dev_bgr, int w, int h, int stride, const hp_mapview_desc* d, const int32_t palette[256][4], float opacity,
    void* stream)
{
    HP_REQUIRE(v, HP_ERR_INVALID, "hp_mapview_draw_u8c3: null handle");
    call c;
    HP_TRY(call_bgr(c, "hp_mapview_draw_u8c3", dev_bgr, w, h, stride, d, palette, opacity));
    return draw_device(v, "hp_mapview_draw_u8c3", c, d, palette, (hipStream_t)stream);
}

int hp_mapview_draw_yuv(hp_mapview* v, const hp_yuv_image* frame, const hp_mapview_desc* d, const int32_t palette[256][4], float opacity, void* stream)
{
    HP_REQUIRE(v, HP_ERR_INVALID, "hp_mapview_draw_yuv: null handle");
    call c;
    HP_TRY(call_yuv(c, "hp_mapview_draw_yuv", frame, true, d, palette, opacity));
    return draw_device(v, "hp_mapview_draw_yuv", c, d, palette, (hipStream_t)stream);
}

int hp_mapview_draw_u8c3_host(uint8_t* bgr, int w, int h, int stride, const hp_mapview_desc* d, const int32_t palette[256][4], float opacity)
{
    call c;
    HP_TRY(call_bgr(c, "hp_mapview_draw_u8c3_host", bgr, w, h, stride, d, palette, opacity));
    return draw_host(c, d, palette);
}

int hp_mapview_draw_yuv_host(const hp_yuv_image* frame, const hp_mapview_desc* d, const int32_t palette[256][4], float opacity)
{
    call c;
    HP_TRY(call_yuv(c, "hp_mapview_draw_yuv_host", frame, false, d, palette, opacity));
    return draw_host(c, d, palette);
}

int hp_mapview_index_host(const hp_mapview_desc* d, uint8_t* out)
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_mapview_index_host: null output");
    HP_TRY(check_maps("hp_mapview_index_host", "maps", d));
    index_host(d, out);
    return HP_OK;
}

int hp_mapview_debug_plane(hp_mapview* v, uint8_t* out, int cap)
{
    HP_REQUIRE(v && out && cap >= 0, HP_ERR_INVALID, "hp_mapview_debug_plane: null pointer or negative capacity");
    HP_REQUIRE(v->last_plane, HP_ERR_STATE, "hp_mapview_debug_plane: the handle has drawn nothing yet");
    HP_HIP_TRY(hipDeviceSynchronize());
    const int n = v->last_cells < cap ? v->last_cells : cap;
    if (n > 0)
        HP_HIP_TRY(hipMemcpy(out, v->last_plane, (size_t)n, hipMemcpyDeviceToHost));
    return v->last_cells;
}

} // extern "C"
