// The host side of hyperpose_amd/csrc/mapview.hpp - index plane, taps, pixel index, palettes and the host painter - on frames, maps and tables
// allocated with NO slack: one malloc of exactly the needed size each, so that under -fsanitize=address,undefined any read or write outside them, and
// any overflow of the integer rules, aborts.  Every layout (BGR and the nine hp_yuv_image formats), the smallest frame (2 x 2 with a 1 x 1 map), the
// small odd ones, the widest one (U = 8192), all eight orientations, rois with odd offsets and sizes, and the extreme operands of the pixel index
// (weight 2048, cells of 255).  That this file compiles with plain g++ and no ROCm include path is the proof that mapview.hpp and the headers it
// includes are host-pure.  Prints "OK <frames painted>"; run by tests/test_cpp_mapview_rules.py.
#include "../../hyperpose_amd/csrc/mapview.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace hp_mv;

static int painted = 0;

template <class T> struct exact { // n elements and not a byte more
    T* p;
    explicit exact(size_t n) : p((T*)std::malloc(n * sizeof(T))) {}
    ~exact() { std::free(p); }
};

static void fail(int code)
{
    std::printf("FAILED %d\n", code);
    std::exit(code);
}

// a frame's maps: C x mh x mw with the values the index rule must survive
static void fill_maps(float* m, int C, int mh, int mw)
{
    const float special[] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), -3.f, 3e38f, 1e-30f,
        0.999f, 1.f, 0.5f };
    for (int i = 0; i < C * mh * mw; ++i)
        m[i] = i % 11 < 9 && (i / 11) % 3 == 0 ? special[i % 11] : (float)((i * 37) % 101) / 90.f - 0.1f;
}

static void paint_all(const target& f, const hp_yuv_image* im, int w, int h, int C, int mh, int mw)
{
    exact<float> maps((size_t)C * mh * mw);
    fill_maps(maps.p, C, mh, mw);
    exact<uint8_t> plane((size_t)mh * mw);
    int32_t rgba[256][4];
    exact<entry> pal(256);
    const hp_roi rois[] = { { 0, 0, w, h }, { 1, 1, w - 1, h - 1 }, { w / 2, h / 2, 1, 1 }, { w - 1, 0, 1, h }, { 0, h - 1, w, 1 } };
    for (int mode : { HP_MAPVIEW_MAX, HP_MAPVIEW_FIELD }) {
        const int cn = mode == HP_MAPVIEW_FIELD ? C / 2 : C, step = mode == HP_MAPVIEW_FIELD ? 2 : 1;
        if (cn < 1)
            continue;
        for (int cell = 0; cell < mh * mw; ++cell) {
            const int q = index_of(maps.p, mh * mw, cell, 0, cn, step, mode, mode == HP_MAPVIEW_FIELD ? 4.f : 0.5f);
            if (q < 0 || q > 255)
                fail(2);
            plane.p[cell] = (uint8_t)q;
        }
        for (int orientation = 0; orientation < 8; ++orientation)
            for (const hp_roi& r : rois) {
                if (r.w < 1 || r.h < 1)
                    continue;
                const hp_orient::axes ax = hp_orient::axes_of(orientation);
                const int nx = ax.swap ? r.h : r.w, ny = ax.swap ? r.w : r.h;
                exact<uint32_t> tx((size_t)nx), ty((size_t)ny);
                build_taps(nx, mw, orientation & 1 ? 0.75 : 1., tx.p);
                build_taps(ny, mh, 0.9375, ty.p);
                for (int i = 0; i < 256; ++i)
                    palette_entry(orientation % 3, orientation & 1, i, rgba[i]);
                build_entries(im, rgba, opacity_weight(orientation < 4 ? 1.f : 0.5f), pal.p);
                paint_host(f, view{ pal.p, tx.p, ty.p, plane.p, mw, r.x, r.y, r.w, r.h, ax.swap, ax.flip_x, ax.flip_y });
                ++painted;
            }
    }
}

// an odd size next to v, where the layout allows one and v is neither the smallest nor the largest
static int odd(int v) { return v > 2 && v < MAX_DIM ? v | 1 : v; }

static void sweep_layouts(int w0, int h0, int C, int mh, int mw)
{
    {
        const int w = odd(w0), h = odd(h0); // BGR: odd sizes; rows of exactly w * 3 bytes
        exact<uint8_t> p((size_t)w * h * 3);
        std::memset(p.p, 0xFF, (size_t)w * h * 3);
        target f;
        describe_bgr(f, p.p, w * 3);
        paint_all(f, nullptr, w, h, C, mh, mw);
    }
    for (int format = 0; hp_yuv::layout_of(format); ++format) {
        const hp_yuv::layout& l = *hp_yuv::layout_of(format);
        const int w = l.sx ? w0 : odd(w0), h = l.sy ? h0 : odd(h0);
        hp_yuv_image im {};
        im.format = format, im.matrix = HP_YUV_BT2020, im.range = format & 1, im.width = w, im.height = h;
        void* planes[3] = { nullptr, nullptr, nullptr };
        for (int k = 0; k < l.planes; ++k) {
            const size_t bytes = hp_yuv::row_bytes(l, k, w) * (size_t)hp_yuv::rows(l, k, h);
            planes[k] = std::malloc(bytes);
            std::memset(planes[k], 0xFF, bytes);
            im.plane[k] = planes[k], im.stride[k] = (int)hp_yuv::row_bytes(l, k, w);
        }
        target f;
        describe_yuv(f, im);
        paint_all(f, &im, w, h, C, mh, mw);
        for (void* p : planes)
            std::free(p);
    }
}

int main()
{
    // taps: inside [0, m - 1], weights inside [0, 2048], and the weight 2048 does occur
    bool full_weight = false;
    for (int U : { 1, 2, 5, 7, 70, 8192 })
        for (int m : { 1, 2, 7, 9 })
            for (double cover : { 1., 0.75, 0.9375 })
                for (int u = 0; u < U; ++u) {
                    const tap t = tap_of(u, U, m, cover);
                    if (t.i0 < 0 || t.i1 < t.i0 || t.i1 > m - 1 || t.i1 - t.i0 > 1 || t.w < 0 || t.w > ONE)
                        fail(3);
                    full_weight |= t.w == ONE;
                    const uint32_t packed = pack_tap(t);
                    if ((int)(packed & 0xffffu) != t.i0 || (int)((packed >> 16) & 1u) != t.i1 - t.i0 || (int)(packed >> 17) != t.w)
                        fail(4);
                }
    if (!full_weight)
        fail(5);
    // pixel index at its largest operands: cells of 255 under every pair of extreme weights stay 255 and overflow nothing
    const uint8_t cells[4] = { 255, 255, 255, 255 };
    for (int wx : { 0, 1, 1024, 2047, 2048 })
        for (int wy : { 0, 1, 1024, 2047, 2048 })
            if (pixel_index(cells, 2, pack_tap(tap{ 0, 1, wx }), pack_tap(tap{ 0, 1, wy })) != 255)
                fail(6);
    const uint8_t one[1] = { 255 };
    if (pixel_index(one, 1, pack_tap(tap{ 0, 0, 2048 }), pack_tap(tap{ 0, 0, 0 })) != 255)
        fail(7);

    sweep_layouts(2, 2, 2, 1, 1);    // one chroma block, m = 1
    sweep_layouts(70, 46, 9, 7, 5);  // BGR and I444 at 71 x 47, the 4:2:2 layouts at 70 x 47
    sweep_layouts(16, 12, 4, 50, 40); // a map larger than the frame
    sweep_layouts(8192, 2, 2, 1, 9); // U = 8192
    std::printf("OK %d\n", painted);
    return 0;
}
