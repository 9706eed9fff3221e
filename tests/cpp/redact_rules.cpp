// The host side of hyperpose_amd/csrc/redact.hpp - the region list and the host painter - on frames allocated with NO slack: one malloc per plane
// of exactly the plane's size, so that under -fsanitize=address,undefined any read or write outside a plane, and any overflow of the integer
// rules, aborts.  Every layout (BGR and the nine hp_yuv_image formats), both effects, cells 2 and 128, heads and bodies of humans that lie partly
// outside the frame, plus regions at the limits of the coordinate range.  The layouts' geometry is the library's own (yuv_formats.hpp): that this
// file compiles with plain g++ and no ROCm include path is the proof that it, part_points.hpp and redact.hpp are host-pure.
// Prints "OK <frames painted>"; run by tests/test_cpp_redact_rules.py.
#include "../../hyperpose_amd/csrc/redact.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static std::vector<hp_human> humans()
{
    std::vector<hp_human> hs(5);
    std::memset(hs.data(), 0, hs.size() * sizeof(hp_human));
    auto set = [&](int i, int k, float x, float y) { hs[i].parts[k] = hp_body_part{ 1, x, y, 1.f }; };
    set(0, 0, 0.5f, 0.2f), set(0, 1, 0.5f, 0.35f), set(0, 2, 0.4f, 0.36f), set(0, 5, 0.6f, 0.36f), set(0, 14, 0.48f, 0.18f), set(0, 8, 0.45f, 0.7f);
    set(1, 0, -0.02f, -0.03f), set(1, 1, -0.05f, 0.1f), set(1, 16, 1.04f, 0.3f);         // partly outside
    set(2, 0, 0.999f, 0.999f), set(2, 15, 1.2f, 1.1f);                                    // the last pixel and beyond
    set(3, 1, 0.2f, 0.6f), set(3, 8, 0.18f, 0.8f);                                        // no face
    set(4, 0, 3e38f, 0.5f), set(4, 14, -1e30f, 0.5f), set(4, 15, 0.3f, 0.9f), set(4, 1, 0.31f, 0.95f);
    return hs;
}

static int painted = 0;

static void run(hp_red::frame& f, const std::vector<hp_redact_region>& regs)
{
    for (int effect : { HP_REDACT_PIXELATE, HP_REDACT_BLACK })
        for (int cell : { 2, 128 }) {
            if (!hp_red::cell_ok(cell))
                std::exit(4);
            hp_red::paint_host(f, regs.data(), (int)regs.size(), effect, cell);
            ++painted;
        }
}

static std::vector<hp_redact_region> regions(int w, int h)
{
    const auto hs = humans();
    std::vector<hp_redact_region> regs(2 * hs.size()), all;
    for (int what : { HP_REDACT_HEAD, HP_REDACT_BODY })
        for (float margin : { 0.5f, 8.f }) {
            const int n = hp_red::build_regions(hs.data(), (int)hs.size(), w, h, what, margin, regs.data(), (int)regs.size());
            if (n < 0 || n > (int)regs.size())
                std::exit(2);
            all.insert(all.end(), regs.begin(), regs.begin() + n);
        }
    // the limits of the coordinate range: the int64 paths of hits() at their largest operands
    all.push_back(hp_redact_region{ HP_REDACT_DISC, 16383, 16383, 16384, 0, -1 });
    all.push_back(hp_redact_region{ HP_REDACT_DISC, -8192, -8192, 16384, 0, -1 });
    all.push_back(hp_redact_region{ HP_REDACT_RECT, -8192, -8192, 16383, 16383, -1 });
    all.push_back(hp_redact_region{ HP_REDACT_RECT, w - 1, h - 1, w - 1, h - 1, -1 });
    all.push_back(hp_redact_region{ HP_REDACT_DISC, 0, 0, 0, 0, -1 });
    for (const auto& g : all)
        if (hp_red::region_fault(g))
            std::exit(3);
    return all;
}

int main()
{
    for (const int size : { 0, 1 }) {
        // BGR, odd width and height; rows of exactly w * 3 bytes
        {
            const int w = size ? 259 : 97, h = size ? 131 : 65;
            uint8_t* p = (uint8_t*)std::malloc((size_t)w * h * 3);
            std::memset(p, 0xFF, (size_t)w * h * 3);
            hp_red::frame f;
            hp_red::describe_bgr(f, p, w, h, w * 3);
            const auto all = regions(w, h);
            // one region at a time first (a partial cell at every edge), then the union
            for (const auto& g : all)
                run(f, { g });
            run(f, all);
            std::free(p);
        }
        for (int format = 0; hp_yuv::layout_of(format); ++format) {
            const hp_yuv::layout& l = *hp_yuv::layout_of(format);
            const int w = (size ? 258 : 98) - (l.sx ? 0 : 1), h = (size ? 130 : 66) - (l.sy ? 0 : 1);
            hp_yuv_image im {};
            im.format = format, im.matrix = HP_YUV_BT709, im.range = HP_YUV_LIMITED, im.width = w, im.height = h;
            void* planes[3] = { nullptr, nullptr, nullptr };
            for (int k = 0; k < l.planes; ++k) {
                const size_t bytes = hp_yuv::row_bytes(l, k, w) * (size_t)hp_yuv::rows(l, k, h);
                planes[k] = std::malloc(bytes);
                std::memset(planes[k], 0xFF, bytes);
                im.plane[k] = planes[k], im.stride[k] = (int)hp_yuv::row_bytes(l, k, w);
            }
            hp_red::frame f;
            hp_red::describe_yuv(f, im);
            const auto all = regions(w, h);
            for (const auto& g : all)
                run(f, { g });
            run(f, all);
            for (void* p : planes)
                std::free(p);
        }
    }
    std::printf("OK %d\n", painted);
    return 0;
}
