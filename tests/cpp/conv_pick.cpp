// Host-only check of csrc/conv_pick.hpp, the one decision behind conv_weight_layout / conv_mfma_tile / conv_splitk / launch_conv_mfma.
//   conv_pick.bin GOLDEN    every line of tests/golden/conv_pick.txt - the answers of the four separate cascades this picker replaced,
//                           recorded from them over the grid below - is reproduced, and every choice is consistent with itself
//   conv_pick.bin --print   prints the table from the picker as it is now (to record a deliberate change)
// A line is "KH KW Cin Cout H W B stride dil valid align f32 w_layout : layout tile ksplit scratch_bytes"; Cin / Cout are the layer's,
// padded as the engine pads them (Cin to 32; Cout to 64, above 64 to 128).  `align` numbers the slice variants of make_case.
#include "../../hyperpose_amd/csrc/conv_pick.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace hp;

static int g_checks = 0, g_fail = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            if (++g_fail <= 20) {                                \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                        \
                std::printf("\n");                               \
            }                                                    \
        }                                                        \
    } while (0)

static int round_up(int a, int b) { return (a + b - 1) / b * b; }

struct geom {
    int KH, KW, Cin, Cout, H, W, B, stride, dil, valid, align, f32, wl;
};

// the engine's conv_params for a layer (lower16_conv): TF "SAME" padding (valid: none), views into buffers whose channel stride is a
// multiple of 32.  Pointers are never dereferenced by the picker: any non-null value stands for "present".
static conv_params make_case(const geom& g)
{
    static __half buf[1];
    static float fbuf[1];
    conv_params p{};
    p.B = g.B, p.H = g.H, p.W = g.W, p.KH = g.KH, p.KW = g.KW, p.stride = g.stride, p.dil = g.dil;
    p.Cin = round_up(g.Cin, 32), p.Cout = g.Cout, p.Cout_pad = g.Cout > 64 ? round_up(g.Cout, 128) : 64;
    const int eh = (g.KH - 1) * g.dil + 1, ew = (g.KW - 1) * g.dil + 1;
    if (g.valid) {
        p.OH = (g.H - eh) / g.stride + 1, p.OW = (g.W - ew) / g.stride + 1;
    } else {
        p.OH = (g.H + g.stride - 1) / g.stride, p.OW = (g.W + g.stride - 1) / g.stride;
        const int th = (p.OH - 1) * g.stride + eh - g.H, tw = (p.OW - 1) * g.stride + ew - g.W;
        p.pad_t = th > 0 ? th / 2 : 0, p.pad_l = tw > 0 ? tw / 2 : 0;
    }
    p.npix = p.B * p.OH * p.OW;
    // align: 0 whole buffers; 1 aligned slices of wider buffers; 2 input slice off the 8-channel grid; 3 output slice off it; 4 residual,
    // aligned; 5 residual slice off the grid; 6 no fp16 output; 7 residual stride off the grid; 8 output stride off it; 9 input slice
    // that ends beyond its buffer's stride
    const int a = g.align;
    p.in.p = buf, p.in.coff = a == 1 ? 32 : a == 2 ? 4 : 0, p.in.cs = round_up(p.in.coff + p.Cin, 32) - (a == 9 ? 32 : 0);
    p.out.p = a == 6 ? nullptr : buf, p.out.coff = a == 1 ? 8 : a == 3 ? 4 : 0, p.out.cs = round_up(p.out.coff + p.Cout, 32) + (a == 8 ? 4 : 0);
    if (a == 1 || a == 4 || a == 5 || a == 7)
        p.res.p = buf, p.res.coff = a == 1 ? 16 : a == 5 ? 4 : 0, p.res.cs = round_up(p.res.coff + p.Cout, 32) + (a == 7 ? 4 : 0);
    p.in.wp = p.out.wp = p.res.wp = g.W + 6, p.in.img = p.out.img = p.res.img = (g.H + 6) * (g.W + 6);
    p.out_f32 = g.f32 ? fbuf : nullptr;
    p.w_layout = g.wl;
    return p;
}

static std::string line_of(const geom& g)
{
    const conv_params p = make_case(g);
    size_t bytes = 0;
    const int ks = pick::splitk(p, &bytes);
    char s[256];
    std::snprintf(s, sizeof s, "%d %d %d %d %d %d %d %d %d %d %d %d %d : %d %d %d %zu", g.KH, g.KW, g.Cin, g.Cout, g.H, g.W, g.B, g.stride, g.dil,
        g.valid, g.align, g.f32, g.wl, pick::weight_layout(p), pick::tile(p), ks, bytes);
    return s;
}

// ---- the grid: kernels 1 / 3 / 5 / 7 and two non-square ones, the channel counts and maps of the built-in networks, batch 1 / 8 / 32,
// stride and dilation 1 / 2, every slice variant, fp32 output on / off, both weight layouts - pruned to blocks that each cross what one
// group of predicates reads
static const int KS[][2] = {{1, 1}, {3, 3}, {5, 5}, {7, 7}, {1, 3}, {3, 1}};
static const int CIN[] = {3, 32, 64, 96, 128, 192, 256, 512, 2048};
static const int COUT[] = {19, 38, 64, 128, 256, 512};
static const int MAPS[][2] = {{1, 1}, {12, 12}, {25, 25}, {46, 46}, {49, 49}, {96, 54}};

static std::vector<geom> grid()
{
    std::vector<geom> v;
    // 1: kernel x channels x map with fragment-ordered weights at batch 8 (the forms and their geometry tests); 5 x 5 / 7 x 7 and the
    // non-square kernels on the maps their tests tell apart, 38 outputs (padded and off the 8-channel grid like 19) once per input width
    for (int ki = 0; ki < 6; ++ki)
        for (int ci : CIN)
            for (int co : COUT)
                for (int mi = 0; mi < 6; ++mi) {
                    if ((ki >= 2 && (mi == 2 || mi == 4 || mi == 5)) || (ki >= 4 && (mi == 0 || co == 19 || co == 512)) || (co == 38 && (ki > 1 || mi != 3)))
                        continue;
                    v.push_back({KS[ki][0], KS[ki][1], ci, co, MAPS[mi][0], MAPS[mi][1], 8, 1, 1, 0, 0, 0, 1});
                }
    // 2: batch 1 and 32 (block counts: the (TM, NTP) of the pixel-block GEMM, split-K)
    for (int b : {1, 32})
        for (int k : {1, 3, 7})
            for (int ci : {192, 256, 512, 2048})
                for (int co : {128, 256, 512})
                    for (int mi : {1, 2, 3, 5})
                        v.push_back({k, k, ci, co, MAPS[mi][0], MAPS[mi][1], b, 1, 1, 0, 0, 0, 1});
    // 3: weights in rows (the generic GEMM's tile: output rows, pixels, K step)
    for (int ci : {3, 64})
        for (int co : COUT)
            for (auto& m : MAPS)
                for (int b : {1, 8, 32})
                    v.push_back({3, 3, ci, co, m[0], m[1], b, 1, 1, 0, 0, 0, 0});
    // 4: stride 2 / dilation 2 (1 x 1 maps: a stride leaves the map's size alone; 25 x 25: odd, so stride 2 pads like stride 1)
    for (int sd : {1, 2, 3})
        for (int k : {1, 3, 5})
            for (int ci : {64, 128, 256, 512})
                for (int co : {128, 256})
                    for (int mi : {0, 1, 2, 3, 5})
                        v.push_back({k, k, ci, co, MAPS[mi][0], MAPS[mi][1], 8, 1 + (sd & 1), 1 + (sd >> 1), 0, 0, 0, 1});
    for (int sd : {1, 2, 3})
        for (int k : {1, 3})
            v.push_back({k, k, 64, 128, 46, 46, 8, 1 + (sd & 1), 1 + (sd >> 1), 0, 0, 0, 0});
    // 5: slices, residuals and the fp32 output (the fast epilogue and the input-slice tests)
    for (int a = 1; a <= 9; ++a)
        for (int f : {0, 1})
            for (int k : {1, 3, 7})
                for (int ci : {128, 256})
                    for (int co : {19, 128})
                        for (int wl : {0, 1})
                            if (wl == 1 || (k == 3 && ci == 128))
                                v.push_back({k, k, ci, co, 46, 46, 8, 1, 1, 0, a, f, wl});
    // 6: no padding (the output is smaller than the input)
    for (int k : {3, 5})
        for (int ci : {64, 256})
            for (int wl : {0, 1})
                v.push_back({k, k, ci, 128, 46, 46, 8, 1, 1, 1, 0, 0, wl});
    // 7: chunk counts beside the split-K factors: 5 (odd), 6 (even, below 8), 10 (not a multiple of 4) on few blocks
    for (int ci : {320, 384, 640})
        for (int b : {1, 8, 32})
            v.push_back({3, 3, ci, 512, 12, 12, b, 1, 1, 0, 0, 0, 1});
    // 8: output channels off the 8-channel grid under a 128-row pad
    for (int k : {1, 3})
        for (int ci : {128, 512})
            for (int wl : {0, 1})
                v.push_back({k, k, ci, 100, 46, 46, 8, 1, 1, 0, 0, 0, wl});
    return v;
}

// ---- what must hold for any choice, whatever the table says
static void check_consistent(const geom& g)
{
    const conv_params p = make_case(g);
    const conv_choice c1 = pick_conv(p, 1), c0 = pick_conv(p, 0), c = pick_conv(p, p.w_layout);
    const int code = g.KH * 10000000 + g.Cin * 100 + g.align; // (for the message)
    CHECK(c0.form == CONV_GEMM && c0.ok && c1.form != CONV_GEMM, "%d: layout 0 is the GEMM, layout 1 never", code);
    CHECK(pick::weight_layout(p) == (c1.ok ? 1 : 0), "%d: fragment order exactly where layout 1 has a form", code);
    const bool fe = fast_epilogue(p);
    switch (c1.form) {
    case CONV_SMALL1X1:
        CHECK(c1.ok == (use_small1x1(p) && fe) && c1.KP == p.Cin && (c1.KP == 64 || c1.KP == 128 || c1.KP == 192 || c1.KP == 256), "%d: small 1x1", code);
        break;
    case CONV_BIG1X1: {
        const int v = c1.TM * 1000 + c1.NTP;
        CHECK(v == big1x1_variant(p) && c1.ok == (v && fe) && (!c1.ok || v == 1002 || v == 2002 || v == 1004), "%d: big 1x1 %d", code, v);
        CHECK(!c1.ok || (p.Cin % 256 == 0 && p.Cout_pad % (128 * c1.TM) == 0), "%d: big 1x1 %d divides", code, v);
        break;
    }
    case CONV_DIRECT: {
        const int inst = c1.KS * 10000 + c1.CK * 10 + c1.NBUF;
        CHECK(c1.ok && use_gdirect(p) == c1.CK && c1.KS == p.KH && p.KH == p.KW && c1.nchunks * c1.CK == p.Cin && fe, "%d: direct", code);
        CHECK(c1.CK == (p.Cin == 128 ? 128 : 64), "%d: one 128-channel chunk only where it is the whole input", code);
        CHECK(inst == 71281 || inst == 70642 || inst == 51281 || inst == 50642 || inst == 31281 || inst == 30641 || inst == 30642, "%d: direct <%d>", code, inst);
        CHECK(c1.NBUF == 2 || c1.nchunks == 1, "%d: one buffer holds one chunk", code);
        break;
    }
    case CONV_HALO:
        CHECK(c1.ok == (use_halo(p) && fe) && (!c1.ok || c1.CIN == p.Cin), "%d: halo", code);
        break;
    default:
        break;
    }
    CHECK((c0.BM == 64 || c0.BM == 128) && (c0.BN == 64 || c0.BN == 128) && (c0.BK == 32 || c0.BK == 64) && p.Cout_pad % c0.BM == 0 && p.Cin % c0.BK == 0
            && (c0.EPI == 0) == fe, "%d: GEMM tile", code);
    // split-K only where the launcher's split branch takes it: conv_direct_kernel<3, 64, 2> with the chunks dealt evenly
    CHECK(c.ksplit >= 1 && (c.ksplit > 1) == (c.scratch_bytes > 0), "%d: scratch goes with a split", code);
    CHECK(c.ksplit == 1 || (c.form == CONV_DIRECT && c.ok && c.KS == 3 && c.CK == 64 && c.NBUF == 2 && c.nchunks > 1 && c.nchunks % c.ksplit == 0),
        "%d: split %d of %d chunks", code, c.ksplit, c.nchunks);
}

int main(int argc, char** argv)
{
    const std::vector<geom> cases = grid();
    if (argc == 2 && !std::strcmp(argv[1], "--print")) {
        for (const geom& g : cases)
            std::printf("%s\n", line_of(g).c_str());
        return 0;
    }
    if (argc != 2) {
        std::printf("usage: %s GOLDEN | --print\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::printf("cannot open %s\n", argv[1]);
        return 2;
    }
    size_t n = 0;
    char buf[512];
    int forms[5] = {};
    for (; std::fgets(buf, sizeof buf, f); ++n) {
        buf[std::strcspn(buf, "\r\n")] = 0;
        CHECK(n < cases.size(), "the table has more lines than the grid");
        if (n >= cases.size())
            break;
        const std::string got = line_of(cases[n]);
        CHECK(got == buf, "line %zu: want '%s' got '%s'", n + 1, buf, got.c_str());
        check_consistent(cases[n]);
        const conv_params p = make_case(cases[n]);
        const conv_choice c = pick_conv(p, p.w_layout);
        forms[c.form] += c.ok;
    }
    std::fclose(f);
    CHECK(n == cases.size(), "the table has %zu lines, the grid %zu cases", n, cases.size());
    for (int i = 0; i < 5; ++i)
        CHECK(forms[i] > 0, "form %d never chosen", i);
    std::printf("%s %d\n", g_fail ? "FAILED" : "OK", g_checks);
    return g_fail ? 1 : 0;
}
