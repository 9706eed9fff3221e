// Host-only check of csrc/conv32_pick.hpp, the one decision behind the fp32 dense launchers, their profile labels and the engine's fp32 lowerings.
//   conv32_pick.bin GOLDEN    every line of tests/golden/conv32_pick.txt - what the launchers' own arithmetic and the lowerings' own conditions
//                             answered before the picker replaced them, recorded over the grid of conv32_pick_grid.hpp - is reproduced, and
//                             every choice is consistent with itself
//   conv32_pick.bin --print   prints the table from the picker as it is now (to record a deliberate change)
#include "../../hyperpose_amd/csrc/conv32_pick.hpp"

#include "conv32_pick_grid.hpp"

#include <cstring>

using namespace hp;
using namespace grid32;

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

// is the choice one of the compiled instances?
static bool instance_exists(const conv32_choice& c)
{
    const int* t = c.targ;
    bool found = false;
    switch (c.kernel) {
#define HP_X(BM, BN, WM, WN) found |= t[0] == BM && t[1] == BN && t[2] == WM && t[3] == WN && (t[4] == 0 || t[4] == 1);
    case K32_CONV: HP_CONV32_INSTANCES(HP_X) break;
#undef HP_X
#define HP_X(BN, WN) found |= t[0] == BN && t[1] == WN;
    case K32_T16: HP_CONV32_T16_INSTANCES(HP_X) break;
#undef HP_X
#define HP_X(KT, BN) found |= t[0] == KT && t[1] == BN;
    case K32_WK: HP_CONV32_WK_INSTANCES(HP_X) break;
#undef HP_X
#define HP_X(MW, PIPE, NC) found |= t[0] == MW && t[1] == PIPE && t[2] == NC;
    case K32_WINO2: HP_CONV32_WINO_INSTANCES(HP_X) break;
#undef HP_X
#define HP_X(SPLIT, KS, CK, MW, DWD) found |= t[0] == SPLIT && t[1] == KS && t[2] == CK && t[3] == MW && t[4] == DWD;
    case K32_DIRECT: HP_CONV32_DIRECT_INSTANCES(HP_X) break;
#undef HP_X
#define HP_X(TM2) found |= t[0] == TM2;
    case K32_HEAD: HP_CONV32_HEAD_INSTANCES(HP_X) break;
#undef HP_X
#define HP_X(TMA, TMB) found |= t[0] == TMA && t[1] == TMB;
    case K32_HEAD_PAIR: HP_CONV32_HEAD_PAIR_INSTANCES(HP_X) break;
#undef HP_X
    }
    return found;
}

// ---- what must hold for any choice, whatever the table says
static void check_consistent(const conv_case& g, size_t line)
{
    const conv32_params p = make_case(g);
    const conv32_choice c = pick_conv32(p, switches_of(g), (conv32_form)g.form, g.split != 0);
    const int n = (int)line;
    if (!c.ok)
        return;
    const int* t = c.targ;
    CHECK(instance_exists(c), "line %d: kernel %d <%d, %d, %d, %d, %d> is not compiled", n, (int)c.kernel, t[0], t[1], t[2], t[3], t[4]);
    CHECK(c.lds <= 160 * 1024 && c.threads >= 64 && c.threads <= 1024 && c.grid_x >= 1 && c.grid_y >= 1, "line %d: LDS %zu, %d threads", n, c.lds, c.threads);
    const long xcd = 8;
    switch (c.kernel) {
    case K32_CONV:
    case K32_T16:
    case K32_WK: {
        const int BM = c.kernel == K32_CONV ? t[0] : 64, BN = c.kernel == K32_CONV ? t[1] : c.kernel == K32_T16 ? t[0] : t[1];
        const long groups = p.Cout_pad / BM;
        CHECK(p.Cout_pad % BM == 0 && c.grid_y == 1 && c.grid_x % (xcd * groups) == 0 && (long)(c.grid_x / groups) * BN >= p.npix, "line %d: GEMM grid %u", n, c.grid_x);
        CHECK(c.threads == 256 && (c.kernel == K32_WK ? c.lds == (size_t)pick32::wk_lds(p.Cin, BN) && t[0] == p.Cin : c.lds == 0), "line %d: GEMM block", n);
        if (c.kernel == K32_WK)
            CHECK(c.tile == 39000000 + t[0] * 1000 + t[1], "line %d: tile %d", n, c.tile);
        else
            CHECK(c.tile == 32000000 + (c.kernel == K32_CONV && t[4] ? 400000 : 0) + BM * 1000 + BN, "line %d: tile %d", n, c.tile);
        CHECK(c.kernel != K32_CONV || !t[4] || (p.out.p && !p.out_f32), "line %d: the row-major epilogue writes NHWC only", n);
        break;
    }
    case K32_WINO2: {
        const int nc = t[2], bh = 8 * nc, T = (p.OH + 1) / 2;
        const long groups = p.Cout_pad / (16 * t[0]), blocks = c.grid_x / groups;
        CHECK(pick32::winograd_ok(p) && c.threads == 64 * t[0] && c.lds == (size_t)WINO_LDS[nc], "line %d: Winograd block", n);
        CHECK(c.grid_x % (xcd * groups) == 0 && c.tiles_x * WINO_BW >= p.OW, "line %d: Winograd grid %u", n, c.grid_x);
        if (c.rows) // tile rows numbered through the batch
            CHECK(c.rows == T && c.vh == 0 && c.tiles_y * 4 * nc >= p.B * T && blocks >= (long)c.tiles_x * c.tiles_y, "line %d: rows form", n);
        else if (c.vh) // the batch as one tall image
            CHECK(c.vh * p.in.wp == p.in.img && c.vh % 2 == 0 && c.vh >= p.H + 2 && c.tiles_y * bh >= (p.B - 1) * c.vh + p.H && blocks >= (long)c.tiles_x * c.tiles_y,
                "line %d: tall form", n);
        else
            CHECK(c.tiles_y * bh >= p.OH && blocks >= (long)c.tiles_x * c.tiles_y * p.B, "line %d: per-image form", n);
        CHECK(c.tile == 35000000 + 3000 + t[0], "line %d: tile %d", n, c.tile);
        break;
    }
    case K32_DIRECT: {
        const int per_block = (t[0] ? 64 : 32) * t[3];
        CHECK(pick32::direct_ok(p) && t[0] == g.split && t[1] == p.KH && t[2] == pick32::direct_chunk(p.KH * p.KW) && p.Cin % t[2] == 0 && t[4] == g.dwd, "line %d: direct form", n);
        CHECK(c.threads == (t[0] ? 64 : 128) * t[3] && (long)c.grid_y * per_block == p.Cout_pad, "line %d: direct block, %u groups of %d channels", n, c.grid_y, per_block);
        CHECK(c.tiles_x * DIRECT_T >= p.OW && c.tiles_y * DIRECT_T >= p.OH && c.grid_x == (unsigned)(c.tiles_x * c.tiles_y * p.B), "line %d: direct grid", n);
        CHECK(c.lds == (size_t)pick32::direct_lds(t[0], t[1], t[3], t[4]) + (t[4] ? 40 * p.Cin : 0), "line %d: direct LDS %zu", n, c.lds);
        CHECK(c.tile == (t[0] ? 33000000 : 34000000) + 100000 * t[4] + t[1] * 1000 + t[3], "line %d: tile %d", n, c.tile);
        CHECK(!t[4] || pick32::dw_fusable(p, t[0], t[4]), "line %d: a fused launch the fusion pass would refuse", n);
        break;
    }
    default: CHECK(false, "line %d: kernel %d from pick_conv32", n, (int)c.kernel);
    }
}

static void check_consistent(const head_case& g, size_t line)
{
    conv32_params a, b;
    make_heads(g, a, b);
    const conv32_choice c = g.hidb ? pick_head32(a, g.hid, &b, g.hidb) : pick_head32(a, g.hid);
    const int n = (int)line;
    if (!c.ok)
        return;
    CHECK(instance_exists(c) && c.threads == 256 && c.lds == 0, "line %d: head kernel %d <%d, %d>", n, (int)c.kernel, c.targ[0], c.targ[1]);
    CHECK(c.targ[0] * 32 >= a.Cout && (!g.hidb || c.targ[1] * 32 >= b.Cout), "line %d: output tiles", n);
    const long tiles = g.hidb ? c.grid_x / 16 * 8 : c.grid_x;
    CHECK(tiles * HEAD_PX >= a.npix && (!g.hidb || c.grid_x % 16 == 0), "line %d: head grid %u", n, c.grid_x);
    CHECK(c.tile == 37000000 + g.hid * 100 + g.c2 && pick32::head_ok(HK1, g.hid, g.c2), "line %d: tile %d", n, c.tile);
}

// a form the layer is given must take the parameters it will be launched with (bound(): Cin = cin_split for the direct kernel)
static void check_consistent(const form_case& g, size_t line)
{
    conv32_params p = make_layer(g);
    engine_switches sw;
    sw.no_winograd32 = g.no_wino != 0;
    const conv32_forms f = conv32_layer_forms(p, g.dtype, sw, g.dwf != 0, g.room, g.cin);
    const int n = (int)line;
    if (g.dwf) { // (the engine's sep32 pass fuses a depthwise layer in front only where dw_fusable said yes for every pipe the engine may run on)
        conv32_params q = p;
        q.Cin = round_up(g.cin, 64), q.dw_w = nullptr;
        if (!pick32::dw_fusable(q, false, 1) || (g.dtype == HP_DTYPE_F32S && !pick32::dw_fusable(q, true, 1)))
            return;
    }
    static float buf[1];
    p.w_wino = p.w_frag = buf, p.w_split = reinterpret_cast<const _Float16*>(buf);
    CHECK(f.w_wino == (f.kind == C32_WINO2), "line %d: Winograd weights", n);
    CHECK(f.w_frag == (f.kind == C32_DIRECT) && f.w_split == (f.w_frag && g.dtype == HP_DTYPE_F32S), "line %d: direct weights", n);
    CHECK(g.dtype == HP_DTYPE_F32 || !f.w_wino, "line %d: Winograd is the fp32 pipe's", n);
    if (f.kind == C32_DIRECT) {
        p.Cin = f.cin_split;
        CHECK(f.cin_split >= g.cin && f.cin_split <= g.room, "line %d: %d channels read, %d there", n, f.cin_split, g.room);
        CHECK(pick_conv32(p, sw, C32_DIRECT, false).ok && (!f.w_split || pick_conv32(p, sw, C32_DIRECT, true).ok), "line %d: direct form refused at launch", n);
    } else
        CHECK(f.cin_split == 0 && pick_conv32(p, sw, f.kind, false).ok, "line %d: form %d refused at launch", n, (int)f.kind);
}

int main(int argc, char** argv)
{
    const cases v = grid();
    std::vector<std::string> lines;
    for (auto& g : v.conv)
        lines.push_back(line_of(g));
    for (auto& g : v.head)
        lines.push_back(line_of(g));
    for (auto& g : v.form)
        lines.push_back(line_of(g));
    if (argc == 2 && !std::strcmp(argv[1], "--print")) {
        for (auto& l : lines)
            std::printf("%s\n", l.c_str());
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
    for (; std::fgets(buf, sizeof buf, f); ++n) {
        buf[std::strcspn(buf, "\r\n")] = 0;
        CHECK(n < lines.size(), "the table has more lines than the grid");
        if (n >= lines.size())
            break;
        CHECK(lines[n] == buf, "line %zu: want '%s' got '%s'", n + 1, buf, lines[n].c_str());
    }
    std::fclose(f);
    CHECK(n == lines.size(), "the table has %zu lines, the grid %zu cases", n, lines.size());
    int kernels[7] = {};
    size_t line = 0;
    for (auto& g : v.conv) {
        check_consistent(g, ++line);
        const conv32_choice c = pick_conv32(make_case(g), switches_of(g), (conv32_form)g.form, g.split != 0);
        kernels[c.kernel] += c.ok;
    }
    for (auto& g : v.head) {
        check_consistent(g, ++line);
        conv32_params a, b;
        make_heads(g, a, b);
        const conv32_choice c = g.hidb ? pick_head32(a, g.hid, &b, g.hidb) : pick_head32(a, g.hid);
        kernels[c.kernel] += c.ok;
    }
    for (auto& g : v.form)
        check_consistent(g, ++line);
    for (int i = 0; i < 7; ++i)
        CHECK(kernels[i] > 0, "kernel %d never chosen", i);
    // every compiled direct instance is reachable by the picker's own rule for some layer of the grid
#define HP_X(SPLIT, KS, CK, MW, DWD)                                                                                                  \
    {                                                                                                                                 \
        bool seen = false;                                                                                                            \
        for (auto& g : v.conv) {                                                                                                      \
            const conv32_choice c = pick_conv32(make_case(g), switches_of(g), (conv32_form)g.form, g.split != 0);                      \
            seen |= c.ok && c.kernel == K32_DIRECT && c.targ[0] == SPLIT && c.targ[1] == KS && c.targ[3] == MW && c.targ[4] == DWD;    \
        }                                                                                                                             \
        CHECK(seen, "conv32_direct_kernel<%d, %d, %d, %d, %d> never chosen", (int)SPLIT, KS, CK, MW, DWD);                              \
    }
    HP_CONV32_DIRECT_INSTANCES(HP_X)
#undef HP_X
    std::printf("%s %d\n", g_fail ? "FAILED" : "OK", g_checks);
    return g_fail ? 1 : 0;
}
