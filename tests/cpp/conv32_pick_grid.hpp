// The cases of tests/cpp/conv32_pick.cpp and the line each prints: included behind csrc/conv32_pick.hpp (the table was recorded by a program that
// included this file behind the launchers' own arithmetic instead).  Three kinds of line:
//   C form split KH Cin Cout H W B stride dil out pickB lane bn160 wk latency nc tall view dwd : ok kernel targ[5] grid_x grid_y threads lds tiles_x tiles_y vh rows tile
//   H hid c2 hidb c2b same pair_switch npix : ok kernel TMA TMB grid_x threads tile head_ok head_pair_ok        (hidb = 0: one head)
//   F dtype no_winograd32 dw_in_front room KH cin cout stride : w_wino w_frag w_split kind cin_split dw_fusable(fp32, split; dilation 1)
#include <cstdio>
#include <string>
#include <vector>

namespace grid32 {
using namespace hp;

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

struct conv_case {
    int form, split, KH, Cin, Cout, H, W, B, stride, dil;
    int out;   // 0: NHWC output; 1: + the fp32 NCHW copy; 2: the copy alone (out.p null)
    int pickB; // max_batch where the call brings fewer frames (0: B)
    int lane, bn160, wk, latency, nc, tall;
    int view;  // in.img / in.wp: 0 even and >= H + 2; 1 odd; 2 not integral; 3 smaller than H + 2
    int dwd;   // a depthwise 3 x 3 of this dilation fused in front
};
// (switches at their defaults)
inline conv_case cc(int form, int split, int KH, int Cin, int Cout, int H, int W, int B)
{
    return { form, split, KH, Cin, Cout, H, W, B, 1, 1, 0, 0, 0, -1, -1, 0, 0, 1, 0, 0 };
}

inline engine_switches switches_of(const conv_case& g)
{
    engine_switches sw;
    sw.c32_bn160 = g.bn160, sw.c32_wk = g.wk, sw.wino_nc = g.nc, sw.wino_tall = g.tall != 0, sw.lane_epilogue = g.lane;
    return sw;
}

// the engine's conv32_params of a layer (lower32_conv, bound): TF "SAME" padding, Cout padded to 64, views with a zero halo.  Pointers are
// never dereferenced by the picker: any non-null value stands for "present".
inline conv32_params make_case(const conv_case& g)
{
    static float buf[1];
    conv32_params p{};
    p.B = g.B, p.H = g.H, p.W = g.W, p.KH = p.KW = g.KH, p.stride = g.stride, p.dil = g.dil;
    p.Cin = g.Cin, p.Cout = g.Cout, p.Cout_pad = round_up(g.Cout, 64);
    const int e = (g.KH - 1) * g.dil + 1;
    p.OH = (g.H + g.stride - 1) / g.stride, p.OW = (g.W + g.stride - 1) / g.stride;
    const int th = (p.OH - 1) * g.stride + e - g.H, tw = (p.OW - 1) * g.stride + e - g.W;
    p.pad_t = th > 0 ? th / 2 : 0, p.pad_l = tw > 0 ? tw / 2 : 0;
    p.npix = p.B * p.OH * p.OW, p.pick_npix = (g.pickB ? g.pickB : g.B) * p.OH * p.OW;
    int rows = g.H + 2 + (g.H & 1); // even
    if (g.view == 1)
        rows += 1;
    if (g.view == 3)
        rows = g.H & ~1;
    p.in.p = buf, p.in.cs = round_up(g.Cin, 32), p.in.wp = g.W + 2, p.in.img = rows * p.in.wp + (g.view == 2 ? 1 : 0);
    p.out = p.in, p.out.cs = round_up(g.Cout, 32), p.out.p = g.out == 2 ? nullptr : buf;
    p.out_f32 = g.out ? buf : nullptr;
    p.lane_epilogue = g.lane, p.latency = g.latency;
    p.w = p.w_frag = p.w_wino = buf, p.w_split = reinterpret_cast<const _Float16*>(buf);
    if (g.dwd)
        p.dw_w = buf, p.dw_dil = g.dwd;
    return p;
}

inline std::string line_of(const conv_case& g)
{
    const conv32_params p = make_case(g);
    conv32_choice c = pick_conv32(p, switches_of(g), (conv32_form)g.form, g.split != 0);
    if (!c.ok) { // (the launcher returns an error: only the profile label is still asked for)
        const int tile = c.tile;
        c = conv32_choice{}, c.tile = tile;
    }
    char s[320];
    std::snprintf(s, sizeof s, "C %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %u %u %d %zu %d %d %d %d %d", g.form, g.split, g.KH,
        g.Cin, g.Cout, g.H, g.W, g.B, g.stride, g.dil, g.out, g.pickB, g.lane, g.bn160, g.wk, g.latency, g.nc, g.tall, g.view, g.dwd, (int)c.ok, (int)c.kernel,
        c.targ[0], c.targ[1], c.targ[2], c.targ[3], c.targ[4], c.grid_x, c.grid_y, c.threads, c.lds, c.tiles_x, c.tiles_y, c.vh, c.rows, c.tile);
    return s;
}

struct head_case {
    int hid, c2, hidb, c2b, same, sw, npix;
};
inline void make_heads(const head_case& g, conv32_params& a, conv32_params& b)
{
    static float buf[2];
    a = conv32_params{};
    a.B = 1, a.H = a.OH = 1, a.W = a.OW = g.npix, a.npix = g.npix, a.Cin = 128, a.Cout = g.c2, a.Cout_pad = 64, a.KH = a.KW = 1, a.stride = a.dil = 1;
    a.in.p = buf, a.in.cs = 128, a.in.wp = g.npix + 2, a.in.img = 4 * a.in.wp, a.out = a.in;
    b = a, b.Cout = g.c2b;
    if (g.same == 0)
        b.in.p = buf + 1;
    if (g.same == 2)
        b.in.coff = 4;
    if (g.same == 3)
        b.npix = b.OW = g.npix - 1;
}
inline std::string line_of(const head_case& g)
{
    conv32_params a, b;
    make_heads(g, a, b);
    engine_switches sw;
    sw.head_pair32 = g.sw != 0;
    conv32_choice c = g.hidb ? pick_head32(a, g.hid, &b, g.hidb) : pick_head32(a, g.hid);
    if (!c.ok) {
        const int tile = c.tile;
        c = conv32_choice{}, c.tile = tile;
    }
    char s[200];
    std::snprintf(s, sizeof s, "H %d %d %d %d %d %d %d : %d %d %d %d %u %d %d %d %d", g.hid, g.c2, g.hidb, g.c2b, g.same, g.sw, g.npix, (int)c.ok, (int)c.kernel, c.targ[0],
        c.targ[1], c.grid_x, c.threads, c.tile, (int)pick32::head_ok(128, g.hid, g.c2), (int)pick32::head_pair_ok(a, b, sw));
    return s;
}

struct form_case {
    int dtype, no_wino, dwf, room, KH, cin, cout, stride;
};
// what lower32_conv hands over: Cin padded to 16, the forms' pointers null; dwf: the depthwise layer's weights set (lower32_dw_in_front)
inline conv32_params make_layer(const form_case& g)
{
    conv_case c = cc(0, 0, g.KH, round_up(g.cin, 16), g.cout, 46, 54, 8);
    c.stride = g.stride;
    conv32_params p = make_case(c);
    p.w_frag = p.w_wino = nullptr, p.w_split = nullptr;
    if (g.dwf)
        p.dw_w = p.w, p.dw_dil = 1;
    return p;
}
inline std::string line_of(const form_case& g)
{
    const conv32_params p = make_layer(g);
    engine_switches sw;
    sw.no_winograd32 = g.no_wino != 0;
    const conv32_forms f = conv32_layer_forms(p, g.dtype, sw, g.dwf != 0, g.room, g.cin);
    conv32_params q = p;
    q.Cin = round_up(g.cin, 64), q.dw_w = nullptr;
    char s[200];
    std::snprintf(s, sizeof s, "F %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d", g.dtype, g.no_wino, g.dwf, g.room, g.KH, g.cin, g.cout, g.stride, (int)f.w_wino,
        (int)f.w_frag, (int)f.w_split, (int)f.kind, f.cin_split, (int)pick32::dw_fusable(q, false, 1), (int)pick32::dw_fusable(q, true, 1));
    return s;
}

// ---- the grid, pruned to blocks that each cross what one group of rules reads
// the built-in networks' own maps and batches, then the tiny maps (smaller than any tile) at batch 1 and 3
static const int MAPS[][3] = { { 46, 54, 8 }, { 92, 108, 8 }, { 184, 216, 8 }, { 96, 96, 32 }, { 48, 48, 32 }, { 24, 24, 32 }, { 12, 12, 32 }, { 54, 96, 16 },
    { 97, 97, 8 }, { 49, 49, 8 }, { 25, 25, 8 }, { 3, 5, 1 }, { 3, 5, 3 } };

struct cases {
    std::vector<conv_case> conv;
    std::vector<head_case> head;
    std::vector<form_case> form;
};

inline cases grid()
{
    cases v;
    auto& C = v.conv;
    // GEMM 1: maps x widths (the tile by block count; the whole-K and short-K rules by Cin / Cout)
    for (auto& m : MAPS)
        for (int co : { 64, 128, 512 }) {
            for (int ci : { 32, 64, 128 })
                C.push_back(cc(C32_GEMM, 0, 1, ci, co, m[0], m[1], m[2]));
            C.push_back(cc(C32_GEMM, 0, 3, 128, co, m[0], m[1], m[2]));
        }
    // GEMM 2: 128-pixel block counts around 448 and 1024 (64 and 128 output rows), b128 > 1024 with b160 on both sides of it; conv32_wk_kernel's
    // block count around 768
    for (int n : { 447 * 128, 447 * 128 + 1, 1023 * 128, 1023 * 128 + 1, 1024 * 128, 1024 * 128 + 1, 1024 * 160, 1024 * 160 + 1 })
        for (int co : { 64, 128 })
            C.push_back(cc(C32_GEMM, 0, 3, 256, co, 1, n, 1));
    for (int n : { 767 * 64, 767 * 64 + 1, 768 * 64 + 1 })
        for (int ci : { 32, 64, 128 })
            C.push_back(cc(C32_GEMM, 0, 1, ci, 64, 1, n, 1));
    // GEMM 3: the switches, the output kinds and a call of fewer frames than max_batch
    for (int mi : { 0, 3, 6 })
        for (int w = 0; w < 2; ++w) {
            const conv_case base = cc(C32_GEMM, 0, 1, w ? 128 : 64, w ? 64 : 256, MAPS[mi][0], MAPS[mi][1], MAPS[mi][2]);
            for (int lane : { -1, 0, 1 })
                for (int bn : { -1, 0, 1 }) {
                    conv_case c = base;
                    c.lane = lane, c.bn160 = bn, C.push_back(c);
                }
            for (int wk : { -1, 0, 1 })
                for (int out : { 0, 1, 2 }) {
                    conv_case c = base;
                    c.wk = wk, c.out = out, C.push_back(c);
                }
            conv_case c = base;
            c.B = 3, c.pickB = MAPS[mi][2], C.push_back(c);
            c.B = 1, C.push_back(c);
        }
    // GEMM 4: strides, dilations, 7 x 7, channel counts off the chunk grid
    for (int sd : { 1, 2, 3 })
        for (int k : { 1, 3, 7 }) {
            conv_case c = cc(C32_GEMM, 0, k, k == 1 ? 256 : 48, 128, 46, 54, 8);
            c.stride = 1 + (sd & 1), c.dil = 1 + (sd >> 1), C.push_back(c);
        }
    // direct 1: both pipes x kernel size x fused dilation x wavefront-group counts (split: 1 2 3 4 6 8 16; fp32: twice that) on four maps
    static const int DK[][2] = { { 1, 0 }, { 1, 1 }, { 1, 2 }, { 3, 0 } };
    for (int split : { 0, 1 })
        for (auto& k : DK)
            for (int co : { 64, 128, 192, 256, 384, 512, 1024 })
                for (int mi : { 0, 3, 6, 12 }) {
                    conv_case c = cc(C32_DIRECT, split, k[0], 128, co, MAPS[mi][0], MAPS[mi][1], MAPS[mi][2]);
                    c.dwd = k[1], C.push_back(c);
                }
    // direct 2: tile counts around 256 / groups (split) and 640 / groups (fp32): 512 outputs = 8 | 16 groups
    for (int split : { 0, 1 })
        for (auto& k : DK)
            for (int t : { 31, 32, 63, 64, 79, 80, 127, 128, 159, 160, 255, 256 }) {
                conv_case c = cc(C32_DIRECT, split, k[0], 64, 512, 8, 8 * t, 1);
                c.dwd = k[1], C.push_back(c);
            }
    // direct 3: fused LDS around 160 KB (40 bytes per depthwise channel behind the tiles), channel counts off the chunk grid, what the form refuses
    for (int split : { 0, 1 })
        for (int dwd : { 1, 2 })
            for (int ci : { 2304, 2368, 2624, 2688, 2944, 3008 })
                for (int mi : { 0, 12 }) {
                    conv_case c = cc(C32_DIRECT, split, 1, ci, 512, MAPS[mi][0], MAPS[mi][1], MAPS[mi][2]);
                    c.dwd = dwd, C.push_back(c);
                }
    for (int split : { 0, 1 })
        for (int k : { 1, 3, 5 })
            for (int ci : { 32, 48, 64, 96 })
                C.push_back(cc(C32_DIRECT, split, k, ci, 64, 46, 54, 8));
    for (int sd : { 1, 2 }) {
        conv_case c = cc(C32_DIRECT, 0, 3, 64, 64, 46, 54, 8);
        c.stride = 1 + (sd & 1), c.dil = 1 + (sd >> 1), C.push_back(c);
    }
    // Winograd 1: maps that are whole 16-row blocks (48) and maps that are not x batch x one or two batches in flight
    static const int WM[][2] = { { 46, 54 }, { 48, 48 }, { 49, 49 }, { 25, 25 }, { 24, 24 }, { 97, 97 }, { 3, 5 } };
    for (auto& m : WM)
        for (int b : { 1, 2, 8 })
            for (int lat : { 0, 1 })
                for (int co : { 128, 512 }) {
                    conv_case c = cc(C32_WINO2, 0, 3, 128, co, m[0], m[1], b);
                    c.latency = lat, C.push_back(c);
                }
    // Winograd 2: the distance between two images (even, odd, not whole rows, less than H + 2) with and without the tall / rows forms
    for (int mi : { 0, 1, 3, 6 })
        for (int b : { 2, 8 })
            for (int view : { 0, 1, 2, 3 })
                for (int tall : { 0, 1 }) {
                    conv_case c = cc(C32_WINO2, 0, 3, 64, 64, WM[mi][0], WM[mi][1], b);
                    c.view = view, c.tall = tall, C.push_back(c);
                }
    // Winograd 3: forced column tiles; NC = 2 block counts around 512; T >= 4 nc on both sides (T = 3 4 7 8)
    for (int nc : { 1, 2 })
        for (int lat : { 0, 1 })
            for (int mi : { 0, 3 })
                for (int b : { 1, 8 }) {
                    conv_case c = cc(C32_WINO2, 0, 3, 64, 128, WM[mi][0], WM[mi][1], b);
                    c.nc = nc, c.latency = lat, C.push_back(c);
                }
    for (int t : { 512, 513 })
        for (int lat : { 0, 1 }) {
            conv_case c = cc(C32_WINO2, 0, 3, 16, 64, 16, 8 * t, 1);
            c.latency = lat, C.push_back(c);
        }
    for (int h : { 6, 7, 14, 15 })
        for (int lat : { 0, 1 }) {
            conv_case c = cc(C32_WINO2, 0, 3, 32, 64, h, 16, 8);
            c.latency = lat, C.push_back(c);
        }
    // Winograd 4: what the form refuses
    {
        conv_case c = cc(C32_WINO2, 0, 3, 64, 64, 46, 54, 8);
        c.stride = 2, C.push_back(c);
        c.stride = 1, c.dil = 2, C.push_back(c);
        c.dil = 1, c.out = 1, C.push_back(c);
        c.out = 2, C.push_back(c);
        c.out = 0, c.Cin = 24, C.push_back(c);
        c.Cin = 64, c.KH = 1, C.push_back(c);
    }
    // heads: outputs around the 32-row tile, hidden widths (192: refused), pairs on the same / another tensor, slice, map; the switch
    for (int hid : { 128, 256, 192, 64 })
        for (int c2 : { 1, 32, 33, 64, 65 })
            for (int n : { 5, 8 * 46 * 54 })
                v.head.push_back({ hid, c2, 0, 0, 1, 1, n });
    for (int c2 : { 19, 38 })
        for (int c2b : { 19, 38, 65 })
            for (int same : { 0, 1, 2, 3 })
                for (int sw : { 0, 1 })
                    if (same == 1 || (sw == 1 && c2b != 65))
                        v.head.push_back({ 128, c2, 256, c2b, same, sw, 8 * 46 * 54 });
    v.head.push_back({ 128, 19, 192, 19, 1, 1, 31 });
    v.head.push_back({ 128, 19, 128, 19, 1, 1, 33 });
    // layer forms: both fp32 engine types x the Winograd switch x a depthwise layer in front x room below / at the padded slice
    static const int FL[][4] = { { 3, 128, 128, 1 }, { 3, 48, 128, 1 }, { 3, 128, 128, 2 }, { 1, 128, 64, 1 }, { 1, 128, 512, 1 }, { 1, 100, 64, 1 } };
    for (int dt : { HP_DTYPE_F32, HP_DTYPE_F32S })
        for (auto& l : FL)
            for (int nw : { 0, 1 })
                for (int dwf : { 0, 1 })
                    for (int short_room : { 0, 1 }) {
                        if (l[0] == 3 ? dwf : nw)
                            continue;
                        const int cin_s = round_up(l[1], l[0] == 1 ? 64 : 32);
                        v.form.push_back({ dt, nw, dwf, cin_s - (short_room ? 16 : 0), l[0], l[1], l[2], l[3] });
                    }
    return v;
}

} // namespace grid32
