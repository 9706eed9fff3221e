// engine_timeline.cpp — stamp buffers of the HP_*_DBG relaunches decoded to text (engine_timeline.hpp).  The stamps are s_memtime values
// (shader cycles) inside a block and the 100 MHz clock across blocks.
#include "engine_timeline.hpp"

#include <algorithm>
#include <map>
#include <vector>

namespace {

// conv32_kernel's residency stamps (HP_DIRECT_DBG): every block's (start, end) on the 100 MHz clock and the CU it ran on (XCC_ID, HW_ID: se_id
// [15:13], sh_id [12], cu_id [11:8]) at h[128 + 3 b], b < 4096
void print_conv32_residency(FILE* f, const unsigned long long* h)
{
    struct blk { unsigned long long t0, t1; unsigned cu; };
    std::vector<blk> bl;
    unsigned long long tmin = ~0ull, tmax = 0;
    for (int b = 0; b < 4096; ++b) {
        const unsigned long long t0 = h[128 + 3 * b], t1 = h[128 + 3 * b + 1], id = h[128 + 3 * b + 2];
        if (!t0 || !t1)
            continue;
        bl.push_back({ t0, t1, (unsigned)(((id >> 32) & 0xf) << 8 | ((id >> 8) & 0xff)) });
        tmin = std::min(tmin, t0), tmax = std::max(tmax, t1);
    }
    if (bl.empty())
        return;
    std::map<unsigned, std::vector<std::pair<unsigned long long, int>>> ev; // per CU: (time, +1 / -1)
    double dsum = 0, dmin = 1e30, dmax = 0;
    for (const auto& b : bl) {
        ev[b.cu].push_back({ b.t0, +1 }), ev[b.cu].push_back({ b.t1, -1 });
        const double d = (b.t1 - b.t0) * 0.01;
        dsum += d, dmin = std::min(dmin, d), dmax = std::max(dmax, d);
    }
    int peak = 0;
    std::map<int, int> blocks_per_cu, peak_hist;
    for (auto& kv : ev) {
        std::sort(kv.second.begin(), kv.second.end());
        int cur = 0, pk = 0;
        for (auto& e2 : kv.second)
            cur += e2.second, pk = std::max(pk, cur);
        peak = std::max(peak, pk), ++peak_hist[pk], ++blocks_per_cu[(int)kv.second.size() / 2];
    }
    fprintf(f, "  residency: %zu blocks on %zu CUs in %.2f us (first start -> last end); block duration %.2f .. %.2f us, mean %.2f; peak resident blocks per CU:",
        bl.size(), ev.size(), (tmax - tmin) * 0.01, dmin, dmax, dsum / bl.size());
    for (auto& kv : peak_hist)
        fprintf(f, " %d x%d", kv.first, kv.second);
    fprintf(f, "; blocks run per CU:");
    for (auto& kv : blocks_per_cu)
        fprintf(f, " %d x%d", kv.first, kv.second);
    fprintf(f, "; active blocks at 10 %% .. 90 %% of the launch:");
    for (int k = 1; k < 10; ++k) {
        const unsigned long long t = tmin + (tmax - tmin) * k / 10;
        int a = 0;
        for (const auto& b : bl)
            a += b.t0 <= t && t < b.t1;
        fprintf(f, " %d", a);
    }
    // block 9 (the one with the s_memtime stamps) on the 100 MHz clock; duration histogram; mean duration per XCD; starts of the late blocks
    fprintf(f, "; block 9: %.2f us", (h[128 + 3 * 9 + 1] - h[128 + 3 * 9]) * 0.01);
    fprintf(f, "; durations (10 bins from min to max):");
    int hist[10] = { 0 };
    for (const auto& b : bl)
        ++hist[std::min(9, (int)(((b.t1 - b.t0) * 0.01 - dmin) / std::max(1e-9, dmax - dmin) * 10))];
    for (int k = 0; k < 10; ++k)
        fprintf(f, " %d", hist[k]);
    double xs[16] = { 0 };
    int xn[16] = { 0 };
    for (const auto& b : bl)
        xs[(b.cu >> 8) & 15] += (b.t1 - b.t0) * 0.01, ++xn[(b.cu >> 8) & 15];
    fprintf(f, "; mean duration per XCD:");
    for (int k = 0; k < 16; ++k)
        if (xn[k])
            fprintf(f, " %.1f", xs[k] / xn[k]);
    double late0 = 1e30, late_d = 0;
    int nlate = 0;
    for (const auto& b : bl)
        if ((b.t0 - tmin) * 0.01 > 5.0)
            late0 = std::min(late0, (b.t0 - tmin) * 0.01), late_d += (b.t1 - b.t0) * 0.01, ++nlate;
    if (nlate)
        fprintf(f, "; %d blocks started later than 5 us after the first (earliest at %.1f us), their mean duration %.2f us", nlate, late0, late_d / nlate);
    fprintf(f, "\n");
}

// (start, end) of the first 1024 blocks on the 100 MHz clock at h[64 + 2 i]: their number, first start -> last end, the spread of their starts and durations
struct block_spans {
    int nb = 0;
    unsigned long long t0 = ~0ull, t1 = 0, smax = 0, dmin = ~0ull, dmax = 0, dsum = 0;
    explicit block_spans(const unsigned long long* h)
    {
        for (int i = 0; i < 1024 && h[64 + 2 * i]; ++i, ++nb) {
            const unsigned long long d = h[65 + 2 * i] - h[64 + 2 * i];
            t0 = std::min(t0, h[64 + 2 * i]), t1 = std::max(t1, h[65 + 2 * i]), smax = std::max(smax, h[64 + 2 * i]);
            dmin = std::min(dmin, d), dmax = std::max(dmax, d), dsum += d;
        }
    }
};

} // namespace

size_t hp::timeline_words(timeline_kind k)
{
    switch (k) {
    case timeline_kind::bneck: return 64 + 2 * 1024;
    case timeline_kind::chain: return 32;
    case timeline_kind::sep: return 64 + 2 * 1024 + 64; // [0, 64) block 0's stamps, then (start, end) of the first 1024 blocks, then wavefront 4 of block 1
    case timeline_kind::wino: return 128;
    case timeline_kind::conv32: return 128 + 3 * 4096;
    default: return 64; // conv, direct
    }
}

void hp::print_timeline(FILE* f, timeline_kind k, const timeline_header& hd, const unsigned long long* h)
{
    auto deltas = [f, h](int from, int to) {
        for (int i = from; i < to && h[i]; ++i)
            fprintf(f, " %llu", h[i] - h[i - 1]);
    };
    switch (k) {
    case timeline_kind::conv:
        fprintf(f, "conv layer %d %d->%d tile %d consumer:", hd.layer, hd.cin, hd.cout, hd.tile);
        deltas(1, 32);
        fprintf(f, " | producer (from consumer start %lld):", (long long)(h[32] - h[0]));
        deltas(33, 64);
        fprintf(f, "\n");
        break;
    case timeline_kind::bneck: { // block 0's phase timeline and the start / end of the first 1024 blocks
        fprintf(f, "bottleneck layer %d variant %d timeline:", hd.layer, hd.tile);
        deltas(1, 60);
        const block_spans b(h);
        if (b.nb)
            fprintf(f, "\n  first %d blocks: %.2f us from first start to last end; block duration %.2f .. %.2f us, mean %.2f", b.nb, (b.t1 - b.t0) * 0.01,
                b.dmin * 0.01, b.dmax * 0.01, b.dsum * 0.01 / b.nb);
        fprintf(f, "\n");
        break;
    }
    case timeline_kind::chain:
        fprintf(f, "chain layer %d variant %d timeline:", hd.layer, hd.tile);
        deltas(1, 32);
        fprintf(f, "\n");
        break;
    case timeline_kind::sep:
        fprintf(f, "sep layer %d C=%d timeline:", hd.layer, hd.cin);
        deltas(1, 40);
        if (h[41])
            fprintf(f, " | total-to-epi0 %llu pass1 %llu epi1 %llu | total %llu", h[41] - h[0], h[42] - h[41], h[43] - h[42], h[43] - h[0]);
        fprintf(f, "\n");
        if (h[2112]) {
            fprintf(f, "  wavefront 4 of block 1:");
            for (int i = 1; i < 40 && h[2112 + i]; ++i)
                fprintf(f, " %llu", h[2112 + i] - h[2112 + i - 1]);
            fprintf(f, "\n");
        }
        if (h[64]) {
            const block_spans b(h);
            fprintf(f, "  %d blocks: first start -> last end %.2f us, starts spread over %.2f us, block duration %.2f .. %.2f us\n", b.nb,
                (b.t1 - b.t0) * 0.01, (b.smax - b.t0) * 0.01, b.dmin * 0.01, b.dmax * 0.01);
        }
        break;
    case timeline_kind::wino:
        fprintf(f, "winograd layer %d %d->%d tile %d cycles [chunk 0 staged | transformed, chunk 1 stored | per chunk: multiplied, next patch stored | epilogue requests | output transform | slab complete | stored]:", hd.layer, hd.cin, hd.cout,
            hd.tile);
        deltas(1, 119);
        fprintf(f, " | s_memtime ticks %llu in %llu ticks of the 100 MHz clock; blocks per CU %d\n", h[121] - h[119], h[122] - h[120], hd.blocks_per_cu);
        break;
    case timeline_kind::direct:
        fprintf(f, "direct layer %d %dx%d %d->%d tile %d cycles [start | staged, multiplied per chunk | stored]:", hd.layer, hd.kh, hd.kw, hd.cin, hd.cout, hd.tile);
        deltas(1, 64);
        fprintf(f, "\n");
        break;
    case timeline_kind::conv32: // start | first tile staged | every 8 K-steps | stored; then every block's residency
        fprintf(f, "conv32 layer %d %dx%d %d->%d tile %d cycles [start | staged | per 8 K-steps | stored]:", hd.layer, hd.kh, hd.kw, hd.cin, hd.cout, hd.tile);
        deltas(1, 128);
        fprintf(f, "\n");
        print_conv32_residency(f, h);
        break;
    }
}
