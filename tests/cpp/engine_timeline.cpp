// Host-only check of csrc/engine_timeline.cpp, the text of the HP_CONV_DBG / HP_BN_DBG / HP_CHAIN_DBG / HP_SEP_DBG / HP_DIRECT_DBG block
// timelines (tools/*_timeline.py users diff these lines).
//   engine_timeline.bin GOLDEN    the text of every case below equals tests/golden/engine_timelines.txt byte for byte.  That file was recorded
//                                 from the printing code as it stood inside engine.cpp (hp_engine::print_timeline, print_conv32_residency,
//                                 block_spans) on the same buffers, before it moved into its own unit
//   engine_timeline.bin --print   prints the text as the unit gives it now (to record a deliberate change)
// Every case is a line "== name" followed by what the printer writes for one synthetic stamp buffer.
#include "../../hyperpose_amd/csrc/engine_timeline.cpp"

#include <cstring>
#include <string>

using hp::timeline_kind;
using stamps = std::vector<unsigned long long>;
typedef void (*printer)(FILE*, timeline_kind, const hp::timeline_header&, const unsigned long long*);

static const timeline_kind KINDS[] = { timeline_kind::conv, timeline_kind::bneck, timeline_kind::chain, timeline_kind::sep, timeline_kind::wino,
    timeline_kind::direct, timeline_kind::conv32 };
static const char* const NAMES[] = { "conv", "bneck", "chain", "sep", "wino", "direct", "conv32" };
static const hp::timeline_header HD = { 7, 128, 256, 3, 3, 35003004, 2 };

static unsigned long long g_seed;
static unsigned rnd(unsigned n) // deterministic, the same on every platform
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_seed >> 33) % n;
}

// stamps [from, to) of one block: a start and growing cycle counts behind it
static void phases(stamps& h, int from, int to)
{
    unsigned long long t = 1000000 + rnd(1000);
    for (int i = from; i < to; ++i)
        h[i] = t, t += 100 + rnd(900);
}
// (start, end) of nb blocks on the 100 MHz clock at h[64 + 2 i] (block_spans)
static void spans(stamps& h, int nb)
{
    for (int i = 0; i < nb; ++i) {
        h[64 + 2 * i] = 5000000 + rnd(2000);
        h[65 + 2 * i] = h[64 + 2 * i] + 500 + rnd(1500);
    }
}
// conv32_kernel's residency records at h[128 + 3 b]: nb blocks over `xcds` XCDs of 32 CUs; every `late_every`-th block starts `late` ticks
// of the 100 MHz clock after the others; dur = 0: random durations
static void residency(stamps& h, int nb, int xcds, int late_every, unsigned late, unsigned dur)
{
    for (int b = 0; b < nb; ++b) {
        const unsigned long long t0 = 7000000 + rnd(300) + (late_every && b % late_every == late_every - 1 ? late : 0);
        const unsigned long long xcd = b % xcds, cu = (b / xcds) % 32; // cu: HW_ID bits [15:8] (se_id, sh_id, cu_id)
        h[128 + 3 * b] = t0, h[128 + 3 * b + 1] = t0 + (dur ? dur : 2000 + rnd(3000)), h[128 + 3 * b + 2] = xcd << 32 | cu << 8;
    }
}

static stamps typical(timeline_kind k)
{
    stamps h(hp::timeline_words(k), 0);
    switch (k) {
    case timeline_kind::conv: phases(h, 0, 30), phases(h, 32, 60); break; // consumer, producer: each ends at its first zero
    case timeline_kind::bneck: phases(h, 0, 50), spans(h, 300); break;
    case timeline_kind::chain: phases(h, 0, 32); break; // (no zero inside the buffer: the loop ends at `to`)
    case timeline_kind::sep: phases(h, 0, 44), spans(h, 700), phases(h, 2112, 2112 + 30); break;
    case timeline_kind::wino: phases(h, 0, 100), h[119] = 500, h[120] = 9000, h[121] = 210500, h[122] = 19000; break;
    case timeline_kind::direct: phases(h, 0, 64); break;
    case timeline_kind::conv32: phases(h, 0, 128), residency(h, 1000, 8, 0, 0, 0); break;
    }
    return h;
}

static void run_cases(FILE* f, printer print)
{
    auto one = [&](const std::string& name, timeline_kind k, const stamps& h) {
        std::fprintf(f, "== %s\n", name.c_str());
        std::fflush(f);
        print(f, k, HD, h.data());
        std::fflush(f);
    };
    g_seed = 20240607;
    for (int i = 0; i < 7; ++i) {
        if (KINDS[i] == timeline_kind::wino) // (a kind that stood here, F(3 x 3) Winograd, drew 41 numbers: the recorded texts behind it keep theirs)
            for (int d = 0; d < 41; ++d)
                rnd(1);
        one(std::string(NAMES[i]) + " typical", KINDS[i], typical(KINDS[i]));
        one(std::string(NAMES[i]) + " all zero", KINDS[i], stamps(hp::timeline_words(KINDS[i]), 0));
    }
    // the residency printer: one block; every block of the buffer over 3 XCDs, a quarter of them starting 8 us late; all durations equal
    // (the histogram's dmax == dmin guard)
    stamps h(hp::timeline_words(timeline_kind::conv32), 0);
    residency(h, 1, 1, 0, 0, 0);
    one("conv32 residency of 1 block", timeline_kind::conv32, h);
    residency(h, 4096, 3, 4, 800, 0);
    one("conv32 residency of 4096 blocks on 3 XCDs, late starters", timeline_kind::conv32, h);
    residency(h, 4096, 8, 0, 0, 2500);
    one("conv32 residency with equal durations", timeline_kind::conv32, h);
    // block_spans through both kinds that print it: 0, 1 and 1024 blocks (0 blocks and a live block 0)
    for (int nb : { 0, 1, 1024 })
        for (int i : { 1, 3 }) {
            stamps b(hp::timeline_words(KINDS[i]), 0);
            phases(b, 0, 20), spans(b, nb);
            one(std::string(NAMES[i]) + " spans of " + std::to_string(nb) + " blocks", KINDS[i], b);
        }
}

static std::string slurp(FILE* f)
{
    std::string s;
    char buf[4096];
    std::rewind(f);
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;)
        s.append(buf, n);
    return s;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "--print")) {
        run_cases(stdout, hp::print_timeline);
        return 0;
    }
    if (argc != 2) {
        std::printf("usage: %s GOLDEN | --print\n", argv[0]);
        return 2;
    }
    FILE* g = std::fopen(argv[1], "rb");
    FILE* t = std::tmpfile();
    if (!g || !t) {
        std::printf("cannot open %s or a temporary file\n", argv[1]);
        return 2;
    }
    run_cases(t, hp::print_timeline);
    const std::string want = slurp(g), got = slurp(t);
    size_t cases = 0, at = 0;
    while (at < want.size() && at < got.size() && want[at] == got[at])
        ++at;
    for (size_t p = 0; (p = want.find("== ", p)) != std::string::npos; ++p)
        cases += p == 0 || want[p - 1] == '\n';
    if (want != got) {
        const size_t from = want.rfind("\n== ", at) == std::string::npos ? 0 : want.rfind("\n== ", at) + 1;
        std::printf("FAIL: the text differs from %s at byte %zu, in case \"%s\"\n  recorded: ...%s\n  printed:  ...%s\n", argv[1], at,
            want.substr(from + 3, want.find('\n', from) - from - 3).c_str(), want.substr(at < 60 ? 0 : at - 60, 120).c_str(), got.substr(at < 60 ? 0 : at - 60, 120).c_str());
        return 1;
    }
    std::printf("OK %zu %zu\n", cases, got.size());
    return 0;
}
