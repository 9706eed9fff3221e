// Host-only check of csrc/call_plan.hpp with the scale ensemble (call_settings::scales = K).  Every combination of max_batch {1, 2, 3, 4, 8, 12} x
// n 0 .. max_batch + 1 x K 1 .. 4 x flip x concurrency 1 / 2 x halves_ok x captured graphs x host / device x u8 / f32 is held to `rules`, the
// plan restated from include/hp_hip.h ("scale ensemble") and the header's own comment: refusals in their order, (flip ? 2 : 1) * K * n images of
// flip_in covering exactly the ranges, stage and merge inside one range or around two, the uploads, the keys.  With K == 1 every plan equals,
// field by field, the plan of a call_settings that leaves `scales` at its default; the keys of one call differ across (flip, K).  Prints "OK <checks>".
#include "../../hyperpose_amd/csrc/call_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

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

static const void* const IN_STAGE = (const void*)(uintptr_t)0x7f0000100000ull;
static const void* const FLIP_IN = (const void*)(uintptr_t)0x7f0000200000ull;
static const void* const CALLER = (const void*)(uintptr_t)0x7f0000300000ull;

struct expected {
    hp::call_refusal refusal = hp::CALL_OK;
    int images = 0, nr = 0, b0[2] = {}, cnt[2] = {};
    const void *read = nullptr, *fl_src = nullptr, *host_src = nullptr;
    bool staged = false, inside = false;
    const void* key_ptr = nullptr;
    int key_kind = 0;
};

static expected rules(int max_batch, int parts, bool halves_ok, bool flip, int K, int n, int on_device, int kind)
{
    expected x;
    if (n < 1)
        return x.refusal = hp::CALL_EMPTY, x;
    if (n > max_batch)
        return x.refusal = hp::CALL_OVERFLOW, x;
    x.staged = flip || K > 1;
    if (x.staged && kind != 0)
        return x.refusal = hp::CALL_F32_ENSEMBLE, x;
    x.images = (flip ? 2 : 1) * K * n;
    if (x.images > max_batch)
        return x.refusal = hp::CALL_ENSEMBLE_OVERFLOW, x;
    x.read = x.staged ? FLIP_IN : on_device ? CALLER : IN_STAGE;
    x.host_src = on_device ? nullptr : CALLER;
    x.fl_src = x.staged && on_device ? CALLER : nullptr;
    const bool halves = parts == 2 && halves_ok && x.images >= 2;
    x.nr = halves ? 2 : 1;
    x.b0[0] = 0, x.cnt[0] = halves ? (x.images + 1) / 2 : x.images;
    x.b0[1] = x.cnt[0], x.cnt[1] = x.images - x.cnt[0];
    x.inside = x.staged && !halves;
    x.key_ptr = x.fl_src && !halves ? x.fl_src : x.read;
    x.key_kind = K == 1 ? (flip ? 2 : kind) : (flip ? 4 : 1) + K; // 3 .. 5 and 6 .. 8: none of the kinds 0, 1, 2 of the parent
    return x;
}

static bool same_plan(const hp::call_plan& a, const hp::call_plan& b)
{
    bool same = a.refusal == b.refusal;
    if (same && a.refusal == hp::CALL_OK) {
        same = a.kind == b.kind && a.images == b.images && a.read == b.read && a.host_src == b.host_src && a.fl_src == b.fl_src && a.ensemble == b.ensemble
            && a.stage_inside == b.stage_inside && a.captured == b.captured && a.nr == b.nr && a.scales == b.scales && a.staged == b.staged;
        for (int i = 0; i < a.nr && same; ++i)
            same = a.ranges[i].b0 == b.ranges[i].b0 && a.ranges[i].cnt == b.ranges[i].cnt && a.ranges[i].second == b.ranges[i].second && !(a.keys[i] < b.keys[i])
                && !(b.keys[i] < a.keys[i]);
    }
    return same;
}

static int enumerate()
{
    int plans = 0;
    for (int max_batch : { 1, 2, 3, 4, 8, 12 })
        for (int n = 0; n <= max_batch + 1; ++n)
            for (int bits = 0; bits < 64; ++bits) {
                const int parts = 1 + (bits & 1), on_device = bits >> 4 & 1, kind = bits >> 5 & 1;
                const bool halves_ok = bits & 2, flip = bits & 4, graph = bits & 8;
                const hp::call_args a{ CALLER, n, on_device, kind, nullptr };
                std::set<std::tuple<int, const void*, int, int>> keys_of_call; // (flip, K) -> this call's first key: all distinct
                for (int K = 1; K <= 4; ++K) {
                    char what[160];
                    std::snprintf(what, sizeof what, "max_batch %d n %d K %d flip %d parts %d halves_ok %d graph %d device %d kind %d", max_batch, n, K, flip, parts,
                        halves_ok, graph, on_device, kind);
                    hp::call_settings cfg{ max_batch, parts, halves_ok, flip, graph };
                    cfg.scales = K;
                    const hp::call_plan p = hp::plan_call(cfg, { IN_STAGE, FLIP_IN }, a);
                    const expected x = rules(max_batch, parts, halves_ok, flip, K, n, on_device, kind);
                    CHECK(p.refusal == x.refusal && p.refusal == hp::refusal_of(cfg, a), "%s: refusal %d, by the rules %d", what, (int)p.refusal, (int)x.refusal);
                    if (K == 1) { // the plan of today: a call_settings that does not name the field
                        const hp::call_settings old{ max_batch, parts, halves_ok, flip, graph };
                        CHECK(same_plan(p, hp::plan_call(old, { IN_STAGE, FLIP_IN }, a)), "%s: K = 1 is not the plan of a call_settings without the field", what);
                    }
                    if (x.refusal != hp::CALL_OK || p.refusal != hp::CALL_OK)
                        continue;
                    ++plans;
                    CHECK(p.images == x.images && p.images == hp::images_of(cfg, n) && p.scales == K && p.staged == x.staged && p.ensemble == flip && p.kind == kind
                            && p.captured == graph,
                        "%s: %d images (%d), scales %d, staged %d", what, p.images, x.images, p.scales, p.staged);
                    CHECK(p.read == x.read && (p.read == IN_STAGE) == hp::reads_in_stage(cfg, a), "%s: the network reads %p (%p)", what, p.read, x.read);
                    CHECK(p.host_src == x.host_src && p.fl_src == x.fl_src, "%s: host_src %p fl_src %p", what, p.host_src, p.fl_src);
                    // stage and merge: inside the one range's body, or around the fork and the join of two; never without an ensemble
                    CHECK(p.stage_inside == x.inside && (p.staged && !p.stage_inside) == (x.staged && x.nr == 2), "%s: stage / merge inside %d", what, p.stage_inside);
                    CHECK(p.nr == x.nr, "%s: %d ranges (%d)", what, p.nr, x.nr);
                    int next = 0;
                    for (int i = 0; i < p.nr && i < x.nr; ++i) {
                        const hp::call_range& r = p.ranges[i];
                        CHECK(r.b0 == x.b0[i] && r.cnt == x.cnt[i] && r.second == (i == 1) && r.b0 == next && r.cnt >= 1, "%s: range %d is [%d, +%d)", what, i, r.b0,
                            r.cnt);
                        next = r.b0 + r.cnt;
                        const hp::graph_key& k = p.keys[i];
                        CHECK(k.n == r.cnt && k.b0 == r.b0 && k.ptr == x.key_ptr && k.kind == x.key_kind, "%s: key %d is (%d, %p, %d, %d)", what, i, k.n, k.ptr,
                            k.kind, k.b0);
                    }
                    CHECK(next == p.images && p.images <= max_batch, "%s: the ranges cover %d of %d images (max_batch %d)", what, next, p.images, max_batch);
                    const hp::graph_key& k0 = p.keys[0];
                    CHECK(keys_of_call.insert(std::make_tuple(k0.n, k0.ptr, k0.kind, k0.b0)).second, "%s: a key shared with another K", what);
                }
            }
    return plans;
}

// keys across (flip, K) on the same call: the kinds alone differ, so two settings never share a graph
static void distinct_kinds()
{
    std::set<int> kinds = { 0, 1 }; // the parent's plain kinds
    for (int flip = 0; flip < 2; ++flip)
        for (int K = 1; K <= 4; ++K) {
            if (!flip && K == 1)
                continue;
            hp::call_settings cfg{ 64, 1, true, flip != 0, true };
            cfg.scales = K;
            const hp::call_plan p = hp::plan_call(cfg, { IN_STAGE, FLIP_IN }, { CALLER, 2, 1, 0, nullptr });
            CHECK(p.refusal == hp::CALL_OK && kinds.insert(p.keys[0].kind).second, "flip %d K %d: key kind %d is in use", flip, K, p.keys[0].kind);
        }
    CHECK(kinds.size() == 9, "%zu kinds", kinds.size());
}

// the cases a reader would check by hand
static void by_hand()
{
    const hp::call_buffers buf{ IN_STAGE, FLIP_IN };
    hp::call_settings s{ 8, 1, true, false, true };
    s.scales = 2;
    { // K = 2, device, one stream: 2n images of flip_in, stage and merge inside, keyed by the caller's pointer with kind 3
        const hp::call_plan p = hp::plan_call(s, buf, { CALLER, 4, 1, 0, nullptr });
        CHECK(p.refusal == hp::CALL_OK && p.images == 8 && p.nr == 1 && p.read == FLIP_IN && p.fl_src == CALLER && p.stage_inside && p.keys[0].kind == 3
                && p.keys[0].ptr == CALLER,
            "K = 2, device, one stream");
        CHECK(hp::plan_call(s, buf, { CALLER, 5, 1, 0, nullptr }).refusal == hp::CALL_ENSEMBLE_OVERFLOW, "K = 2: 10 images > 8");
    }
    { // K = 2 and the flip: 4n images, the flips behind the K n slots; two halves of 2n, stage and merge around the fork and the join
        hp::call_settings t = s;
        t.ensemble = true, t.parts = 2;
        const hp::call_plan p = hp::plan_call(t, buf, { CALLER, 2, 0, 0, nullptr });
        CHECK(p.refusal == hp::CALL_OK && p.images == 8 && p.nr == 2 && p.ranges[0].cnt == 4 && p.ranges[1].b0 == 4 && !p.stage_inside && p.host_src == CALLER
                && !p.fl_src && p.keys[0].kind == 6 && p.keys[0].ptr == FLIP_IN,
            "K = 2 with the flip, two halves");
        CHECK(hp::plan_call(t, buf, { CALLER, 3, 0, 0, nullptr }).refusal == hp::CALL_ENSEMBLE_OVERFLOW, "K = 2 with the flip: 12 images > 8");
    }
    { // the refusals, in the order they are tested: empty, capacity of n, the f32 entry, capacity of the images
        hp::call_settings t = s;
        t.scales = 4;
        CHECK(hp::refusal_of(t, { CALLER, 0, 0, 1, nullptr }) == hp::CALL_EMPTY, "empty batch");
        CHECK(hp::refusal_of(t, { CALLER, 9, 0, 1, nullptr }) == hp::CALL_OVERFLOW, "capacity of n before the entry");
        CHECK(hp::refusal_of(t, { CALLER, 3, 0, 1, nullptr }) == hp::CALL_F32_ENSEMBLE, "the entry before the capacity of K n");
        CHECK(hp::refusal_of(t, { CALLER, 1, 0, 1, nullptr }) == hp::CALL_F32_ENSEMBLE, "f32 refused even where K n fits");
        CHECK(hp::refusal_of(t, { CALLER, 3, 0, 0, nullptr }) == hp::CALL_ENSEMBLE_OVERFLOW, "capacity of K n");
        CHECK(hp::refusal_of(t, { CALLER, 2, 0, 0, nullptr }) == hp::CALL_OK, "K n == max_batch fits");
    }
}

int main()
{
    const int plans = enumerate();
    distinct_kinds();
    by_hand();
    if (g_fail) {
        std::printf("FAILED %d of %d\n", g_fail, g_checks);
        return 1;
    }
    std::printf("plans %d\nOK %d\n", plans, g_checks);
    return 0;
}
