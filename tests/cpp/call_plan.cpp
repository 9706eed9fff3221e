// Host-only check of csrc/call_plan.hpp, the decisions of one hp_engine_infer_u8 / hp_engine_infer_f32 call as data.  Every combination of
// max_batch {1, 2, 3, 4, 8} x n 0 .. max_batch + 1 x concurrency 1 / 2 x halves_ok x ensemble x captured graphs x host / device x u8 / f32 is
// held to `parent_rules`, a restatement of what infer_common and hp_engine::enqueue did before the header, written in their order (checks;
// ensemble: upload or fl_src, then a device batch of 2n; halves; staging buffer; eager or captured, one range or fork / two / join).  A short
// literal table holds the cases a reader would check by hand.  Prints "OK <checks>".
#include "../../hyperpose_amd/csrc/call_plan.hpp"

#include <cstdint>
#include <cstdio>

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
    int refusal = 0; // 0 none, 1 empty batch, 2 capacity, 3 hp_engine_infer_f32 under the ensemble, 4 capacity of 2n
    int images = 0, nr = 0;
    int b0[2] = {}, cnt[2] = {};
    bool second[2] = {};
    const void *read = nullptr, *fl_src = nullptr;
    const void* first_upload = nullptr;           // host frames that go up on the call's stream before anything else (into flip_in)
    const void* range_upload = nullptr;           // host frames that go up range by range, each on its range's stream
    bool bracket_inside = false, bracket_around = false; // flip_stage / flip_merge in the range's body, or around the fork and the join
    const void* key_ptr = nullptr;
    int key_kind = 0;
};

// the parent's infer_common + hp_engine::enqueue, read top to bottom
static expected parent_rules(int max_batch, int parts, bool halves_ok, bool fl, const void* input, int n, int on_device, int kind)
{
    expected x;
    if (n < 1)
        return x.refusal = 1, x;
    if (n > max_batch)
        return x.refusal = 2, x;
    const void* dev_in = input;
    if (fl) {
        if (kind != 0)
            return x.refusal = 3, x;
        if (2 * n > max_batch)
            return x.refusal = 4, x;
        if (on_device)
            x.fl_src = input;
        else
            x.first_upload = input; // hipMemcpyAsync(flip_in, input, n frames, s)
        dev_in = FLIP_IN, on_device = 1, n *= 2;
    }
    const bool halves = parts == 2 && halves_ok && n >= 2;
    if (!on_device) {
        dev_in = IN_STAGE;      // one range: copied on s in front of the graph launch or by enqueue's h2d; halves: one copy per half on its stream
        x.range_upload = input;
    }
    x.images = n, x.read = dev_in;
    x.bracket_inside = fl && !halves; // `staged`, and the eager branch around a one-range enqueue
    x.bracket_around = fl && halves;
    if (halves) {
        const int n0 = (n + 1) / 2;
        x.nr = 2, x.b0[0] = 0, x.cnt[0] = n0, x.second[0] = false, x.b0[1] = n0, x.cnt[1] = n - n0, x.second[1] = true;
    } else
        x.nr = 1, x.b0[0] = 0, x.cnt[0] = n, x.second[0] = false;
    x.key_ptr = x.fl_src && !halves ? x.fl_src : dev_in;
    x.key_kind = fl ? 2 : kind;
    return x;
}

static int enumerate()
{
    int plans = 0;
    for (int max_batch : { 1, 2, 3, 4, 8 })
        for (int n = 0; n <= max_batch + 1; ++n)
            for (int bits = 0; bits < 64; ++bits) {
                const int parts = 1 + (bits & 1), on_device = bits >> 4 & 1, kind = bits >> 5 & 1;
                const bool halves_ok = bits & 2, fl = bits & 4, graph = bits & 8;
                char what[128];
                std::snprintf(what, sizeof what, "max_batch %d n %d parts %d halves_ok %d ensemble %d graph %d device %d kind %d", max_batch, n, parts, halves_ok, fl, graph,
                    on_device, kind);
                const hp::call_settings cfg{ max_batch, parts, halves_ok, fl, graph };
                const hp::call_args a{ CALLER, n, on_device, kind, nullptr };
                const hp::call_plan p = hp::plan_call(cfg, { IN_STAGE, FLIP_IN }, a);
                const expected x = parent_rules(max_batch, parts, halves_ok, fl, CALLER, n, on_device, kind);
                CHECK((int)p.refusal == x.refusal && p.refusal == hp::refusal_of(cfg, a), "%s: refusal %d, by the parent's rules %d", what, (int)p.refusal, x.refusal);
                if (x.refusal || p.refusal)
                    continue;
                ++plans;
                CHECK(p.images == x.images && p.kind == kind && p.captured == graph && p.ensemble == fl, "%s: %d images (%d), kind %d, captured %d", what, p.images, x.images,
                    p.kind, p.captured);
                CHECK(p.read == x.read && (p.read == IN_STAGE) == hp::reads_in_stage(cfg, a), "%s: the network reads %p, by the parent's rules %p", what, p.read, x.read);
                CHECK(p.fl_src == x.fl_src, "%s: fl_src %p (%p)", what, p.fl_src, x.fl_src);
                // uploads: under the ensemble all frames first, otherwise range by range; never both, and none for a device batch
                CHECK((p.ensemble ? p.host_src : nullptr) == x.first_upload && (p.ensemble ? nullptr : p.host_src) == x.range_upload, "%s: host source %p", what, p.host_src);
                CHECK(p.stage_inside == x.bracket_inside && (p.ensemble && !p.stage_inside) == x.bracket_around, "%s: stage / merge inside %d", what, p.stage_inside);
                CHECK(p.nr == x.nr, "%s: %d ranges (%d)", what, p.nr, x.nr);
                int next = 0;
                for (int i = 0; i < p.nr && i < x.nr; ++i) {
                    const hp::call_range& r = p.ranges[i];
                    CHECK(r.b0 == x.b0[i] && r.cnt == x.cnt[i] && r.second == x.second[i], "%s: range %d is [%d, +%d) second %d", what, i, r.b0, r.cnt, r.second);
                    CHECK(r.b0 == next && r.cnt >= 1, "%s: range %d does not continue at frame %d", what, i, next);
                    next = r.b0 + r.cnt;
                    const hp::graph_key& k = p.keys[i];
                    CHECK(k.n == x.cnt[i] && k.ptr == x.key_ptr && k.kind == x.key_kind && k.b0 == x.b0[i], "%s: key %d is (%d, %p, %d, %d)", what, i, k.n, k.ptr, k.kind, k.b0);
                }
                CHECK(next == p.images && p.images <= max_batch, "%s: the ranges cover %d of %d images", what, next, p.images);
            }
    return plans;
}

// the cases a reader would check by hand
static void by_hand()
{
    const hp::call_buffers buf{ IN_STAGE, FLIP_IN };
    { // batch 3 with concurrency 2: 2 + 1, the second on the second stream
        const hp::call_plan p = hp::plan_call({ 4, 2, true, false, true }, buf, { CALLER, 3, 1, 0, nullptr });
        CHECK(p.refusal == hp::CALL_OK && p.nr == 2 && p.ranges[0].b0 == 0 && p.ranges[0].cnt == 2 && !p.ranges[0].second && p.ranges[1].b0 == 2 && p.ranges[1].cnt == 1
                && p.ranges[1].second,
            "batch 3 is not 2 + 1");
        CHECK(p.keys[0].n == 2 && p.keys[0].b0 == 0 && p.keys[1].n == 1 && p.keys[1].b0 == 2 && p.keys[0].ptr == CALLER && p.keys[1].ptr == CALLER && p.keys[0].kind == 0,
            "batch 3: the halves' keys");
    }
    { // batch 1 with concurrency 2: one range, and the key of a two-frame call's first half
        const hp::call_plan p = hp::plan_call({ 4, 2, true, false, true }, buf, { CALLER, 1, 1, 0, nullptr });
        const hp::call_plan q = hp::plan_call({ 4, 2, true, false, true }, buf, { CALLER, 2, 1, 0, nullptr });
        CHECK(p.nr == 1 && p.ranges[0].cnt == 1 && !p.ranges[0].second, "batch 1 with concurrency 2 is not one range");
        CHECK(q.nr == 2 && !(p.keys[0] < q.keys[0]) && !(q.keys[0] < p.keys[0]), "batch 1 does not share the key of batch 2's first half");
    }
    { // concurrency 2 on an engine without half-batches (fp16, int8): one range
        const hp::call_plan p = hp::plan_call({ 4, 2, false, false, true }, buf, { CALLER, 4, 1, 0, nullptr });
        CHECK(p.nr == 1 && p.ranges[0].cnt == 4, "halves on an engine that has none");
    }
    { // ensemble + device + one stream: 2n images of flip_in, flip and merge inside, keyed by the CALLER's pointer with kind 2
        const hp::call_plan p = hp::plan_call({ 4, 1, true, true, true }, buf, { CALLER, 2, 1, 0, nullptr });
        CHECK(p.images == 4 && p.nr == 1 && p.read == FLIP_IN && p.fl_src == CALLER && p.stage_inside && !p.host_src, "ensemble, device, one stream: the plan");
        CHECK(p.keys[0].n == 4 && p.keys[0].ptr == CALLER && p.keys[0].kind == 2 && p.keys[0].b0 == 0, "ensemble, device, one stream: keyed by %p", p.keys[0].ptr);
    }
    { // ensemble + halves: the frames are the first half, their flips the second; flip and merge around; keyed by flip_in
        const hp::call_plan p = hp::plan_call({ 4, 2, true, true, true }, buf, { CALLER, 2, 1, 0, nullptr });
        CHECK(p.images == 4 && p.nr == 2 && p.ranges[0].cnt == 2 && p.ranges[1].b0 == 2 && p.ranges[1].cnt == 2 && !p.stage_inside && p.fl_src == CALLER,
            "ensemble, two halves: the plan");
        CHECK(p.keys[0].ptr == FLIP_IN && p.keys[1].ptr == FLIP_IN && p.keys[0].kind == 2 && p.keys[1].kind == 2, "ensemble, two halves: keyed by %p", p.keys[0].ptr);
    }
    { // ensemble + host: the frames go up into flip_in first; no fl_src; keyed by flip_in
        const hp::call_plan p = hp::plan_call({ 4, 1, true, true, true }, buf, { CALLER, 2, 0, 0, nullptr });
        CHECK(p.host_src == CALLER && !p.fl_src && p.read == FLIP_IN && p.keys[0].ptr == FLIP_IN && p.keys[0].kind == 2 && p.stage_inside, "ensemble, host batch");
    }
    { // host batch: staged in in_stage, which is the key, for either entry
        const hp::call_plan p = hp::plan_call({ 4, 2, true, false, true }, buf, { CALLER, 4, 0, 1, nullptr });
        CHECK(p.read == IN_STAGE && p.host_src == CALLER && p.nr == 2 && p.keys[0].ptr == IN_STAGE && p.keys[1].ptr == IN_STAGE && p.keys[0].kind == 1, "host batch, f32 entry");
    }
    { // the refusals, in the order they are tested
        CHECK(hp::refusal_of({ 4, 1, true, true, true }, { CALLER, 0, 0, 1, nullptr }) == hp::CALL_EMPTY, "empty batch");
        CHECK(hp::refusal_of({ 4, 1, true, true, true }, { CALLER, 5, 0, 1, nullptr }) == hp::CALL_OVERFLOW, "capacity before the entry");
        CHECK(hp::refusal_of({ 4, 1, true, true, true }, { CALLER, 3, 0, 1, nullptr }) == hp::CALL_F32_ENSEMBLE, "the entry before the capacity of 2n");
        CHECK(hp::refusal_of({ 4, 1, true, true, true }, { CALLER, 3, 0, 0, nullptr }) == hp::CALL_ENSEMBLE_OVERFLOW, "capacity of 2n");
        CHECK(hp::refusal_of({ 4, 1, true, true, true }, { CALLER, 2, 0, 0, nullptr }) == hp::CALL_OK, "2n == max_batch fits");
    }
}

int main()
{
    const int plans = enumerate();
    by_hand();
    if (g_fail) {
        std::printf("FAILED %d of %d\n", g_fail, g_checks);
        return 1;
    }
    std::printf("plans %d\nOK %d\n", plans, g_checks);
    return 0;
}
