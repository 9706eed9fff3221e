// Host-only check of csrc/graph_cache.hpp, the cache of captured-graph executables that hp_engine's run_call, drop_graphs and destructor
// use.  The executables are integers; a ledger records for each: created, in flight on stream k, destroyed.  `engine_sim` replays the
// engine's call: one acquire() for all keys of the call (the whole batch, or its two halves with concurrency 2), then one launch per
// executable on its stream; now and then a stream or the device is synchronised, or a setting changes (drop).  The ledger reports
//   a launch of a destroyed handle, a destroy of a handle in flight, a double destroy, a leak at the end, a size above the bound,
//   and any eviction, synchronisation or capture on a call whose keys all hit.
// The keys of a call are the engine's own: csrc/call_plan.hpp plans every simulated call, device or host batch, flip ensemble on or off.
// Seeded key streams: one or two keys per call, pointer pools of 1, 8, 33, 64, 65 and 200, n = 1 .. 8, both entries, three streams, drops,
// once with plain device batches alone and once mixed with host batches and the ensemble, and sequences that sit exactly at the bound.  So that the checker cannot go blind, `parent_sim` restates the order the engine had before
// this header (look up the first half; look up the second and, on a miss above the bound, synchronise three streams and destroy everything;
// launch the first half) and runs through the same ledger: it MUST report a launch of a destroyed handle, and a destroy of a handle in
// flight on a caller's stream.  Prints "OK <checks>".
#include "../../hyperpose_amd/csrc/call_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

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

enum { S_OWN = 0, S_SECOND = 1, S_A = 2, S_B = 3, N_STREAMS = 4 };
static constexpr size_t BOUND = 64;

struct ledger {
    struct rec {
        hp::graph_key key;
        int destroyed = 0;
        bool in_flight[N_STREAMS] = {};
    };
    std::vector<rec> h; // handle = index + 1 (0 is "no executable")
    int created = 0, destroys = 0, device_syncs = 0;
    // what it reports
    int launch_of_destroyed = 0, destroy_in_flight = 0, double_destroy = 0, unknown_handle = 0;

    int create(const hp::graph_key& k)
    {
        h.push_back(rec{ k });
        ++created;
        return (int)h.size();
    }
    bool known(int x) const { return x >= 1 && x <= (int)h.size(); }
    void launch(int x, int stream)
    {
        if (!known(x)) {
            ++unknown_handle;
            return;
        }
        if (h[x - 1].destroyed)
            ++launch_of_destroyed;
        h[x - 1].in_flight[stream] = true;
    }
    void destroy(int x)
    {
        if (!known(x)) {
            ++unknown_handle;
            return;
        }
        rec& r = h[x - 1];
        ++destroys;
        if (r.destroyed++)
            ++double_destroy;
        for (bool f : r.in_flight)
            if (f) {
                ++destroy_in_flight;
                break;
            }
    }
    void sync_stream(int stream)
    {
        for (rec& r : h)
            r.in_flight[stream] = false;
    }
    int sync_device()
    {
        ++device_syncs;
        for (int s = 0; s < N_STREAMS; ++s)
            sync_stream(s);
        return 0;
    }
    int live() const
    {
        int n = 0;
        for (const rec& r : h)
            n += r.destroyed == 0;
        return n;
    }
    int leaks() const { return live(); }                                             // at the end: created and never destroyed
    int faults() const { return launch_of_destroyed + destroy_in_flight + double_destroy + unknown_handle; }
    // the live handle of a key, 0 if none: the checker's own view, built from create / destroy alone
    int live_handle(const hp::graph_key& k) const
    {
        for (size_t i = h.size(); i-- > 0;)
            if (!h[i].destroyed && !(h[i].key < k) && !(k < h[i].key))
                return (int)i + 1;
        return 0;
    }
};

struct fake_destroy {
    ledger* L;
    void operator()(int x) const { L->destroy(x); }
};
using cache_t = hp::graph_cache<int, fake_destroy>;
static_assert(cache_t::bound == BOUND, "the issue keeps the bound at 64");

static const void* ptr_of(int i) { return (const void*)(uintptr_t)(0x7f0000001000ull + 4608ull * (unsigned)i); }

// the keys of one call and the streams of their launches, as the engine forms them: csrc/call_plan.hpp, for an fp32 engine (half-batches
// allowed) of max_batch 16 with captured graphs on, its staging buffer and its flip buffer at two addresses no pool pointer has
static const void* const IN_STAGE = (const void*)(uintptr_t)0x7e0000001000ull;
static const void* const FLIP_IN = (const void*)(uintptr_t)0x7e0000002000ull;
static int keys_of(const void* p, int n, int kind, int parts, hp::graph_key keys[2], int streams[2], int s, bool ensemble = false, bool on_device = true)
{
    const hp::call_plan plan = hp::plan_call({ 16, parts, true, ensemble, true }, { IN_STAGE, FLIP_IN }, { p, n, on_device, kind, nullptr });
    CHECK(plan.refusal == hp::CALL_OK, "a simulated call of %d frames, kind %d, was refused (%d)", n, kind, (int)plan.refusal);
    for (int i = 0; i < plan.nr; ++i)
        keys[i] = plan.keys[i], streams[i] = plan.ranges[i].second ? S_SECOND : s;
    return plan.nr;
}

// ---- the engine's order: graph_cache.hpp as run_call, drop_graphs and the destructor use it
struct engine_sim {
    ledger& L;
    cache_t cache;
    int parts = 1;
    bool ensemble = false; // hp_engine_set_flip_ensemble
    int fail_make_at = -1; // make(i) fails for this i (a capture that fails)
    explicit engine_sim(ledger& l)
        : L(l)
        , cache(fake_destroy{ &l })
    {
    }
    int call(const void* p, int n, int kind, int s, bool on_device = true)
    {
        hp::graph_key keys[2];
        int streams[2], out[2] = { 0, 0 };
        const int nk = keys_of(p, n, kind, parts, keys, streams, s, ensemble, on_device);
        int want[2];
        bool all_hit = true;
        for (int i = 0; i < nk; ++i)
            want[i] = L.live_handle(keys[i]), all_hit = all_hit && want[i] != 0;
        const int created = L.created, destroys = L.destroys, syncs = L.device_syncs;
        const size_t before = cache.size();
        const int rc = cache.acquire(
            keys, nk, out, [&](int i, int* made) { return i == fail_make_at ? -7 : (*made = L.create(keys[i]), 0); }, [&] { return L.sync_device(); });
        CHECK(cache.size() <= BOUND, "%zu entries after a call", cache.size());
        CHECK((int)cache.size() == L.live(), "%zu entries, %d live executables", cache.size(), L.live());
        if (all_hit) {
            CHECK(rc == 0 && L.created == created && L.destroys == destroys && L.device_syncs == syncs && cache.size() == before,
                "a call whose keys all hit: rc %d, %d captures, %d destroys, %d synchronisations", rc, L.created - created, L.destroys - destroys, L.device_syncs - syncs);
            for (int i = 0; i < nk; ++i)
                CHECK(out[i] == want[i], "key %d: handle %d, cached %d", i, out[i], want[i]);
        } else {
            CHECK(L.device_syncs - syncs == (L.destroys > destroys ? 1 : 0), "%d synchronisations for %d destroys", L.device_syncs - syncs, L.destroys - destroys);
            CHECK(L.destroys == destroys || L.destroys - destroys == (int)before, "an eviction destroyed %d of %zu", L.destroys - destroys, before);
            // an eviction happens exactly when the missing keys do not fit
            int missing = 0;
            for (int i = 0; i < nk; ++i)
                missing += want[i] == 0;
            CHECK((L.destroys > destroys) == (before + missing > BOUND), "%zu cached + %d missing: %d destroyed", before, missing, L.destroys - destroys);
        }
        if (rc != 0)
            return rc;
        for (int i = 0; i < nk; ++i) {
            CHECK(out[i] == L.live_handle(keys[i]), "key %d: handle %d is not the live one (%d)", i, out[i], L.live_handle(keys[i]));
            L.launch(out[i], streams[i]);
        }
        return 0;
    }
    void drop()
    {
        const int syncs = L.device_syncs;
        CHECK(cache.drop([&] { return L.sync_device(); }) == 0 && cache.size() == 0 && L.live() == 0 && L.device_syncs == syncs + 1, "drop left %zu entries", cache.size());
    }
};

// ---- the order before graph_cache.hpp, restated: one look-up per half, eviction inside the second, launches afterwards
struct parent_sim {
    ledger& L;
    std::map<hp::graph_key, int> graphs;
    int parts = 1;
    explicit parent_sim(ledger& l)
        : L(l)
    {
    }
    int graph_for(const hp::graph_key& key, int s)
    {
        auto it = graphs.find(key);
        if (it == graphs.end()) {
            const int exec = L.create(key);
            if (graphs.size() > 64) {
                L.sync_stream(s), L.sync_stream(S_OWN), L.sync_stream(S_SECOND);
                for (auto& g : graphs)
                    L.destroy(g.second);
                graphs.clear();
            }
            it = graphs.emplace(key, exec).first;
        }
        return it->second;
    }
    void call(const void* p, int n, int kind, int s)
    {
        hp::graph_key keys[2];
        int streams[2], out[2];
        const int nk = keys_of(p, n, kind, parts, keys, streams, s);
        for (int i = 0; i < nk; ++i)
            out[i] = graph_for(keys[i], s);
        for (int i = 0; i < nk; ++i)
            L.launch(out[i], streams[i]);
    }
    void destroy()
    {
        L.sync_stream(S_OWN);
        for (auto& g : graphs)
            L.destroy(g.second);
        graphs.clear();
    }
};

static void expect_clean(const ledger& L, const char* what)
{
    CHECK(L.launch_of_destroyed == 0, "%s: %d launches of a destroyed executable", what, L.launch_of_destroyed);
    CHECK(L.destroy_in_flight == 0, "%s: %d executables destroyed in flight", what, L.destroy_in_flight);
    CHECK(L.double_destroy == 0, "%s: %d double destroys", what, L.double_destroy);
    CHECK(L.unknown_handle == 0, "%s: %d handles the ledger never made", what, L.unknown_handle);
    CHECK(L.leaks() == 0, "%s: %d executables never destroyed", what, L.leaks());
    CHECK(L.created == L.destroys, "%s: %d created, %d destroyed", what, L.created, L.destroys);
}

// a seeded stream of calls over a pool of pointers
static void random_run(int pool, int parts0, unsigned seed, int calls, bool mixed)
{
    char what[96];
    std::snprintf(what, sizeof what, "pool %d parts %d seed %u%s", pool, parts0, seed, mixed ? " mixed" : "");
    ledger L;
    int evictions = 0;
    {
        engine_sim e(L);
        e.parts = parts0;
        std::mt19937 rng(seed * 7919u + (unsigned)pool * 31u + (unsigned)parts0);
        auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
        static const int call_streams[3] = { S_OWN, S_A, S_B };
        for (int c = 0; c < calls; ++c) {
            const int destroys = L.destroys;
            if (!mixed)
                e.call(ptr_of(pick(pool)), 1 + pick(8), pick(4) == 0 ? 1 : 0, call_streams[pick(3)]);
            else { // a fifth of the calls bring a host batch (the pointer is then the caller's host buffer); the ensemble takes u8 frames only
                const bool on_device = pick(5) != 0;
                e.call(ptr_of(pick(pool)), 1 + pick(8), !e.ensemble && pick(4) == 0 ? 1 : 0, call_streams[pick(3)], on_device);
            }
            evictions += L.destroys > destroys;
            const int r = pick(100);
            if (r < 10)
                L.sync_stream(pick(N_STREAMS));
            else if (r < 12)
                L.sync_device();
            if (pick(150) == 0) { // a setting changes: concurrency, flip ensemble, int8 scales
                e.drop();
                if (pick(2))
                    e.parts = 3 - e.parts;
                else if (mixed)
                    e.ensemble = !e.ensemble;
            }
        }
        L.sync_device(); // hp_engine_destroy; then the cache's destructor
    }
    expect_clean(L, what);
    // n in 1 .. 8 and two entries: a pointer has 16 keys with one stream and 30 with two halves (n = 1: one key, n >= 2: two); a pool whose keys
    // all fit may never evict.  (Mixed: the staging buffer is one pointer more; under the ensemble a pointer has 8 keys with one stream, and with
    // two halves all calls share flip_in's 16; a change of concurrency or ensemble drops, so only one setting's keys live at a time.)
    const int most_keys = (pool + (mixed ? 1 : 0)) * 30;
    if (most_keys <= (int)BOUND)
        CHECK(evictions == 0, "%s: %d evictions with at most %d keys", what, evictions, most_keys);
    if (pool >= 33)
        CHECK(evictions > 0, "%s: the run never reached eviction", what);
}

// sequences that sit exactly at the bound
static void at_the_bound()
{
    { // one key per call: 64 pointers fit, twice round; the 65th empties the cache
        ledger L;
        {
            engine_sim e(L);
            for (int round = 0; round < 2; ++round)
                for (int i = 0; i < 64; ++i)
                    e.call(ptr_of(i), 4, 0, round ? S_A : S_OWN);
            CHECK(L.created == 64 && L.destroys == 0 && L.device_syncs == 0 && e.cache.size() == 64, "64 keys: %d captures, %d destroys", L.created, L.destroys);
            e.call(ptr_of(64), 4, 0, S_B);
            CHECK(L.destroys == 64 && L.device_syncs == 1 && e.cache.size() == 1, "the 65th key: %d destroys, %zu entries", L.destroys, e.cache.size());
            L.sync_device();
        }
        expect_clean(L, "64 + 1 keys");
    }
    { // two keys per call: 32 pointers fill it exactly; a one-key call is then one too many
        ledger L;
        {
            engine_sim e(L);
            e.parts = 2;
            for (int round = 0; round < 2; ++round)
                for (int i = 0; i < 32; ++i)
                    e.call(ptr_of(i), 3, 0, S_OWN);
            CHECK(L.created == 64 && L.destroys == 0 && L.device_syncs == 0, "32 x 2 keys: %d captures, %d destroys", L.created, L.destroys);
            e.call(ptr_of(0), 1, 0, S_OWN);
            CHECK(L.destroys == 64 && e.cache.size() == 1, "the 65th key: %d destroys, %zu entries", L.destroys, e.cache.size());
            L.sync_device();
        }
        expect_clean(L, "32 x 2 + 1 keys");
    }
    { // 62 + 2 fits; 63 + 2 does not, and BOTH halves are captured after the eviction
        for (int filled : { 62, 63 }) {
            ledger L;
            {
                engine_sim e(L);
                for (int i = 0; i < filled; ++i)
                    e.call(ptr_of(i), 1, 0, S_OWN);
                e.parts = 2; // (the engine drops here; the cache itself must not need that)
                e.call(ptr_of(100), 2, 0, S_A);
                if (filled == 62)
                    CHECK(L.destroys == 0 && e.cache.size() == 64, "62 + 2: %d destroys, %zu entries", L.destroys, e.cache.size());
                else
                    CHECK(L.destroys == 63 && e.cache.size() == 2 && L.created == 65, "63 + 2: %d destroys, %zu entries", L.destroys, e.cache.size());
                L.sync_device();
            }
            expect_clean(L, "62 / 63 + 2 keys");
        }
    }
    { // the defect's own pattern: the first half HITS, the second misses on a full cache
        ledger L;
        {
            engine_sim e(L);
            for (int i = 0; i < 64; ++i)
                e.call(ptr_of(i), 1, 0, S_OWN); // (1, p_i, u8, 0)
            e.parts = 2;
            e.call(ptr_of(5), 2, 0, S_A); // halves (1, p_5, u8, 0): cached, and (1, p_5, u8, 1): not
            CHECK(L.destroys == 64 && L.created == 66 && e.cache.size() == 2, "hit + miss on a full cache: %d destroys, %d captures", L.destroys, L.created);
            e.call(ptr_of(5), 1, 0, S_B); // n = 2 then n = 1 on one pointer: the first half's key
            CHECK(L.created == 66, "n = 1 after n = 2 on one pointer captured again (%d)", L.created);
            L.sync_device();
        }
        expect_clean(L, "hit + miss on a full cache");
    }
    { // the ensemble and host batches: which pointer a call is keyed by
        ledger L;
        {
            engine_sim e(L);
            e.ensemble = true; // one stream, device batches: the caller's pointer, so 64 pointers fill the cache and the 65th empties it
            for (int i = 0; i < 65; ++i)
                e.call(ptr_of(i), 2, 0, S_OWN);
            CHECK(L.created == 65 && L.destroys == 64 && e.cache.size() == 1, "ensemble, 65 pointers: %d captures, %d destroys", L.created, L.destroys);
            e.drop();
            e.parts = 2; // two halves read flip_in alone: every pointer, and a host batch, has the same two keys
            for (int i = 0; i < 70; ++i)
                e.call(ptr_of(i), 2, 0, i & 1 ? S_A : S_OWN, i % 7 != 0);
            CHECK(L.created == 67 && e.cache.size() == 2, "ensemble with two halves, 70 pointers: %d captures, %zu entries", L.created - 65, e.cache.size());
            e.drop();
            e.ensemble = false; // host batches are keyed by the staging buffer: 70 host buffers, 2 halves, one capture each
            for (int i = 0; i < 70; ++i)
                e.call(ptr_of(i), 3, 0, S_B, false);
            CHECK(L.created == 69 && e.cache.size() == 2, "70 host batches: %d captures, %zu entries", L.created - 67, e.cache.size());
            e.call(ptr_of(0), 3, 0, S_B); // the same frames as a device batch: keys of their own
            CHECK(L.created == 71 && e.cache.size() == 4, "a device batch after host batches: %zu entries", e.cache.size());
            L.sync_device();
        }
        expect_clean(L, "ensemble and host batches");
    }
    { // a capture that fails: what was made before it stays cached and is destroyed once
        ledger L;
        {
            engine_sim e(L);
            e.parts = 2;
            e.fail_make_at = 1;
            CHECK(e.call(ptr_of(0), 2, 0, S_OWN) == -7 && e.cache.size() == 1 && L.created == 1, "failed capture: %zu entries", e.cache.size());
            e.fail_make_at = -1;
            CHECK(e.call(ptr_of(0), 2, 0, S_OWN) == 0 && e.cache.size() == 2 && L.created == 2, "after a failed capture: %zu entries", e.cache.size());
            L.sync_device();
        }
        expect_clean(L, "failed capture");
    }
    { // a synchronisation that fails destroys nothing
        ledger L;
        cache_t cache(fake_destroy{ &L });
        hp::graph_key k{ 1, ptr_of(0), 0, 0 };
        int out = 0;
        for (int i = 0; i <= 64; ++i) {
            k.ptr = ptr_of(i);
            const int rc = cache.acquire(&k, 1, &out, [&](int, int* made) { return *made = L.create(k), 0; }, [] { return -2; });
            CHECK(rc == (i < 64 ? 0 : -2), "call %d: rc %d", i, rc);
        }
        CHECK(cache.size() == 64 && L.destroys == 0, "failed synchronisation: %zu entries, %d destroys", cache.size(), L.destroys);
        CHECK(cache.drop([] { return -2; }) == -2 && cache.size() == 64 && L.destroys == 0, "failed synchronisation in drop");
    }
}

// the checker is not blind: the parent's order, and hand-made faults, through the same ledger
static void checker_sees()
{
    { // concurrency 2, more pointers than the cache holds, one stream, synchronised after every call
        ledger L;
        parent_sim p(L);
        p.parts = 2;
        int first_bad_call = -1;
        for (int i = 0; i < 70 && first_bad_call < 0; ++i) {
            p.call(ptr_of(i), 4, 0, S_OWN);
            L.sync_device();
            if (L.launch_of_destroyed)
                first_bad_call = i;
        }
        CHECK(L.launch_of_destroyed >= 1, "the parent's order: no launch of a destroyed executable reported");
        // 32 pointers leave 64 entries; the next first-half makes 65 (no eviction: > 64 is tested before the insert); its second half evicts
        CHECK(first_bad_call == 32, "the parent's first launch of a destroyed executable at pointer %d, by the code's reading 32", first_bad_call);
        std::printf("parent order: launch of a destroyed executable at the call on distinct pointer %d\n", first_bad_call + 1);
    }
    { // one stream per call, alternating caller streams, nothing synchronised: the eviction waits for the wrong streams
        ledger L;
        parent_sim p(L);
        for (int i = 0; i < 70; ++i)
            p.call(ptr_of(i), 4, 0, i & 1 ? S_A : S_B);
        CHECK(L.destroy_in_flight >= 1 && L.launch_of_destroyed == 0, "the parent's eviction: %d destroyed in flight", L.destroy_in_flight);
        CHECK(p.graphs.size() <= 65, "%zu entries", p.graphs.size());
        p.destroy();
    }
    { // the parent holds 65 entries after a call
        ledger L;
        parent_sim p(L);
        for (int i = 0; i < 65; ++i)
            p.call(ptr_of(i), 4, 0, S_OWN);
        CHECK(p.graphs.size() == 65, "%zu entries", p.graphs.size());
        L.sync_device();
        p.destroy();
        CHECK(L.faults() == 0 && L.leaks() == 0, "a parent run below eviction is clean");
    }
    { // hand-made faults
        ledger L;
        const hp::graph_key k{ 1, ptr_of(0), 0, 0 };
        const int a = L.create(k), b = L.create(k), c = L.create(k);
        L.launch(a, S_A);
        L.destroy(a);
        CHECK(L.destroy_in_flight == 1, "destroy in flight not seen");
        L.destroy(a);
        CHECK(L.double_destroy == 1, "double destroy not seen");
        L.launch(b, S_B);
        L.sync_stream(S_A);
        const int seen = L.destroy_in_flight; // (the second destroy of `a`, still in flight, counted too)
        L.destroy(b);
        CHECK(L.destroy_in_flight == seen + 1, "a synchronisation of another stream cleared the launch");
        L.launch(b, S_OWN);
        CHECK(L.launch_of_destroyed == 1, "launch of a destroyed handle not seen");
        L.launch(99, S_OWN);
        CHECK(L.unknown_handle == 1, "unknown handle not seen");
        CHECK(L.leaks() == 1 && L.live_handle(k) == c, "leak not seen");
    }
}

int main()
{
    at_the_bound();
    checker_sees();
    for (int pool : { 1, 8, 33, 64, 65, 200 })
        for (int parts : { 1, 2 })
            for (unsigned seed = 0; seed < 4; ++seed)
                for (bool mixed : { false, true })
                    random_run(pool, parts, seed, 600, mixed);
    if (g_fail) {
        std::printf("FAILED %d of %d\n", g_fail, g_checks);
        return 1;
    }
    std::printf("OK %d\n", g_checks);
    return 0;
}
