// graph_cache.hpp — the engine's cache of captured-graph executables: one per (frames, input pointer, kind, first frame), at most `bound`
// of them.  Host only and templated on the executable's type, so tests/cpp/graph_cache.cpp drives the very code of hp_engine with fake handles
// and a ledger (created / in flight on stream k / destroyed).  What it guarantees, with the callers' part of each in brackets:
//
//  (a) no executable handed out for a call is destroyed before the call has issued its launches: a call asks for ALL its keys in ONE acquire(),
//      which decides about eviction once, before the first capture [the caller launches what acquire() gave it before it calls the cache again];
//      a call whose keys all hit evicts nothing and synchronises nothing: it costs its look-ups
//  (b) nothing is destroyed while a launch of it may be in flight: eviction and drop() call `sync` first and destroy only when it succeeded
//      [`sync` waits for EVERY stream of the device - the engine passes hipDeviceSynchronize - since an earlier call may have launched on a
//      caller's stream, which the caller may have destroyed since: a remembered list of streams cannot be waited on]
//  (c) every executable is destroyed exactly once: at eviction, at drop() or by the destructor [which does not synchronise: the owner has]
//  (d) size() <= bound whenever acquire() returns
//
// Eviction empties the cache: a caller that cycles more pointers than the bound pays one synchronisation and the re-captures of what it uses
// next; one that stays below it never evicts.
#pragma once
#include <cstddef>
#include <map>
#include <tuple>
#include <utility>

namespace hp {

struct graph_key {
    int n;
    const void* ptr;
    int kind;
    int b0; // first frame of the range the graph covers (hp_engine_set_concurrency(2): one graph per half-batch, launched on its own stream)
    bool operator<(const graph_key& o) const { return std::tie(n, ptr, kind, b0) < std::tie(o.n, o.ptr, o.kind, o.b0); }
};

template <typename Exec, typename Destroy>
class graph_cache {
public:
    static constexpr size_t bound = 64;
    static constexpr int max_keys = 2; // per call: the whole batch, or its two halves

    explicit graph_cache(Destroy d = Destroy())
        : destroy_(d)
    {
    }
    graph_cache(const graph_cache&) = delete;
    graph_cache& operator=(const graph_cache&) = delete;
    ~graph_cache() { destroy_all(); }

    size_t size() const { return map_.size(); }

    // The executables of one call's keys[0 .. nk), nk <= max_keys, into out[]: found, or made by `make(i, &exec)` (capture + instantiate; 0 = ok)
    // and kept.  When the missing ones do not fit, `sync()` (0 = ok) and then every cached executable is destroyed - before anything is handed
    // out or made.  Returns 0, or what sync / make returned; after a failed make the executables made before it stay cached.
    template <typename Make, typename Sync>
    int acquire(const graph_key* keys, int nk, Exec* out, Make&& make, Sync&& sync)
    {
        if (nk < 1 || nk > max_keys)
            return -1;
        bool have[max_keys] = {};
        int missing = 0;
        for (int i = 0; i < nk; ++i) {
            const auto it = map_.find(keys[i]);
            if (it != map_.end())
                out[i] = it->second, have[i] = true;
            else
                ++missing;
        }
        if (missing == 0)
            return 0; // the steady state
        if (map_.size() + missing > bound) {
            if (const int rc = sync())
                return rc;
            destroy_all();
            for (int i = 0; i < nk; ++i)
                have[i] = false;
        }
        for (int i = 0; i < nk; ++i) {
            if (have[i])
                continue;
            const auto it = map_.find(keys[i]); // (the same key twice in one call)
            if (it != map_.end()) {
                out[i] = it->second;
                continue;
            }
            Exec made{};
            if (const int rc = make(i, &made))
                return rc;
            map_.emplace(keys[i], made);
            out[i] = made;
        }
        return 0;
    }

    // forget everything (a setting changed: the captured schedules are of the old form); `sync` is called whether or not anything is cached
    template <typename Sync>
    int drop(Sync&& sync)
    {
        if (const int rc = sync())
            return rc;
        destroy_all();
        return 0;
    }

private:
    void destroy_all()
    {
        for (auto& g : map_)
            destroy_(g.second);
        map_.clear();
    }

    std::map<graph_key, Exec> map_;
    Destroy destroy_;
};

} // namespace hp
