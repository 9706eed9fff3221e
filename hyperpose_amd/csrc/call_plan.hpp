// call_plan.hpp — what one hp_engine_infer_u8 / hp_engine_infer_f32 call does, decided ONCE and as data: a refusal, or the buffer the network
// reads, the frames that still go up, one range or two half-batches, where the flip ensemble's stage and merge lie, the captured graphs' keys.
// Pure host code (no HIP header, no allocation), so tests/cpp/call_plan.cpp enumerates it and tests/cpp/graph_cache.cpp takes its keys from it;
// hp_engine::run_call (engine.cpp) only carries a plan out.  The rules, each stated here and nowhere else:
//   ensemble setup  a host batch goes up into flip_in first, on the call's stream; a device batch is copied there by flip_stage (fl_src); from
//                   then on the call is a device batch of 2n frames - the caller's frames, their left-right flips behind them
//   half-batches    two ranges when parts == 2 && halves_ok && images >= 2, images counted after the doubling; the first has (images + 1) / 2
//   host uploads    every range's frames go up on that range's OWN stream, after the fork and before the range runs (one range: the call's
//                   stream) and never inside a captured graph.  An event recorded behind ONE hipMemcpyAsync from pageable memory does not cover
//                   all of that copy's staged chunks - measured: stream2's first layer now and then read a few stale input rows of frames 4 / 5
//                   of 8, tools/r6_halves_debug.py - while a kernel behind the copy on the same stream always saw it complete.
//   stage and merge inside the range's body with one range (a captured graph then holds them, and the copy from the caller's buffer), around the
//                   fork and the join with two (the frames are the first half-batch, their flips the second)
//   key pointer     fl_src when the ensemble is on, the batch is on the device and there is one range (that graph holds the copy from the
//                   caller's buffer); otherwise the address the network reads
//   key kind        2 under the ensemble, otherwise 0 (u8) or 1 (f32)
#pragma once
#include "graph_cache.hpp"

namespace hp {

struct call_settings { int max_batch, parts; bool halves_ok, ensemble, use_graph; }; // the engine's settings that bear on a call
struct call_buffers { const void *in_stage, *flip_in; };
struct call_args { // hp_engine_infer_*'s arguments; kind 0: u8 HWC frames, 1: f32 NCHW
    const void* input = nullptr;
    int n = 0, on_device = 0, kind = 0;
    void* stream = nullptr; // the caller's, or null for the engine's own (the plan does not read it)
};

enum call_refusal { CALL_OK, CALL_EMPTY, CALL_OVERFLOW, CALL_F32_ENSEMBLE, CALL_ENSEMBLE_OVERFLOW }; // in the order they are tested
struct call_range { int b0, cnt; bool second; }; // frames [b0, b0 + cnt) of the network's batch, on the engine's second stream or the call's

struct call_plan {
    call_refusal refusal; // != CALL_OK: nothing else is set
    int kind, images;     // images: what the network runs, 2n under the ensemble
    const void* read;     // the device address the network reads: the caller's pointer, in_stage or flip_in
    const void* host_src; // frames that still have to go up to `read`, or null: under the ensemble first of all, else range by range
    const void* fl_src;   // ensemble on a device batch: what flip_stage copies into flip_in first, else null
    bool ensemble, stage_inside, captured; // stage_inside: flip and merge lie inside the one range's body, not around the fork and the join
    int nr;                                // ranges[0 .. nr) and their keys
    call_range ranges[2];
    graph_key keys[2];
};

inline call_refusal refusal_of(const call_settings& e, const call_args& a)
{
    return a.n < 1 ? CALL_EMPTY : a.n > e.max_batch ? CALL_OVERFLOW : !e.ensemble ? CALL_OK : a.kind != 0 ? CALL_F32_ENSEMBLE
        : 2 * a.n > e.max_batch ? CALL_ENSEMBLE_OVERFLOW : CALL_OK;
}

inline bool reads_in_stage(const call_settings& e, const call_args& a) { return !a.on_device && !e.ensemble; } // (the engine grows it, then plans)

inline call_plan plan_call(const call_settings& e, const call_buffers& b, const call_args& a)
{
    call_plan p{};
    if ((p.refusal = refusal_of(e, a)) != CALL_OK)
        return p;
    p.kind = a.kind, p.ensemble = e.ensemble, p.captured = e.use_graph, p.images = e.ensemble ? 2 * a.n : a.n;
    p.read = e.ensemble ? b.flip_in : reads_in_stage(e, a) ? b.in_stage : a.input;
    p.host_src = a.on_device ? nullptr : a.input, p.fl_src = e.ensemble && a.on_device ? a.input : nullptr;
    const bool halves = e.parts == 2 && e.halves_ok && p.images >= 2;
    const int n0 = halves ? (p.images + 1) / 2 : p.images;
    p.nr = halves ? 2 : 1, p.ranges[0] = { 0, n0, false }, p.ranges[1] = { n0, p.images - n0, true }; // (one range: the second is empty)
    p.stage_inside = e.ensemble && !halves;
    for (int i = 0; i < p.nr; ++i)
        p.keys[i] = graph_key{ p.ranges[i].cnt, p.fl_src && p.nr == 1 ? p.fl_src : p.read, e.ensemble ? 2 : a.kind, p.ranges[i].b0 };
    return p;
}

} // namespace hp
