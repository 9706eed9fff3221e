// call_plan.hpp — what one hp_engine_infer_u8 / hp_engine_infer_f32 call does, decided ONCE and as data: a refusal, or the buffer the network
// reads, the frames that still go up, one range or two half-batches, where the flip ensemble's stage and merge lie, the captured graphs' keys.
// Pure host code (no HIP header, no allocation), so tests/cpp/call_plan.cpp enumerates it and tests/cpp/graph_cache.cpp takes its keys from it;
// hp_engine::run_call (engine.cpp) only carries a plan out.  The rules, each stated here and nowhere else:
//   ensemble setup  a host batch goes up into flip_in first, on the call's stream; a device batch is copied there by ensemble_stage (fl_src); from
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
//   key kind        2 under the ensemble, otherwise 0 (u8) or 1 (f32); under the scale ensemble of K maps per frame 1 + K (3 .. 5), or
//                   4 + K (6 .. 8) with the flip ensemble as well: a graph captured under one setting is never replayed under another
//   scale ensemble  (scales = K > 1; csrc/scale_ensemble.hpp) a u8 batch of n frames runs as (ensemble ? 2 : 1) * K * n images of flip_in:
//                   the frames, their K - 1 shrunken copies behind them (scale-major), and with the flip ensemble the flips of all K n slots
//                   behind those.  It is staged and merged exactly where the flip ensemble is - the scale stage first, then the flip; the
//                   flip merge over the K n slots first, then the scale merge over the n frames - and refuses what the flip ensemble refuses.
//                   With scales == 1 every plan is the plan of a call_settings that leaves the field at its default.
#pragma once
#include "graph_cache.hpp"

namespace hp {

struct call_settings { // the engine's settings that bear on a call
    int max_batch, parts;
    bool halves_ok, ensemble, use_graph;
    int scales = 1; // K of the scale ensemble, 1 while it is off
};
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
    int kind, images;     // images: what the network runs, 2n under the ensemble (images_of)
    const void* read;     // the device address the network reads: the caller's pointer, in_stage or flip_in
    const void* host_src; // frames that still have to go up to `read`, or null: under the ensemble first of all, else range by range
    const void* fl_src;   // ensemble on a device batch: what ensemble_stage copies into flip_in first, else null
    bool ensemble, stage_inside, captured; // stage_inside: flip and merge lie inside the one range's body, not around the fork and the join
    int nr;                                // ranges[0 .. nr) and their keys
    call_range ranges[2];
    graph_key keys[2];
    int scales;  // K of the scale ensemble (1: off)
    bool staged; // either ensemble: the network reads flip_in, staged and merged as the flip ensemble alone is
};

// the images one call of n frames runs; under either ensemble, images of flip_in
inline int images_of(const call_settings& e, int n) { return (e.ensemble ? 2 : 1) * e.scales * n; }
inline bool staged(const call_settings& e) { return e.ensemble || e.scales > 1; }

inline call_refusal refusal_of(const call_settings& e, const call_args& a)
{
    return a.n < 1 ? CALL_EMPTY : a.n > e.max_batch ? CALL_OVERFLOW : !staged(e) ? CALL_OK : a.kind != 0 ? CALL_F32_ENSEMBLE
        : images_of(e, a.n) > e.max_batch ? CALL_ENSEMBLE_OVERFLOW : CALL_OK;
}

inline bool reads_in_stage(const call_settings& e, const call_args& a) { return !a.on_device && !staged(e); } // (the engine grows it, then plans)

inline call_plan plan_call(const call_settings& e, const call_buffers& b, const call_args& a)
{
    call_plan p{};
    if ((p.refusal = refusal_of(e, a)) != CALL_OK)
        return p;
    p.kind = a.kind, p.ensemble = e.ensemble, p.captured = e.use_graph, p.images = images_of(e, a.n);
    p.scales = e.scales, p.staged = staged(e);
    p.read = p.staged ? b.flip_in : reads_in_stage(e, a) ? b.in_stage : a.input;
    p.host_src = a.on_device ? nullptr : a.input, p.fl_src = p.staged && a.on_device ? a.input : nullptr;
    const bool halves = e.parts == 2 && e.halves_ok && p.images >= 2;
    const int n0 = halves ? (p.images + 1) / 2 : p.images;
    p.nr = halves ? 2 : 1, p.ranges[0] = { 0, n0, false }, p.ranges[1] = { n0, p.images - n0, true }; // (one range: the second is empty)
    p.stage_inside = p.staged && !halves;
    const int key_kind = e.scales > 1 ? (e.ensemble ? 4 : 1) + e.scales : e.ensemble ? 2 : a.kind;
    for (int i = 0; i < p.nr; ++i)
        p.keys[i] = graph_key{ p.ranges[i].cnt, p.fl_src && p.nr == 1 ? p.fl_src : p.read, key_kind, p.ranges[i].b0 };
    return p;
}

} // namespace hp
