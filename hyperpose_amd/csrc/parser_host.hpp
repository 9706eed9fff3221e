// parser_host.hpp — the host side that the three parsers (paf_parser.hip, ppn_parser.hip, pifpaf_parser.hip) share on the road from an
// engine's output maps to the hp_human lists a caller receives.  Kernels, shapes, list sizes and host tails stay with each parser.
// Host-only; DESIGN.md section 7E.3.
#pragma once
#include "hp_common.hpp"

#include <algorithm>
#include <memory>

namespace hp {

// One batch at a time: launch on a stream, record `done` there, pending = n; later wait for `done`, pending = 0.  The session owns the
// stream and the event.  A parser handle derives from it and its destructor's body is drain(), so that its buffers outlive the work that
// uses them; the order is then the same for all three: wait for `done` if a batch is pending (it may have been enqueued on a caller's
// stream), wait for the own stream, destroy the event, destroy the stream.
struct parser_session {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    int max_batch = 0;
    int pending = 0; // frames of the enqueued, not yet collected batch

    virtual ~parser_session()
    {
        drain();
        if (done)
            (void)hipEventDestroy(done);
        if (stream)
            (void)hipStreamDestroy(stream);
    }
    // what a pipeline asks of its parser (pipeline.cpp): the number of outputs its network has, parse the n frames that lie in the engine's
    // output buffers in stream order on `s`, and later the humans of that batch.  Which output is which argument is the parser's knowledge.
    virtual int engine_outputs() const = 0;
    virtual int enqueue_outputs(hp_engine* e, int n, hipStream_t s) = 0;
    virtual int collect(hp_human* out, int cap_per_frame, int* n_out) = 0;

    int open(int max_batch_) // (a failure half-way leaves what was made to the destructor)
    {
        max_batch = max_batch_;
        HP_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HP_HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        return HP_OK;
    }
    void drain()
    {
        if (pending && done)
            (void)hipEventSynchronize(done);
        pending = 0;
        if (stream)
            (void)hipStreamSynchronize(stream);
    }
    hipStream_t stream_or_own(void* s) const { return s ? (hipStream_t)s : stream; }
    // the entry checks of every call that launches a batch (null arguments are the caller's)
    int begin(const char* who, int n) const
    {
        HP_REQUIRE(n >= 1 && n <= max_batch, HP_ERR_CAPACITY, "%s: batch %d > max_batch %d", who, n, max_batch);
        HP_REQUIRE(pending == 0, HP_ERR_STATE, "%s: a batch is already in flight, collect it first", who);
        return HP_OK;
    }
    int launched(int n, hipStream_t s)
    {
        HP_HIP_TRY(hipEventRecord(done, s));
        pending = n;
        return HP_OK;
    }
    int wait(const char* who, int* n)
    {
        HP_REQUIRE(pending > 0, HP_ERR_STATE, "%s: nothing was enqueued", who);
        *n = pending;
        pending = 0;
        HP_HIP_TRY(hipEventSynchronize(done));
        return HP_OK;
    }
};
// a handle of the C ABI as its session (each parser unit defines its own)
parser_session* session_of(hp_paf* p);
parser_session* session_of(hp_ppn* p);
parser_session* session_of(hp_pifpaf* p);

// Host inputs of a process_batch call: allocated once for max_batch frames of `per_frame` bytes, n frames copied on `s`.
struct staged_input {
    dev_buf buf;
    int stage(const float* host, size_t per_frame, int n, int max_batch, hipStream_t s, const float** dev)
    {
        if (buf.bytes < per_frame * max_batch)
            HP_TRY(buf.alloc(per_frame * max_batch));
        HP_HIP_TRY(hipMemcpyAsync(buf.p, host, per_frame * n, hipMemcpyHostToDevice, s));
        *dev = buf.as<float>();
        return HP_OK;
    }
};

// What a collect hands back: frame f's humans at out + f * cap (out may be null), its true count in n_out[f], and per frame either
// nothing (complete) or the message of its capacity failure - the other frames of such a batch are complete.  Frames may be delivered
// from the pool's threads, each frame by one of them.
struct frame_results {
    const char* who; // "paf" | "ppn" | "pifpaf", as the messages name the parser
    hp_human* out;
    int cap;
    int* n_out;
    std::vector<std::string> failed;

    // `count` humans were found, the first `have` of them lie at src
    void deliver(int f, const hp_human* src, int count, int have)
    {
        n_out[f] = count;
        have = std::min(have, cap);
        if (out && have > 0)
            memcpy(out + (size_t)f * cap, src, sizeof(hp_human) * have);
        if (count > have)
            fail(f, "%s: frame %d has %d humans, capacity %d", who, f, count, have);
    }
    void fail(int f, const char* fmt, ...) __attribute__((format(printf, 3, 4)))
    {
        char msg[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        failed[f] = msg;
    }
    // HP_OK, or HP_ERR_CAPACITY with hp_last_error() = the message of the last failing frame
    int code() const
    {
        for (size_t f = failed.size(); f-- > 0;)
            if (!failed[f].empty()) {
                set_error("%s", failed[f].c_str());
                return HP_ERR_CAPACITY;
            }
        return HP_OK;
    }
};

// fn(k, worker) for k in [0, frames), over the parsers' host worker pool (hp_common.hpp); returns when all are done
template <typename F>
void on_host_pool(int frames, F&& fn)
{
    frame_pool::instance().run(frames, [](int k, int worker, void* c) { (*static_cast<std::remove_reference_t<F>*>(c))(k, worker); }, &fn);
}

// A collected batch whose lists overflowed is parsed again with larger ones, at most `limit` times.  grow(&grown): look at what the last
// launch reported and enlarge what can grow (the rule is the parser's); relaunch(): the parser's launch from the inputs it kept, on the
// stream it chooses, ending in launched().
template <typename Grow, typename Relaunch>
int reparse(parser_session& s, const char* who, int limit, Grow&& grow, Relaunch&& relaunch)
{
    for (int round = 0, n = 0; round < limit; ++round) {
        bool grown = false;
        HP_TRY(grow(&grown));
        if (!grown)
            break;
        HP_TRY(relaunch());
        HP_TRY(s.wait(who, &n));
    }
    return HP_OK;
}

} // namespace hp
