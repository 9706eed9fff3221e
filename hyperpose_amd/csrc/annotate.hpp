// annotate.hpp — what the units that write into device-resident frames (overlay.hip, redact.hip, mapview.hip; a further annotator is a kernel and
// its rules on top of this) share on the host: the ring that takes a call's list or tables to the device, and the argument checks of a frame.
#pragma once
#include "hp_common.hpp"
#include "part_points.hpp"

namespace hp {

// The staged list ring: SLOTS pinned staging buffers and as many device lists, used in turn, so that a call neither allocates nor waits for
// the device unless the slot's use SLOTS calls ago has not finished.  One call, in order: take() the slot's pinned buffer (waits, on the
// host, for that earlier use) and fill it; upload() n bytes of it to device() on the caller's stream; launch; commit() records the slot's
// event and advances.  A call that returns before commit() leaves the ring where it was.  One ring = one thread at a time.
struct staged_ring {
    static constexpr int SLOTS = 4;
    host_buf stage[SLOTS];
    dev_buf list[SLOTS];
    hipEvent_t done[SLOTS] = {};
    bool used[SLOTS] = {};
    int next = 0;

    // `bytes` per slot; on failure the error is set and the destructor frees what was allocated
    int alloc(size_t bytes, const char* who)
    {
        for (int k = 0; k < SLOTS; ++k) {
            HP_TRY(stage[k].alloc(bytes));
            HP_TRY(list[k].alloc(bytes));
            HP_REQUIRE(hipEventCreateWithFlags(&done[k], hipEventDisableTiming) == hipSuccess, HP_ERR_HIP, "%s: hipEventCreateWithFlags failed", who);
        }
        return HP_OK;
    }
    template <typename T> int take(T*& pinned)
    {
        if (used[next])
            HP_HIP_TRY(hipEventSynchronize(done[next])); // the use SLOTS calls ago
        pinned = stage[next].as<T>();
        return HP_OK;
    }
    int upload(size_t n, hipStream_t s) { HP_HIP_TRY(hipMemcpyAsync(list[next].p, stage[next].p, n, hipMemcpyHostToDevice, s)); return HP_OK; }
    template <typename T> const T* device() const { return list[next].as<T>(); }
    int commit(hipStream_t s)
    {
        HP_HIP_TRY(hipGetLastError()); // the launch
        HP_HIP_TRY(hipEventRecord(done[next], s));
        used[next] = true;
        next = (next + 1) % SLOTS;
        return HP_OK;
    }
    // drain, then free: what a late call returns (the runtime may be gone) is ignored
    ~staged_ring()
    {
        for (int k = 0; k < SLOTS; ++k)
            if (used[k])
                (void)hipEventSynchronize(done[k]);
        for (auto& e : done)
            if (e)
                (void)hipEventDestroy(e);
    }
};

// ---- argument checks; `who` is the entry point, `name` the layout ("BGR" or hp_yuv::layout::name) ----------------------------------------

inline int check_bgr_frame(const char* who, const uint8_t* bgr, int w, int h, int stride)
{
    HP_REQUIRE(bgr, HP_ERR_INVALID, "%s: BGR: null frame", who);
    HP_REQUIRE(w > 0 && h > 0, HP_ERR_INVALID, "%s: BGR: empty frame (%d x %d)", who, w, h);
    HP_REQUIRE(stride > 0 && (int64_t)stride >= (int64_t)w * 3, HP_ERR_INVALID, "%s: BGR: stride %d is smaller than a row (%lld bytes)", who, stride, (long long)w * 3);
    return HP_OK;
}

inline int check_max_dim(const char* who, const char* name, int w, int h)
{
    HP_REQUIRE(w <= hp_pts::MAX_DIM && h <= hp_pts::MAX_DIM, HP_ERR_INVALID, "%s: %s: a frame of %d x %d is beyond the %d x %d the coverage arithmetic is stated for", who,
        name, w, h, hp_pts::MAX_DIM, hp_pts::MAX_DIM);
    return HP_OK;
}

} // namespace hp
