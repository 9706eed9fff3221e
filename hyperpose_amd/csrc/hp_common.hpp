// hp_common.hpp — shared host-side plumbing of libhp_hip.so: error reporting across the C ABI,
// HIP call checking, RAII device/pinned buffers.  No reference counterpart (the reference's error
// policy is print + std::exit, src/logging.hpp:31-37; the C ABI returns codes instead and the C++
// mirror classes in include/hyperpose/ restore the throw/exit behaviour on top).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hp_hip.h"

namespace hp {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* last_error();

#define HP_HIP_TRY(expr)                                                                                     \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess) {                                                                              \
            ::hp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);      \
            return HP_ERR_HIP;                                                                               \
        }                                                                                                    \
    } while (0)

#define HP_REQUIRE(cond, code, ...)                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            ::hp::set_error(__VA_ARGS__);                                                                    \
            return (code);                                                                                   \
        }                                                                                                    \
    } while (0)

#define HP_TRY(expr)                                                                                         \
    do {                                                                                                     \
        int _rc = (expr);                                                                                    \
        if (_rc != HP_OK)                                                                                    \
            return _rc;                                                                                      \
    } while (0)

// Owning device buffer (hipMalloc / hipFree).
struct dev_buf {
    void* p = nullptr;
    size_t bytes = 0;
    dev_buf() = default;
    dev_buf(const dev_buf&) = delete;
    dev_buf& operator=(const dev_buf&) = delete;
    ~dev_buf() { release(); }
    int alloc(size_t n)
    {
        release();
        if (n == 0)
            return HP_OK;
        HP_HIP_TRY(hipMalloc(&p, n));
        bytes = n;
        return HP_OK;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

// Owning pinned host buffer.
struct host_buf {
    void* p = nullptr;
    size_t bytes = 0;
    host_buf() = default;
    host_buf(const host_buf&) = delete;
    host_buf& operator=(const host_buf&) = delete;
    ~host_buf() { release(); }
    int alloc(size_t n)
    {
        release();
        if (n == 0)
            return HP_OK;
        HP_HIP_TRY(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
        return HP_OK;
    }
    void release()
    {
        if (p)
            (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// tiles.cpp: hp_humans_merge without its capacity rule - the kept humans in kept order (hp_pipeline_collect in tiled mode)
int merge_humans(const hp_human* in, const int32_t* region_of, int n, int frame_w, int frame_h, int min_common, double tol, std::vector<hp_human>& kept);

// The engine's environment switches ("Engine switches"), read once by read_engine_switches() when hp_engine_create or
// hp_engine_load makes an engine: its schedule, its launches and the graphs it captures follow the environment of that moment.  Host-only:
// the launchers and pickers that consult one get it as an argument.  Unset = the default below.
struct engine_switches {
    bool no_fuse = false;        // HP_NO_FUSE: no fused launches (separable blocks, heads, chains, bottlenecks, pairs)
    bool no_fuse_head = false;   // HP_NO_FUSE_HEAD: fp16 heads as two launches (mlp_head_variant)
    bool no_splitk = false;      // HP_NO_SPLITK: fp16 convolutions without split-K
    bool no_chain = false;       // HP_NO_CHAIN: no conv_chain launches
    bool no_bneck = false;       // HP_NO_BNECK: no bottleneck launches
    bool no_seppair = false;     // HP_NO_SEPPAIR: no two-block separable launches
    bool no_pair_heads = false;  // HP_NO_PAIR_HEADS: fp16 sibling heads as two launches
    bool fuse32 = false;         // HP_FUSE32: depthwise + pointwise fusion on HP_DTYPE_F32 engines too (always on for F32S)
    bool no_fuse32 = false;      // HP_NO_FUSE32: no depthwise + pointwise fusion on fp32 engines
    bool no_head32 = false;      // HP_NO_HEAD32: fp32 1 x 1 head pairs as two launches
    bool no_arena = false;       // HP_NO_ARENA: every fp32 activation tensor in its own allocation
    bool no_winograd32 = false;  // HP_NO_WINOGRAD32: no fp32 Winograd layers
    bool wino_tall = true;       // HP_WINO_TALL=0: the per-image Winograd form instead of the tall one
    int wino_nc = 0;             // HP_WINO_NC=1 | 2: force the Winograd column tiles per block (0: by the engine's mode)
    bool head_pair32 = true;     // HP_HEAD_PAIR=0: fp32 sibling heads as two launches instead of one grid
    int c32_wk = -1;             // HP_C32_WK: 0 = no conv32_wk_kernel, 1 = every layer of its shape, -1 = by size
    int c32_bn160 = -1;          // HP_C32_BN160: 0 = no 64 x 160 tiles, 1 = every layer on them, -1 = by size
    int dw32_px = 0;             // HP_DW32_PX: 1 = one depthwise column per thread, 2 = column pairs always, 0 = by size
    int lane_epilogue = 0;       // HP_LANE_EPILOGUE: conv32_params::lane_epilogue
    bool first_conv_verify = false; // HP_FIRST_CONV_VERIFY: first_conv32_kernel compares its LDS with global memory (first_conv32_verify_counts)
    // block timelines printed per launch (s_memtime stamps; tools/*_timeline.py)
    bool dbg_conv = false, dbg_bn = false, dbg_chain = false, dbg_sep = false; // HP_CONV_DBG, HP_BN_DBG, HP_CHAIN_DBG, HP_SEP_DBG
    bool dbg_direct = false;     // HP_DIRECT_DBG: the fp32 direct, Winograd and conv32 kernels
    int dbg_min_cin = 256;       // HP_DIRECT_DBG_MINCIN: conv32 layers with fewer input channels print nothing
};
engine_switches read_engine_switches();

// Host worker pool for the order-dependent parser tails (PoseProposal limb selection / merge, PifPaf grow / soft-NMS): frames are
// independent, so hp_*_collect hands frame indices to a few persistent threads, the way the reference replicates its parser per
// pool thread (include/hyperpose/utility/thread_pool.hpp:21, include/hyperpose/stream/stream.hpp:139-144).  The calling thread
// takes part; run() returns when every frame is done.  `fn(frame, worker)`: worker in [0, workers()) selects per-thread scratch.
// HP_PARSER_THREADS overrides the default min(8, hardware threads).
class frame_pool {
public:
    static frame_pool& instance();
    int workers() const { return n_threads_ + 1; }
    void run(int n_frames, void (*fn)(int frame, int worker, void* ctx), void* ctx);
    ~frame_pool();

private:
    frame_pool();
    struct impl;
    impl* d_;
    int n_threads_;
};

} // namespace hp
