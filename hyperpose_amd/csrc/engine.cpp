// engine.cpp — hyperpose::dnn engine on gfx950 (replaces reference src/tensorrt.cpp).
//
// The reference hands an exported graph to TensorRT (create_{uff,onnx,serialized}_engine, src/tensorrt.cpp:121-252),
// allocates one device buffer per binding for max_batch (:255-316) and, per call, does H2D of an f32 NCHW
// batch, executeV2, and one D2H per (output x image) (:364-434).  Here the graph is a static layer list
// (include/hp_hip.h: hp_layer) executed as a fixed schedule of hand-written HIP kernels (conv_kernels.hip)
// on one stream, optionally replayed from a captured hipGraph:
//   * input stays u8 HWC in HBM; the u8->f32 / BGR->RGB / mean-std step of src/data.cpp:21-51 is folded into the
//     first convolution's load;
//   * activations are NHWC fp16 with fp32 MFMA accumulation, concat is a channel offset into a shared buffer;
//   * heads write fp32 NCHW straight from the conv epilogue into the buffers the parser kernels read —
//     feature maps never cross PCIe.
#include "conv32_pick.hpp"
#include "conv_i8.hpp"
#include "conv_kernels.hpp"
#include "engine_timeline.hpp"
#include "call_plan.hpp"
#include "hp_common.hpp"
#include "scale_ensemble.hpp"
#include "weight_pack.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <variant>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

struct tensor_info {
    bool defined = false;
    bool elided = false;     // produced and consumed inside one fused launch: never materialised in HBM
    bool unwritten = false;  // a network output nobody else reads: only its fp32 NCHW form is produced
    int H = 0, W = 0, C = 0; // C = total channels written
    int cs = 0;              // channel stride of the buffer
    int P = 0;               // zero halo (pixels) around every image: the largest padding any consumer needs
    hp::dev_buf buf;         // the tensor's own allocation, or
    void* shared = nullptr;  // ... a buffer of the engine's activation arena that tensors of the same geometry take turns in (hp_engine::arena)
    int arena_slot = -1;
    template <typename T>
    T* base() const { return static_cast<T*>(shared ? shared : buf.p); }
    hp::tview view(int coff) const
    {
        hp::tview v;
        const int wp = W + 2 * P;
        v.p = base<__half>() + ((size_t)P * wp + P) * cs;
        v.cs = cs, v.coff = coff, v.wp = wp, v.img = (H + 2 * P) * wp;
        return v;
    }
    // rows one image takes in an fp32 buffer: H + 2 P, made EVEN when there is a halo - the images of a batch then form one tall image whose
    // separator rows are zeros and whose 2 x 2 Winograd tiles fall on the same rows in every image (conv32_winograd.hip, "tall" form)
    int rows32() const { return P > 0 ? (H + 2 * P + 1) / 2 * 2 : H; }
    hp::tview32 view32(int coff) const // the same geometry with 4-byte elements (HP_DTYPE_F32 engines)
    {
        hp::tview32 v;
        const int wp = W + 2 * P;
        v.p = base<float>() + ((size_t)P * wp + P) * cs;
        v.cs = cs, v.coff = coff, v.wp = wp, v.img = rows32() * wp;
        return v;
    }
};

struct out_info {
    std::string name;
    int tensor, coff, channels, act;
    int H, W;       // source tensor size
    hp::out_xform x{}; // conversion parameters; x.out_h / x.out_w / (C / shuffle^2) is the reported shape
    int out_c() const { return x.C / (x.shuffle * x.shuffle); }
    bool plain() const { return x.shuffle == 1 && x.group == 0 && x.out_h == H && x.out_w == W && x.scale == 1.f && x.grid == 0; }
    int fused_layer = -1; // layer whose epilogue writes it, or -1 -> conversion kernel
    std::unique_ptr<hp::dev_buf> buf;
};

// What the engine can launch: one value per kernel family and form.  Set by the lowering or fusion pass that decides it (lower_layers, fuse_*,
// pair_heads) and never changed afterwards.  Two decisions are left to every launch, because they depend on what it is bound to:
// an int8-capable dense conv runs conv_i8 only while its scale is positive (hp_engine::bound), and two adjacent fp32 heads share a grid when
// pick32::head_pair_ok (conv32_pick.hpp) says so for the batch (hp_engine::launch_head_pair32).
enum class launch_kind : char {
    // fp16 (and int8) engines
    first16,
    conv16,
    dw16,
    maxpool16,
    upsample16,
    sep,       // depthwise layer `layer` fused with the pointwise layer `layer + 1`
    sep_pair,  // ... and the NEXT separable block (layers `layer + 2`, `layer + 3`) in the same launch
    head,      // 1x1 conv `layer` (-> 512, relu) fused with the 1x1 conv `layer + 1`
    head_pair, // ... and the sibling head on the same input (layers `layer + 2`, `layer + 3`)
    chain,     // [1x1 ->] 3x3 -> 3x3 on 128 channels in one launch (conv_chain.hip), layers `layer` ..
    bneck,     // [3x3 ->] expansion 1x1 + shortcut [-> the next block's reduction 1x1] (conv_bottleneck.hip)
    // HP_DTYPE_F32 / F32S engines (conv_fp32.hip): one launch per layer or fused pair
    first32,
    conv32,
    wino2,  // a 3 x 3 stride-1 layer on conv32_winograd_kernel (cp.w_wino)
    direct, // conv32_direct_kernel, which reads `cin_split` input channels (whole chunks)
    head32, // 1 x 1 128 -> HID -> 1 x 1 HID -> C2 in one launch (conv32_head.hip): cp = the second layer's epilogue, hh = the first layer
    dw32,
    maxpool32,
    upsample32,
};
// the payloads that are more than one parameter struct of conv_kernels.hpp / conv_fp32.hpp
struct conv16_launch {
    hp::conv_params cp;
    // HP_DTYPE_I8 engines: a layer conv_i8_kernel covers keeps its fp16 launch (cp) and gets the int8 one beside it; which of the two runs
    // is the layer's entry of hp_engine::i8_scale (> 0: int8 with that activation scale, 0: fp16)
    hp::conv_i8_params q8; // q8.c is cp as bound at every launch; q8.dq points at i8_dq
    float* i8_dq;          // device [cp.Cout_pad]: s_a * s_w[c], rewritten by hp_engine::apply_int8_scales
    bool i8;               // in the schedule: the layer has an int8 launch; in a bound copy: this launch is the int8 one
};
struct sep_pair_launch {
    hp::sep_params a, b;
};
struct head_pair_launch {
    hp::head_params a, b;
};
struct conv32_launch { // conv32, wino2, direct
    hp::conv32_params cp;
    int cin_split; // direct: what the launch sets cp.Cin to
};
struct head32_launch {
    hp::conv32_params cp;
    hp::head32_hidden hh;
};
using launch_payload = std::variant<std::monostate, hp::first_conv_params, conv16_launch, hp::dw_params, hp::pool_params, hp::sep_params, sep_pair_launch,
    hp::head_params, head_pair_launch, hp::chain_params, hp::bneck_params, hp::first_conv32_params, conv32_launch, head32_launch, hp::dw32_params,
    hp::pool32_params>;

// One launch of the schedule.  `p` holds the parameters of `kind` as build() described them for max_batch frames; a launch binds a copy of them
// to its frames (bind), the schedule itself is const while the engine runs.
struct step {
    int layer;
    int op;           // the layer's op, or one of the schedule-only codes below
    launch_kind kind;
    launch_payload p;
    int n_layers = 1; // consecutive layers this step covers
    double flops = 0, bytes = 0; // per frame
    template <typename T>
    T& set(launch_kind k) // (zeroed parameters of a new kind)
    {
        kind = k;
        return p.emplace<T>();
    }
    // typed access: the wrong kind throws std::bad_variant_access (hp_engine_create turns it into an error), it never reads zeros
    template <typename T>
    T& as() { return std::get<T>(p); }
    template <typename T>
    const T& as() const { return std::get<T>(p); }
    hp::conv_params& cp() { return as<conv16_launch>().cp; } // the dense fp16 conv the schedule rewrites look at
    const hp::conv_params& cp() const { return as<conv16_launch>().cp; }
    hp::conv32_params& cp32() { return as<conv32_launch>().cp; }
    const conv16_launch* int8() const // the layer's int8 launch, if it has one
    {
        const auto* c = std::get_if<conv16_launch>(&p);
        return c && c->i8 ? c : nullptr;
    }
    conv16_launch* int8() { return const_cast<conv16_launch*>(static_cast<const step*>(this)->int8()); }
};
struct geo { // a layer's output size and the padding in front of its first row / column
    int OH, OW, pt, pl;
};
// what a layer's launch shares with the next layer's (hp_engine::fuse_next)
enum class fuse_kind : char {
    none,
    sep,    // fp16: depthwise 3x3 + the 1x1 behind it in one sepconv launch
    sep32,  // fp32: depthwise 3x3 fused into conv32_direct_kernel's load of the 1x1 behind it
    head,   // fp16: 1x1 K1 -> 512 + 1x1 512 -> <= 64 in one mlp_head launch
    head32, // fp32: 1x1 128 -> HID + 1x1 HID -> <= 64 in one conv32_head launch
};
constexpr int OP_SEPCONV = 100; // schedule-only op codes (not part of the hp_layer ABI)
constexpr int OP_MLPHEAD = 101;
constexpr int OP_CHAIN = 102;
constexpr int OP_BNECK = 103;
// a single dense layer's launch, as the schedule rewrites look for it
inline bool plain_conv(const step& st) { return st.kind == launch_kind::conv16 && st.n_layers == 1; }

constexpr hp::tview NO_RES{ nullptr, 0, 0, 0, 0 }; // conv_params::res of a layer without a residual
constexpr hp::tview32 NO_RES32{ nullptr, 0, 0, 0, 0 };

void same_pad(int in, int k, int stride, int dil, int& out, int& pad_before)
{
    // TF "SAME": out = ceil(in / stride); pad_total = max((out-1)*stride + (k-1)*dil + 1 - in, 0); extra at the end
    out = (in + stride - 1) / stride;
    const int total = std::max((out - 1) * stride + (k - 1) * dil + 1 - in, 0);
    pad_before = total / 2;
}

} // namespace

struct hp_engine {
    int in_w = 0, in_h = 0, max_batch = 0;
    int dtype = HP_DTYPE_F16; // HP_DTYPE_F32: fp32 storage and arithmetic (the reference's data_type::kFLOAT), conv_fp32.hip;
                              // HP_DTYPE_F32S: the same engine with the dense layers' products on the fp16 pipe (conv32_direct.hip)
    bool is_f32() const { return dtype == HP_DTYPE_F32 || dtype == HP_DTYPE_F32S; }
    // HP_DTYPE_I8 (post-training quantization, TensorRT's kINT8): the fp16 engine's per-layer schedule (no fusions) with the layers conv_i8_kernel
    // covers on the int8 matrix pipe.  One float per layer: > 0 the layer runs int8 with this activation scale s_a, 0 it runs its fp16 kernel
    // (ineligible, or kept in fp16 by the caller), -1 eligible but not calibrated yet (such an engine does not infer).
    std::vector<float> i8_scale;
    std::vector<std::vector<float>> i8_sw; // per layer: the per-output-channel weight scales s_w[c] (empty for ineligible layers)
    bool i8_on(const step& st) const { return st.int8() && i8_scale[st.layer] > 0.f; }
    bool i8_eligible(int layer) const { return !i8_sw[layer].empty(); }
    int check_int8_scales(const float* s, int n, bool allow_uncalibrated) const;
    int apply_int8_scales(); // dq / inv_a of every int8 step from i8_scale; the caller has synchronised and dropped the graphs
    int drop_graphs();       // synchronise the device, then forget every captured graph (they hold the launches and arguments of the old schedule)
    // which engines may run a batch as two half-batches (hp_engine_set_concurrency): the fp32 engines (their steps take a frame offset)
    bool halves_ok() const { return is_f32(); }
    // HP_DTYPE_F32S: a pinned host word the split kernels OR into when an activation exceeds fp16's range (|x| > 65504); once seen
    // (hp_engine_synchronize / hp_engine_inference) the engine runs conv32_kernel instead - exact fp32 products, any range
    hp::host_buf ovf_flag;
    bool split_off = false;
    int split_fallbacks = 0;
    hp::call_args last; // the newest hp_engine_infer_* call
    bool on_split_pipe() const { return dtype == HP_DTYPE_F32S && !split_off; } // the direct kernel: on the fp16 pipe until a value left fp16's range, then on the fp32 pipe
    bool split_overflowed() const { return on_split_pipe() && ovf_flag.p && *static_cast<volatile unsigned*>(ovf_flag.p) != 0; }
    int leave_split(); // stop using conv32_direct_kernel: drop the captured graphs (they hold its launches), count the event
    hp::engine_switches switches; // read_engine_switches() at hp_engine_create / hp_engine_load
    double factor = 1.0 / 255;
    int flip_rb = 1;
    float mean[3] = { 0, 0, 0 }, inv_std[3] = { 1, 1, 1 };
    std::vector<hp_layer> layers;
    std::vector<hp_output_desc> out_descs; // as given (hp_engine_save)
    std::vector<float> weights_blob;       // as given (hp_engine_save)
    std::vector<std::unique_ptr<tensor_info>> tensors;
    std::vector<out_info> outputs; // sorted by name
    std::vector<step> steps;
    std::vector<std::unique_ptr<hp::dev_buf>> weight_bufs;
    // Activation arena (HP_DTYPE_F32 / F32S engines; HP_NO_ARENA=1 gives every tensor its own allocation, as before round 6).  TensorRT re-uses
    // activation memory between layers (the reference's engine owns only the binding buffers, src/tensorrt.cpp:255-316); here tensors of ONE
    // geometry class - same H x W, halo, channel stride and channel count, so that the zero halo and the zero pad channels of a buffer stay valid
    // for every tenant - take turns in the minimum number of buffers their lifetimes in the schedule need (interval colouring in layer order).
    struct arena_buf {
        std::unique_ptr<hp::dev_buf> mem;
        int tenants = 0;
    };
    std::vector<arena_buf> arena;
    size_t arena_private_bytes = 0; // what the same tensors took with one allocation each
    hp::dev_buf in_stage; // staging for host inputs, and the hp_engine_profile* calls' synthetic batch: max_batch fp32 frames
    int ensure_in_stage()
    {
        const size_t need = (size_t)max_batch * in_h * in_w * 3 * sizeof(float);
        return in_stage.bytes < need ? in_stage.alloc(need) : HP_OK;
    }
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // hp_engine_set_concurrency(2): a batch runs as two half-batches, the second on `stream2` (fork / join by events; inside a captured graph:
    // two parallel branches) - what a caller with ONE batch in flight gets instead of a second pipe (fp32 engines; frames are independent)
    int parts = 1;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    // captured graphs keyed by (n, input pointer, kind, first frame): csrc/graph_cache.hpp has the rules of their lifetime, call_plan.hpp the keys
    struct graph_destroy {
        void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); }
    };
    hp::graph_cache<hipGraphExec_t, graph_destroy> graphs;
    bool use_graph = true;

    // Flip ensemble (hp_engine_set_flip_ensemble; csrc/flip_ensemble.hpp): one table pair per output while on, empty while off.  A u8 batch of n
    // frames then runs as the 2n frames of flip_in - the caller's frames, their left-right flips behind them - and every output is merged in place.
    struct flip_table {
        std::vector<int32_t> perm;
        std::vector<int8_t> sign;
    };
    std::vector<flip_table> flip;
    hp::dev_buf flip_in; // [max_batch][in_h][in_w][3] u8: the staging buffer of both ensembles
    bool flip_on() const { return !flip.empty(); }
    // Scale ensemble (hp_engine_set_scale_ensemble; csrc/scale_ensemble.hpp): the K - 1 extra scales while on, empty while off.  A u8 batch of n
    // frames then runs as the K n slots of flip_in - the caller's frames, their shrunken copies behind them, scale-major - (and their flips behind
    // those when the flip ensemble is on too), and every output's frames [0, n) become the average of the K passes.
    std::vector<float> scale_ens;
    int scale_bgr[3] = { 0, 0, 0 };
    int scale_map_w = 0, scale_map_h = 0; // every output's W x H
    hp::dev_buf scale_tables;             // hp_scale::tap4 [K-1][W], then [K-1][H]
    int scale_k() const { return 1 + (int)scale_ens.size(); }
    // dev_src != nullptr: the n frames are copied into flip_in first (device to device); then, as the plan says, their shrunken copies are written
    // behind them (scales = K > 1) and the flips of all K n slots behind those (flip)
    int ensemble_stage(const uint8_t* dev_src, int n, int scales, bool with_flip, hipStream_t s) const;
    // hp_flip_merge on every output over the K n slots (flip), then the scale merge over the n frames (scales = K > 1): frames [0, n) become the ensemble
    int ensemble_merge(int n, int scales, bool with_flip, hipStream_t s) const;

    ~hp_engine() // (hp_engine_destroy has synchronised; `graphs` destroys what it still holds)
    {
        if (ev0)
            (void)hipEventDestroy(ev0);
        if (ev1)
            (void)hipEventDestroy(ev1);
        if (ev_fork)
            (void)hipEventDestroy(ev_fork);
        if (ev_join)
            (void)hipEventDestroy(ev_join);
        if (stream2)
            (void)hipStreamDestroy(stream2);
        if (stream)
            (void)hipStreamDestroy(stream);
    }

    int build(const hp_engine_desc* d);
    // build's passes, in order (engine.cpp)
    int validate_and_infer(const hp_engine_desc* d);
    int mark_pair_fusions(const hp_engine_desc* d);
    int bind_outputs(const hp_engine_desc* d);
    int plan_activations();
    int lower_layers();
    int lower_single(size_t i);
    // ... fp32 engines: one step per layer, or per fused pair (described at its second layer)
    int lower32_conv(size_t i, step& st);
    int lower32_dw_in_front(size_t i, step& st);
    int lower32_winograd_forms(size_t i, step& st, const std::vector<float>& packed, const hp::conv32_forms& f);
    int lower32_direct_forms(size_t i, step& st, const std::vector<float>& packed, const hp::conv32_forms& f);
    int lower32_head_in_front(size_t i, step& st, const float* w); // (turns the step's conv32_launch into a head32_launch)
    int lower32_dw(size_t i, step& st);
    // ... fp16 and int8 engines: one layer, a two-layer head, a separable block
    int lower16_first(size_t i, step& st);
    int lower16_conv(size_t i, step& st);
    int lower16_i8(size_t i, step& st, const float* w);
    int lower16_dw(size_t i, step& st);
    int lower16_head_pair(size_t i);
    int lower16_sep_pair(size_t i);
    // ... what the two precisions share (P: the fp16 / fp32 parameter struct of the same launch)
    template <typename P>
    int lower_first(size_t i, step& st, P& p, const float*& w);
    template <typename P>
    int lower_pool(size_t i, step& st, P& p);
    int plan_splitk();
    int fuse_chains();
    int fuse_bottlenecks();
    int fuse_sep_pairs();
    int pair_heads();
    int finish(const hp_engine_desc* d);
    // what the passes share
    std::vector<geo> geos;           // per layer
    std::vector<fuse_kind> fuse_next; // per layer: fused with the next layer (mark_pair_fusions)
    unsigned* ovf_dev = nullptr;     // HP_DTYPE_F32S: device view of ovf_flag
    // HP_NO_FUSE=1: one launch per layer.  An HP_DTYPE_I8 engine always runs that schedule: its fp16 layers are the kernels of the fp16 engine's
    // per-layer plan, its int8 layers replace single launches of it
    bool fuse_off() const { return dtype == HP_DTYPE_I8 || switches.no_fuse; }
    bool tensor_is_read(int t) const; // some layer reads it (input or residual), or an un-fused output conversion will
    // what every fusion asks before it keeps tensor t out of HBM: exactly one layer writes it, no layer but la / lb reads it (as input or
    // residual) and no bound network output exports it
    bool private_to(int t, int la, int lb) const;
    const float* blob(int64_t off, size_t n, const char* what, size_t layer) const; // weights_blob[off, off + n), or nullptr + error
    int upload(const void* src, size_t bytes, void** dst); // a new weight buffer holding src
    // ... what the lowerings repeat: a packed vector uploaded; n blob floats zero-padded to n_pad (off < 0: all zeros) fetched / uploaded;
    // a layer's PReLU slopes (nullptr without PReLU); its residual view; the fp32 network output its epilogue writes
    template <typename T>
    int upload(const std::vector<T>& v, const T*& dst)
    {
        void* d = nullptr;
        HP_TRY(upload(v.data(), v.size() * sizeof(T), &d));
        dst = static_cast<const T*>(d);
        return HP_OK;
    }
    bool fetch_padded(int64_t off, size_t n, size_t n_pad, const char* what, size_t layer, std::vector<float>& v) const;
    int upload_padded(int64_t off, size_t n, size_t n_pad, const char* what, size_t layer, const float*& dst);
    int upload_prelu(size_t layer, int n_pad, const float*& alpha);
    hp::tview res_view(int t) const { return t >= 0 ? tensors[t]->view(0) : NO_RES; }
    hp::tview32 res_view32(int t) const { return t >= 0 ? tensors[t]->view32(0) : NO_RES32; }
    template <typename V>
    float* fused_output(size_t layer, bool whole_tensor_only, V& out);
    int pointwise_params(size_t layer, int H, int W, int cout_pad, hp::conv_params& q); // the 1 x 1 second half of a fused fp16 pair
    hp::call_settings call_settings(bool ensemble, bool graph, int scales = 1) const { return { max_batch, parts, halves_ok(), ensemble, graph, scales }; }
    int run_call(const hp::call_settings& cfg, const hp::call_args& a); // one call, from its arguments to its launches: csrc/call_plan.hpp decides
    // ---- running the schedule: const, `steps` is written by build(), apply_int8_scales() and nobody else
    int enqueue_range(const uint8_t* u8, const float* f32, int b0, int n, hipStream_t s) const;
    // the step's parameters for frames [b0, b0 + n) of the batch at u8 / f32, as its launch gets them (and whether it is the int8 launch)
    launch_payload bound(const step& st, const uint8_t* u8, const float* f32, int n, int b0) const;
    int launch(launch_kind kind, launch_payload& bound, hipStream_t s, unsigned long long* dbg) const; // dbg: the launch's block-timeline stamps, or nullptr
    int launch_head_pair32(size_t i, int n, int b0, hipStream_t s, bool* done) const; // fp32 heads i and i + 1 in one grid, where the bound batch allows it
    int run_step(const step& st, const uint8_t* u8, const float* f32, int n, hipStream_t s, int b0 = 0) const;
    bool timeline_of(const step& st, const launch_payload& bound, hp::timeline_kind& kind, hp::timeline_header& hd) const; // which HP_*_DBG timeline the switches ask for
    int trace_step(const step& st, launch_payload& bound, hipStream_t s) const; // ... launched once more with its stamps, printed to stderr
    int tile_of(launch_kind kind, const launch_payload& bound) const;
    int step_tile(const step& st, int n) const; // hp_layer_time::tile: which kernel form the step launches on n frames (0: ops with one form)
    void fill_row(hp_layer_time* out, int k, int cap, const step& st, int n, float ms) const; // a profile row
};

bool hp_engine::tensor_is_read(int t) const
{
    for (const auto& L2 : layers)
        if (L2.in == t || L2.res == t)
            return true;
    for (const auto& o : outputs)
        if (o.tensor == t && o.fused_layer < 0)
            return true;
    return false;
}

const float* hp_engine::blob(int64_t off, size_t n, const char* what, size_t layer) const
{
    if (off < 0 || (size_t)off + n > weights_blob.size()) {
        hp::set_error("layer %zu: %s range [%lld,+%zu) outside the %zu-float weight blob", layer, what, (long long)off, n, weights_blob.size());
        return nullptr;
    }
    return weights_blob.data() + off;
}

bool hp_engine::private_to(int t, int la, int lb) const
{
    int writers = 0;
    for (size_t j = 0; j < layers.size(); ++j) {
        if ((int)j != la && (int)j != lb && (layers[j].in == t || layers[j].res == t))
            return false;
        writers += layers[j].out == t;
    }
    for (const auto& o : outputs)
        if (o.tensor == t)
            return false;
    return writers == 1;
}

int hp_engine::upload(const void* src, size_t bytes, void** dst)
{
    weight_bufs.push_back(std::make_unique<hp::dev_buf>());
    HP_TRY(weight_bufs.back()->alloc(bytes));
    HP_HIP_TRY(hipMemcpy(weight_bufs.back()->p, src, bytes, hipMemcpyHostToDevice));
    *dst = weight_bufs.back()->p;
    return HP_OK;
}

int hp_engine::build(const hp_engine_desc* d)
{
    HP_TRY(validate_and_infer(d)); // 1. the description, tensor shapes and halos
    HP_TRY(mark_pair_fusions(d));  // 2. which consecutive layers run as one launch
    HP_TRY(bind_outputs(d));       // 3. network outputs
    HP_TRY(plan_activations());    // 4. activation memory
    HP_TRY(lower_layers());        // 5. weights packed and uploaded, one step per layer or fused pair
    // 6. the fp16 schedule rewrites (each a no-op on fp32 engines and under HP_NO_FUSE)
    HP_TRY(plan_splitk());
    HP_TRY(fuse_chains());
    HP_TRY(fuse_bottlenecks());
    HP_TRY(fuse_sep_pairs());
    HP_TRY(pair_heads());
    return finish(d);              // 7. streams, events, int8 scales
}

int hp_engine::validate_and_infer(const hp_engine_desc* d)
{
    HP_REQUIRE(d->in_w > 0 && d->in_h > 0 && d->max_batch >= 1, HP_ERR_INVALID, "engine: bad input size / batch");
    HP_REQUIRE(d->layers && d->n_layers > 0 && d->weights, HP_ERR_INVALID, "engine: no layers / weights");
    in_w = d->in_w, in_h = d->in_h, max_batch = d->max_batch, factor = d->factor, flip_rb = d->flip_rb;
    HP_REQUIRE(d->dtype == HP_DTYPE_F16 || d->dtype == HP_DTYPE_F32 || d->dtype == HP_DTYPE_F32S || d->dtype == HP_DTYPE_I8, HP_ERR_INVALID,
        "engine: dtype %d is none of HP_DTYPE_F16 / HP_DTYPE_F32 / HP_DTYPE_F32S / HP_DTYPE_I8", d->dtype);
    dtype = d->dtype;
    if (dtype == HP_DTYPE_F32S) {
        HP_TRY(ovf_flag.alloc(64));
        memset(ovf_flag.p, 0, 64);
        HP_HIP_TRY(hipHostGetDevicePointer((void**)&ovf_dev, ovf_flag.p, 0));
    }
    for (int c = 0; c < 3; ++c)
        mean[c] = d->mean[c], inv_std[c] = d->inv_std[c];
    layers.assign(d->layers, d->layers + d->n_layers);
    out_descs.assign(d->outputs, d->outputs + (d->outputs ? d->n_outputs : 0));
    weights_blob.assign(d->weights, d->weights + d->n_weights);

    // ---- pass 1: tensor shapes
    int max_id = 0;
    for (const auto& L : layers)
        max_id = std::max({ max_id, L.in, L.out, L.res });
    HP_REQUIRE(max_id < (1 << 16) && d->n_layers < (1 << 16), HP_ERR_INVALID, "engine: %d layers / tensor id %d: not a plausible network", d->n_layers, max_id);
    for (size_t i = 0; i < layers.size(); ++i) {
        const hp_layer& L = layers[i];
        HP_REQUIRE(L.cin > 0 && L.cout > 0 && L.cin <= (1 << 16) && L.cout <= (1 << 16) && L.kh >= 0 && L.kh <= 31 && L.kw >= 0 && L.kw <= 31
                && L.stride >= 1 && L.stride <= 64 && L.dil >= 0 && L.dil <= 64,
            HP_ERR_INVALID, "layer %zu: implausible channel count / geometry", i);
        // channel offsets index device buffers: a negative one walks out of the front of the tensor
        HP_REQUIRE(L.in_coff >= 0 && L.in_coff <= (1 << 16) && L.out_coff >= 0 && L.out_coff + L.cout <= (1 << 16), HP_ERR_INVALID,
            "layer %zu: channel offsets in %d / out %d outside [0, 65536)", i, L.in_coff, L.out_coff);
        HP_REQUIRE(L.res >= -1 && L.res_before_act >= 0 && L.res_before_act <= 1, HP_ERR_INVALID, "layer %zu: bad residual fields", i);
        if (L.pad_explicit)
            for (int k = 0; k < 4; ++k)
                HP_REQUIRE(L.pad[k] >= 0 && L.pad[k] <= 64, HP_ERR_INVALID, "layer %zu: pad[%d] = %d outside [0, 64]", i, k, L.pad[k]);
        // a layer may read one channel slice of a concat buffer and write another, but never the channels it reads (the
        // blocks of one launch would race) - neither through its input nor through its residual
        if (L.in == L.out)
            HP_REQUIRE(L.in_coff + L.cin <= L.out_coff || L.out_coff + L.cout <= L.in_coff, HP_ERR_INVALID,
                "layer %zu reads channels [%d,%d) and writes [%d,%d) of the same tensor %d", i, L.in_coff, L.in_coff + L.cin, L.out_coff,
                L.out_coff + L.cout, L.out);
        if (L.res >= 0 && L.res == L.out)
            HP_REQUIRE(L.cout <= L.out_coff, HP_ERR_INVALID, "layer %zu adds channels [0,%d) of tensor %d while writing [%d,%d) of it", i, L.cout, L.res,
                L.out_coff, L.out_coff + L.cout);
    }
    tensors.resize(max_id + 1);
    for (auto& t : tensors)
        t = std::make_unique<tensor_info>();
    tensors[0]->defined = true, tensors[0]->H = in_h, tensors[0]->W = in_w, tensors[0]->C = 3;
    geos.assign(layers.size(), geo{});
    for (size_t i = 0; i < layers.size(); ++i) {
        const hp_layer& L = layers[i];
        HP_REQUIRE(L.in >= 0 && L.in <= max_id && tensors[L.in]->defined, HP_ERR_INVALID, "layer %zu reads undefined tensor %d", i, L.in);
        HP_REQUIRE(L.out > 0, HP_ERR_INVALID, "layer %zu: bad output tensor %d", i, L.out);
        HP_REQUIRE(L.op == HP_OP_CONV || L.op == HP_OP_DWCONV || L.op == HP_OP_MAXPOOL || L.op == HP_OP_UPSAMPLE, HP_ERR_INVALID, "layer %zu: unknown op %d", i, L.op);
        if (L.op == HP_OP_UPSAMPLE)
            HP_REQUIRE(L.stride >= 1 && L.stride <= 16 && (L.kh == 0 || L.kh == 1) && L.in != 0 && L.res < 0 && L.act == HP_ACT_NONE, HP_ERR_INVALID,
                "layer %zu: up-sampling takes an integer scale 1..16 in `stride`, kh = 0 (nearest) or 1 (bilinear), a feature-map input and no activation / residual", i);
        else
            HP_REQUIRE(L.stride >= 1 && L.kh >= 1 && L.kw >= 1 && L.dil >= 1, HP_ERR_INVALID, "layer %zu: bad geometry", i);
        const tensor_info& ti = *tensors[L.in];
        HP_REQUIRE(L.in_coff >= 0 && L.in_coff + L.cin <= ti.C, HP_ERR_INVALID, "layer %zu reads channels [%d,%d) of a %d-channel tensor", i, L.in_coff, L.in_coff + L.cin, ti.C);
        geo g;
        if (L.op == HP_OP_UPSAMPLE) {
            g.OH = ti.H * L.stride, g.OW = ti.W * L.stride, g.pt = g.pl = 0;
        } else if (L.pad_explicit) {
            HP_REQUIRE(L.pad[0] >= 0 && L.pad[1] >= 0 && L.pad[2] >= 0 && L.pad[3] >= 0, HP_ERR_INVALID, "layer %zu: negative padding", i);
            g.pt = L.pad[0], g.pl = L.pad[1];
            g.OH = (ti.H + L.pad[0] + L.pad[2] - ((L.kh - 1) * L.dil + 1)) / L.stride + 1;
            g.OW = (ti.W + L.pad[1] + L.pad[3] - ((L.kw - 1) * L.dil + 1)) / L.stride + 1;
            HP_REQUIRE(g.OH >= 1 && g.OW >= 1, HP_ERR_INVALID, "layer %zu: empty output", i);
        } else {
            same_pad(ti.H, L.kh, L.stride, L.dil, g.OH, g.pt);
            same_pad(ti.W, L.kw, L.stride, L.dil, g.OW, g.pl);
        }
        geos[i] = g;
        tensor_info& to = *tensors[L.out];
        if (!to.defined)
            to.defined = true, to.H = g.OH, to.W = g.OW;
        HP_REQUIRE(to.H == g.OH && to.W == g.OW, HP_ERR_INVALID, "layer %zu: writers of tensor %d disagree on its size", i, L.out);
        to.C = std::max(to.C, L.out_coff + L.cout);
        if (L.res >= 0) {
            HP_REQUIRE(tensors[L.res]->defined && tensors[L.res]->H == g.OH && tensors[L.res]->W == g.OW && tensors[L.res]->C >= L.cout,
                HP_ERR_INVALID, "layer %zu: residual tensor %d does not match the output", i, L.res);
        }
        if (L.op != HP_OP_CONV)
            HP_REQUIRE(L.cin == L.cout, HP_ERR_INVALID, "layer %zu: depthwise/pool need cin == cout", i);
        // (only the dense convolutions' epilogues add a residual: on a depthwise / pooling layer it would be dropped without a word)
        if (L.op != HP_OP_CONV)
            HP_REQUIRE(L.res < 0, HP_ERR_INVALID, "layer %zu: a residual on a depthwise / pooling layer is not supported", i);
        if (L.op != HP_OP_MAXPOOL && L.op != HP_OP_UPSAMPLE && L.in != 0) {
            // halo this consumer needs on its input: SAME padding before / after in both dimensions
            const int pb_y = std::max((g.OH - 1) * L.stride + (L.kh - 1) * L.dil + 1 - ti.H - g.pt, 0);
            const int pb_x = std::max((g.OW - 1) * L.stride + (L.kw - 1) * L.dil + 1 - ti.W - g.pl, 0);
            tensors[L.in]->P = std::max({ tensors[L.in]->P, g.pt, g.pl, pb_y, pb_x });
        }
    }
    return HP_OK;
}

int hp_engine::mark_pair_fusions(const hp_engine_desc* d)
{
    const bool f32 = is_f32();
    const bool no_fuse = fuse_off();
    fuse_next.assign(layers.size(), fuse_kind::none);
    // ---- what the four rules below share, for A = layer i and B = layer i + 1
    // B is a plain stride-1 1 x 1 that consumes all of A's output (A writes the whole tensor, at channel 0) and writes elsewhere
    auto pointwise_behind = [&](const hp_layer& A, const hp_layer& B) {
        return A.in != 0 && A.out_coff == 0 && tensors[A.out]->C == A.cout && B.op == HP_OP_CONV && B.kh == 1 && B.kw == 1 && B.stride == 1
            && B.in == A.out && B.in_coff == 0 && B.cin == A.cout && B.out != A.out;
    };
    // layer j does not pad and the map keeps its size (a padded 1x1 - ONNX pads - changes it: the fused launches assume it does not)
    auto keeps_map = [&](size_t j) {
        return geos[j].OH == tensors[layers[j].in]->H && geos[j].OW == tensors[layers[j].in]->W && geos[j].pt == 0 && geos[j].pl == 0;
    };
    // (the outputs are not bound yet, pass 3: the description's own list)
    auto is_output = [&](int t) {
        for (int o = 0; o < d->n_outputs; ++o)
            if (d->outputs[o].tensor == t)
                return true;
        return false;
    };
    // A's output is private to the pair: written by A alone, read by B alone, no network output - it is never materialised
    auto private_to_pair = [&](size_t i) { return private_to(layers[i].out, (int)i + 1, (int)i + 1) && !is_output(layers[i].out); };
    auto dw3x3 = [](const hp_layer& A) { return A.op == HP_OP_DWCONV && A.kh == 3 && A.kw == 3; };
    auto conv1x1 = [](const hp_layer& A) { return A.op == HP_OP_CONV && A.kh == 1 && A.kw == 1 && A.stride == 1 && A.res < 0; };
    auto post_op_act = [](const hp_layer& B) { return B.act == HP_ACT_SIGMOID || B.act == HP_ACT_SOFTPLUS; };
    auto fuse = [&](size_t i, fuse_kind k) { fuse_next[i] = k, tensors[layers[i].out]->elided = true; };
    // ---- separable blocks: a depthwise layer whose only consumer is the next layer, a plain 1x1 convolution, runs
    // as ONE launch (sepconv_kernel) and its output tensor is never materialised.  HP_NO_FUSE=1 keeps the two launches.
    if (!no_fuse && !f32) {
        for (size_t i = 0; i + 1 < layers.size(); ++i) {
            const hp_layer &A = layers[i], &Bn = layers[i + 1];
            if (!dw3x3(A) || A.in_coff % 8 || !pointwise_behind(A, Bn) || Bn.res >= 0 || Bn.cout % 8 || Bn.out_coff % 8)
                continue;
            if ((A.act != HP_ACT_RELU && A.act != HP_ACT_RELU6) || post_op_act(Bn))
                continue; // the fused kernel evaluates the depthwise activation as one clamp
            {   // the fused kernel is configured for TF-SAME geometry: explicit pads must reproduce it, the 1x1 half must not pad at all
                int oh, ow, pt, pl;
                same_pad(tensors[A.in]->H, 3, A.stride, A.dil, oh, pt);
                same_pad(tensors[A.in]->W, 3, A.stride, A.dil, ow, pl);
                if (geos[i].OH != oh || geos[i].OW != ow || geos[i].pt != pt || geos[i].pl != pl || !keeps_map(i + 1))
                    continue;
            }
            if (!private_to_pair(i) || is_output(Bn.out))
                continue; // network outputs keep the generic epilogue (fp32 NCHW copy): this rule alone also refuses B's tensor as one
            const int cout_pad = round_up(Bn.cout, 128);
            const int variant = hp::sepconv_variant_for(A.cin, cout_pad, A.stride, A.dil, Bn.cout);
            if (!variant || (Bn.cout <= 64 && variant != 7))
                continue; // (<= 64 output channels idle half of the general fused kernels' wavefronts - slower than two launches - except in the dedicated 32-channel form)
            fuse(i, fuse_kind::sep);
        }
    }
    // ---- fp32 engines: the same pairing for conv32_direct_kernel's depthwise-fused forms (stride 1, dilation 1 | 2, whole 64-channel chunks;
    // whether the 1 x 1 half takes them is decided where its parameters are known: pass 2).  HP_NO_FUSE=1 / HP_NO_FUSE32=1 keep two launches.
    // Default: HP_DTYPE_F32S only (HP_FUSE32=1 fuses on the fp32 pipe too: tests).  Measured on LW-OpenPose @ 8 x 46 x 54, us per batch alone |
    // with a second stream, fused -> two launches: split 1528 | 1077 -> 1514 | 1079 (nothing lost, one 40 MB tensor per block not allocated);
    // fp32 pipe 2880 | 2294 -> 2671 | 1984: conv32_direct_kernel's fused forms compute the depthwise tile once per 128-channel block of the 1 x 1
    // layer (4 x at 512 outputs) between two barriers, the MFMA pipe idle meanwhile - 194 us for dw + 512 -> 512 against 24.5 + 100.  A second
    // attempt in round 5 - one block per pixel tile owning ALL 512 outputs (eight wavefronts, 16-channel chunks double-buffered, the depthwise
    // reads hidden under the chunk's 32 MFMAs, one barrier per chunk) - computed the depthwise tile once and still ran 161 us alone / 108 with
    // a second stream against 125 / 107 for the two launches (profiles/r05_ab_layers_f32_sep_kernel.txt): one block of eight wavefronts per CU
    // moves in step with its own barrier, where conv32_kernel's four independent blocks per CU fill each other's gaps.  Not adopted, removed.
    if (f32 && !no_fuse && !switches.no_fuse32 && (dtype == HP_DTYPE_F32S || switches.fuse32)) {
        for (size_t i = 0; i + 1 < layers.size(); ++i) {
            const hp_layer &A = layers[i], &Bn = layers[i + 1];
            if (!dw3x3(A) || A.in_coff % 4 || A.stride != 1 || (A.dil != 1 && A.dil != 2) || A.cin % 64 || A.res >= 0)
                continue;
            if (A.act != HP_ACT_NONE && A.act != HP_ACT_RELU && A.act != HP_ACT_RELU6 && A.act != HP_ACT_LEAKY)
                continue;
            if (!pointwise_behind(A, Bn) || Bn.res == A.out)
                continue;
            if (geos[i].OH != tensors[A.in]->H || geos[i].OW != tensors[A.in]->W || geos[i].pt != A.dil || geos[i].pl != A.dil || !keeps_map(i + 1))
                continue; // TF-SAME geometry of a stride-1 3 x 3: the map keeps its size, the padding is the dilation; the 1 x 1 half does not pad
            if (!private_to_pair(i))
                continue;
            // the 1 x 1 half as pass 2 will describe it, to ask the kernel family whether a fused form exists for its size
            hp::conv32_params q{};
            q.B = max_batch, q.H = q.OH = geos[i].OH, q.W = q.OW = geos[i].OW, q.Cin = Bn.cin, q.Cout = Bn.cout, q.Cout_pad = round_up(Bn.cout, 64);
            q.KH = q.KW = 1, q.stride = 1, q.dil = 1, q.pad_t = q.pad_l = 0, q.npix = max_batch * q.OH * q.OW;
            // (an HP_DTYPE_F32S engine must also be able to run the block on the fp32 pipe: where it goes when a value leaves fp16's range)
            if (!hp::pick32::dw_fusable(q, false, A.dil) || (dtype == HP_DTYPE_F32S && !hp::pick32::dw_fusable(q, true, A.dil)))
                continue;
            fuse(i, fuse_kind::sep32);
        }
    }
    // ---- two-layer heads: 1x1 K1 -> 512 (relu) whose only consumer is the next layer, a 1x1 512 -> <= 64 channels
    if (!no_fuse && !f32) {
        for (size_t i = 0; i + 1 < layers.size(); ++i) {
            const hp_layer &A = layers[i], &Bn = layers[i + 1];
            if (!conv1x1(A) || A.in_coff % 8 || (A.act != HP_ACT_RELU && A.act != HP_ACT_RELU6))
                continue;
            if (!pointwise_behind(A, Bn) || Bn.res >= 0 || post_op_act(Bn) || !keeps_map(i) || !keeps_map(i + 1))
                continue;
            if (!hp::mlp_head_variant(A.cin, A.cout, Bn.cout, switches.no_fuse_head))
                continue;
            if (i > 0 && (fuse_next[i - 1] == fuse_kind::sep))
                continue; // already the pointwise half of a separable block
            if (private_to_pair(i))
                fuse(i, fuse_kind::head);
        }
    }
    // ---- HP_DTYPE_F32: the same two-layer heads for conv32_head_kernel (1 x 1 128 -> HID, ReLU family, sole consumer a 1 x 1 HID -> <= 64
    // channels; the hidden tensor stays in registers).  HP_NO_FUSE=1 / HP_NO_HEAD32=1 keep two launches.
    if (dtype == HP_DTYPE_F32 && !no_fuse && !switches.no_head32) {
        for (size_t i = 0; i + 1 < layers.size(); ++i) {
            const hp_layer &A = layers[i], &Bn = layers[i + 1];
            if (!conv1x1(A) || A.in_coff % 4 || (A.act != HP_ACT_NONE && A.act != HP_ACT_RELU && A.act != HP_ACT_RELU6 && A.act != HP_ACT_LEAKY))
                continue;
            if (!pointwise_behind(A, Bn) || Bn.res >= 0 || post_op_act(Bn) || !keeps_map(i) || !keeps_map(i + 1))
                continue;
            if (!hp::pick32::head_ok(A.cin, A.cout, Bn.cout) || A.in_coff + A.cin > round_up(tensors[A.in]->C, 32))
                continue;
            if ((i > 0 && (fuse_next[i - 1] == fuse_kind::sep32)) || (fuse_next[i] == fuse_kind::sep32))
                continue;
            if (private_to_pair(i))
                fuse(i, fuse_kind::head32);
        }
    }
    return HP_OK;
}

int hp_engine::bind_outputs(const hp_engine_desc* d)
{
    // ---- outputs
    HP_REQUIRE(d->n_outputs >= 1 && d->outputs, HP_ERR_INVALID, "engine: no outputs");
    for (int i = 0; i < d->n_outputs; ++i) {
        const hp_output_desc& o = d->outputs[i];
        HP_REQUIRE(o.tensor > 0 && o.tensor < (int)tensors.size() && tensors[o.tensor]->defined, HP_ERR_INVALID, "output %d: bad tensor", i);
        const tensor_info& ti = *tensors[o.tensor];
        HP_REQUIRE(o.coff >= 0 && o.channels > 0 && o.coff + o.channels <= ti.C, HP_ERR_INVALID, "output %d: bad channel range", i);
        out_info oi;
        oi.name.assign(o.name, strnlen(o.name, sizeof(o.name)));
        oi.tensor = o.tensor, oi.coff = o.coff, oi.channels = o.channels, oi.act = o.act, oi.H = ti.H, oi.W = ti.W;
        oi.x.C = o.channels, oi.x.act = o.act, oi.x.shuffle = o.shuffle == 2 ? 2 : 1, oi.x.group = o.group;
        oi.x.sigmoid_mask = o.sigmoid_mask, oi.x.softplus_mask = o.softplus_mask;
        HP_REQUIRE(o.shuffle == 0 || o.shuffle == 1 || o.shuffle == 2, HP_ERR_INVALID, "output %d: shuffle must be 0, 1 or 2", i);
        HP_REQUIRE(o.group >= 0 && o.group <= 32 && (o.group == 0 || (o.channels / (oi.x.shuffle * oi.x.shuffle)) % o.group == 0), HP_ERR_INVALID,
            "output %d: group %d must be 0 or divide the channel count (<= 32 components)", i, o.group);
        HP_REQUIRE(o.grid >= 0 && o.grid <= 2 && (o.act == HP_ACT_NONE || o.act == HP_ACT_SIGMOID || o.act == HP_ACT_SOFTPLUS) && o.out_h >= 0
                && o.out_w >= 0 && std::isfinite(o.scale),
            HP_ERR_INVALID, "output %d: bad grid / act / crop / scale", i);
        if (o.group > 0 && o.group < 32)
            HP_REQUIRE((o.sigmoid_mask >> o.group) == 0 && (o.softplus_mask >> o.group) == 0, HP_ERR_INVALID,
                "output %d: sigmoid / softplus masks name components beyond group %d", i, o.group);
        HP_REQUIRE(oi.x.C % (oi.x.shuffle * oi.x.shuffle) == 0, HP_ERR_INVALID, "output %d: channels not divisible by shuffle^2", i);
        oi.x.out_h = o.out_h > 0 ? o.out_h : ti.H * oi.x.shuffle, oi.x.out_w = o.out_w > 0 ? o.out_w : ti.W * oi.x.shuffle;
        HP_REQUIRE(oi.x.out_h <= ti.H * oi.x.shuffle && oi.x.out_w <= ti.W * oi.x.shuffle, HP_ERR_INVALID, "output %d: crop larger than the map", i);
        oi.x.scale = o.scale == 0.f ? 1.f : o.scale, oi.x.grid = o.grid;
        outputs.push_back(std::move(oi));
    }
    std::stable_sort(outputs.begin(), outputs.end(), [](const out_info& a, const out_info& b) { return a.name < b.name; }); // tensorrt.cpp:405
    for (auto& o : outputs) {
        o.buf = std::make_unique<hp::dev_buf>();
        HP_TRY(o.buf->alloc((size_t)max_batch * o.out_c() * o.x.out_h * o.x.out_w * sizeof(float)));
        // fuse into the producing conv when one MFMA conv writes exactly this channel range and no post-op is needed
        int writers = 0, last = -1;
        for (size_t i = 0; i < layers.size(); ++i)
            if (layers[i].out == o.tensor && layers[i].out_coff < o.coff + o.channels && layers[i].out_coff + layers[i].cout > o.coff)
                ++writers, last = (int)i;
        // (a convolution carries ONE fp32 pointer: where the same range is exported under several names the first takes it, the others
        // stay with the conversion kernel - which keeps the fp16 / fp32 tensor alive, tensor_is_read)
        bool taken = false;
        for (const auto& o2 : outputs)
            taken = taken || (&o2 != &o && o2.fused_layer == last && last >= 0);
        if (writers == 1 && !taken && layers[last].op == HP_OP_CONV && layers[last].in != 0 && layers[last].out_coff == o.coff
            && layers[last].cout == o.channels && o.act == HP_ACT_NONE && o.plain())
            o.fused_layer = last;
    }

    return HP_OK;
}

int hp_engine::plan_activations()
{
    const bool f32 = is_f32();
    // ---- activation memory.  fp16 engines: one zero-filled allocation per tensor.  fp32 engines: the arena (see hp_engine::arena).
    {
        const bool use_arena = f32 && !switches.no_arena;
        const int NL = (int)layers.size(), INF = NL + 1;
        std::vector<int> first(tensors.size(), INF), last(tensors.size(), -1);
        for (int i = 0; i < NL; ++i) {
            const hp_layer& L = layers[i];
            // the step a layer's reads happen in: the first half of a fused pair (depthwise / hidden head layer) runs inside the NEXT layer's launch
            const int at = ((fuse_next[i] == fuse_kind::sep32) || (fuse_next[i] == fuse_kind::head32)) ? i + 1 : i;
            first[L.out] = std::min(first[L.out], i);
            last[L.out] = std::max(last[L.out], i);
            if (L.in > 0)
                last[L.in] = std::max(last[L.in], at);
            if (L.res >= 0)
                last[L.res] = std::max(last[L.res], at);
        }
        for (const auto& o : outputs)
            if (o.fused_layer < 0)
                last[o.tensor] = INF; // read by the conversion kernel behind the last layer
        struct cls_key {
            int H, W, P, cs, C;
            bool operator<(const cls_key& o) const { return std::tie(H, W, P, cs, C) < std::tie(o.H, o.W, o.P, o.cs, o.C); }
        };
        std::map<cls_key, std::vector<int>> free_slots; // arena slots of a class nobody lives in at the moment
        std::vector<std::vector<int>> dying(NL + 2);
        for (size_t t = 1; t < tensors.size(); ++t) {
            tensor_info& ti = *tensors[t];
            if (!ti.defined || ti.elided)
                continue;
            ti.cs = round_up(ti.C, 32);
        }
        auto bytes_of = [&](const tensor_info& ti) { return (size_t)max_batch * (f32 ? ti.rows32() : ti.H + 2 * ti.P) * (ti.W + 2 * ti.P) * ti.cs * (f32 ? sizeof(float) : sizeof(__half)); };
        if (!use_arena) {
            for (size_t t = 1; t < tensors.size(); ++t) {
                tensor_info& ti = *tensors[t];
                if (!ti.defined || ti.elided)
                    continue;
                HP_TRY(ti.buf.alloc(bytes_of(ti)));
                HP_HIP_TRY(hipMemset(ti.buf.p, 0, bytes_of(ti))); // the halo and the pad channels must read as zero, forever
            }
        } else {
            for (int i = 0; i < NL; ++i) {
                const int t = layers[i].out;
                tensor_info& ti = *tensors[t];
                if (first[t] == i && !ti.elided && ti.arena_slot < 0) {
                    const cls_key key{ ti.H, ti.W, ti.P, ti.cs, ti.C };
                    auto& fl = free_slots[key];
                    int slot;
                    if (!fl.empty()) {
                        slot = fl.back();
                        fl.pop_back();
                    } else {
                        slot = (int)arena.size();
                        arena.emplace_back();
                        arena.back().mem = std::make_unique<hp::dev_buf>();
                        HP_TRY(arena.back().mem->alloc(bytes_of(ti)));
                        HP_HIP_TRY(hipMemset(arena.back().mem->p, 0, bytes_of(ti))); // halo and pad channels: zero for every tenant, forever
                    }
                    ti.arena_slot = slot, ti.shared = arena[slot].mem->p;
                    ++arena[slot].tenants;
                    arena_private_bytes += bytes_of(ti);
                    dying[std::min(std::max(last[t], i), NL + 1)].push_back(t);
                }
                for (int d : dying[i]) { // tensors whose last reader is this step: their buffers are free from the next step on
                    const tensor_info& td = *tensors[d];
                    free_slots[cls_key{ td.H, td.W, td.P, td.cs, td.C }].push_back(td.arena_slot);
                }
            }
        }
    }
    return HP_OK;
}

bool hp_engine::fetch_padded(int64_t off, size_t n, size_t n_pad, const char* what, size_t layer, std::vector<float>& v) const
{
    const float* src = off < 0 ? nullptr : blob(off, n, what, layer);
    if (off >= 0 && !src)
        return false;
    v = hp::wpack::padded(src, n, n_pad);
    return true;
}

int hp_engine::upload_padded(int64_t off, size_t n, size_t n_pad, const char* what, size_t layer, const float*& dst)
{
    std::vector<float> v;
    if (!fetch_padded(off, n, n_pad, what, layer, v))
        return HP_ERR_INVALID;
    return upload(v, dst);
}

int hp_engine::upload_prelu(size_t layer, int n_pad, const float*& alpha)
{
    const hp_layer& L = layers[layer];
    alpha = nullptr;
    if (L.act != HP_ACT_PRELU)
        return HP_OK;
    HP_REQUIRE(L.alpha_off >= 0, HP_ERR_INVALID, "layer %zu: PReLU without slopes", layer);
    return upload_padded(L.alpha_off, L.cout, n_pad, "prelu slopes", layer, alpha);
}

// The fp32 network output the layer's epilogue writes (bind_outputs), or nullptr.  With one, a tensor nobody reads is not written at all
// (`out.p` cleared) - whole_tensor_only: unless the layer writes a slice of a wider tensor
template <typename V>
float* hp_engine::fused_output(size_t layer, bool whole_tensor_only, V& out)
{
    const hp_layer& L = layers[layer];
    float* f32 = nullptr;
    for (auto& o : outputs)
        if (o.fused_layer == (int)layer)
            f32 = o.buf->as<float>();
    if (f32 && !tensor_is_read(L.out) && (!whole_tensor_only || tensors[L.out]->C == L.cout))
        out.p = nullptr, tensors[L.out]->unwritten = true; // only the fp32 network output is wanted
    return f32;
}

// The second layer of a fused fp16 pair (a separable block's pointwise layer, a head's output layer) as a 1 x 1 conv_params on an H x W map:
// bias and slopes padded to cout_pad, activation, outputs.  q.w is the caller's.
int hp_engine::pointwise_params(size_t layer, int H, int W, int cout_pad, hp::conv_params& q)
{
    const hp_layer& Pn = layers[layer];
    HP_TRY(upload_padded(Pn.b_off, Pn.cout, cout_pad, "bias", layer, q.bias));
    HP_TRY(upload_prelu(layer, cout_pad, q.alpha));
    q.H = H, q.W = W, q.OH = H, q.OW = W, q.Cin = Pn.cin, q.Cout = Pn.cout, q.Cout_pad = cout_pad;
    q.KH = q.KW = 1, q.stride = 1, q.dil = 1, q.pad_t = q.pad_l = 0;
    q.act = Pn.act, q.act_param = Pn.act_param;
    q.res = NO_RES, q.res_before_act = 0;
    q.out = tensors[Pn.out]->view(Pn.out_coff);
    q.out_f32 = fused_output(layer, false, q.out), q.dbg = nullptr;
    HP_REQUIRE(hp::set_act(q), HP_ERR_INVALID, "layer %zu: activation %d cannot be fused into a dense conv", layer, Pn.act);
    return HP_OK;
}

int hp_engine::lower_layers()
{
    i8_sw.assign(layers.size(), {});
    for (size_t i = 0; i < layers.size(); ++i) {
        if (fuse_next[i] == fuse_kind::head || fuse_next[i] == fuse_kind::sep) { // the fp16 pairs: one step, described here
            HP_TRY(fuse_next[i] == fuse_kind::head ? lower16_head_pair(i) : lower16_sep_pair(i));
            ++i; // the second layer is part of this step
        } else
            HP_TRY(lower_single(i));
    }
    return HP_OK;
}

namespace {
inline void set_view(hp::tview& v, const tensor_info& t, int coff) { v = t.view(coff); }
inline void set_view(hp::tview32& v, const tensor_info& t, int coff) { v = t.view32(coff); }
} // namespace

// The 3-channel first convolution, for first_conv_params and first_conv32_params alike: the fp32 weights [Cout][KH][KW][3] as the blob has
// them (`w`), the bias, pre-processing and geometry
template <typename P>
int hp_engine::lower_first(size_t i, step& st, P& p, const float*& w)
{
    const hp_layer& L = layers[i];
    const tensor_info& ti = *tensors[L.in];
    const geo& g = geos[i];
    HP_REQUIRE(L.cin == 3 && L.in_coff == 0, HP_ERR_INVALID, "layer %zu: the network input has 3 channels", i);
    HP_REQUIRE(L.dil == 1 && L.res < 0 && L.act != HP_ACT_PRELU, HP_ERR_INVALID, "layer %zu: unsupported first-layer options", i);
    const size_t nw = (size_t)L.cout * L.kh * L.kw * 3;
    w = blob(L.w_off, nw, "weights", i);
    if (!w)
        return HP_ERR_INVALID;
    p.factor = factor, p.flip_rb = flip_rb;
    for (int c = 0; c < 3; ++c)
        p.mean[c] = mean[c], p.inv_std[c] = inv_std[c];
    p.H = ti.H, p.W = ti.W, p.OH = g.OH, p.OW = g.OW, p.Cout = L.cout, p.KH = L.kh, p.KW = L.kw, p.stride = L.stride;
    p.pad_t = g.pt, p.pad_l = g.pl, p.act = L.act, p.act_param = L.act_param;
    void* dw = nullptr;
    HP_TRY(upload(w, nw * sizeof(float), &dw));
    p.w = (const float*)dw;
    HP_TRY(upload_padded(L.b_off, L.cout, round_up(L.cout, 8), "bias", i, p.bias));
    set_view(p.out, *tensors[L.out], L.out_coff);
    const double opix = (double)g.OH * g.OW;
    st.flops = 2.0 * opix * L.cout * L.kh * L.kw * 3;
    st.bytes = (double)ti.H * ti.W * 3 + opix * L.cout * sizeof(*p.out.p) + nw * 4;
    return HP_OK;
}

// Max-pool / up-sampling, for pool_params and pool32_params alike: 16-byte channel groups (8 halves, 4 floats); up-sampling does not pad
template <typename P>
int hp_engine::lower_pool(size_t i, step& st, P& p)
{
    const hp_layer& L = layers[i];
    const tensor_info& ti = *tensors[L.in];
    const geo& g = geos[i];
    const int elem = sizeof(*p.in.p), align = 16 / elem;
    const bool up = L.op == HP_OP_UPSAMPLE;
    HP_REQUIRE(L.cin % align == 0 && L.in_coff % align == 0 && L.out_coff % align == 0 && (up || L.kh == L.kw), HP_ERR_INVALID,
        "layer %zu: pooling / up-sampling needs %d-aligned channels and a square window", i, align);
    set_view(p.in, ti, L.in_coff);
    p.H = ti.H, p.W = ti.W, p.OH = g.OH, p.OW = g.OW, p.C = L.cin, p.k = L.kh, p.stride = L.stride;
    p.pad_t = up ? 0 : g.pt, p.pad_l = up ? 0 : g.pl;
    set_view(p.out, *tensors[L.out], L.out_coff);
    st.flops = 0;
    st.bytes = (double)ti.H * ti.W * L.cin * elem + (double)g.OH * g.OW * L.cin * elem; // (whole numbers: exact in any order)
    return HP_OK;
}

// One layer as one step.  HP_DTYPE_F32 / F32S: an fp32 launch (conv_fp32.hip), which for a fused pair is described at its second layer
int hp_engine::lower_single(size_t i)
{
    const hp_layer& L = layers[i];
    step st;
    st.layer = (int)i, st.op = L.op;
    const bool f32 = is_f32();
    if (f32 && (fuse_next[i] == fuse_kind::sep32 || fuse_next[i] == fuse_kind::head32)) // the first half of a fused pair: described at the 1 x 1 layer that follows
        return HP_OK;
    const float* w = nullptr;
    if (L.op == HP_OP_CONV && L.in == 0)
        HP_TRY(f32 ? lower_first(i, st, st.set<hp::first_conv32_params>(launch_kind::first32), w) : lower16_first(i, st));
    else if (L.op == HP_OP_CONV)
        HP_TRY(f32 ? lower32_conv(i, st) : lower16_conv(i, st));
    else if (L.op == HP_OP_DWCONV)
        HP_TRY(f32 ? lower32_dw(i, st) : lower16_dw(i, st));
    else if (const bool up = L.op == HP_OP_UPSAMPLE; f32)
        HP_TRY(lower_pool(i, st, st.set<hp::pool32_params>(up ? launch_kind::upsample32 : launch_kind::maxpool32)));
    else
        HP_TRY(lower_pool(i, st, st.set<hp::pool_params>(up ? launch_kind::upsample16 : launch_kind::maxpool16)));
    steps.push_back(st);
    return HP_OK;
}

// a dense fp32 layer: conv32_kernel's rows, then the forms of the other kernels that take it
int hp_engine::lower32_conv(size_t i, step& st)
{
    const hp_layer& L = layers[i];
    const tensor_info& ti = *tensors[L.in];
    const geo& g = geos[i];
    const double opix = (double)g.OH * g.OW;
    const bool dw_in_front = i > 0 && (fuse_next[i - 1] == fuse_kind::sep32);
    const bool head_in_front = i > 0 && (fuse_next[i - 1] == fuse_kind::head32);
    const int cin_pad = round_up(L.cin, 16), cout_pad = round_up(L.cout, 64), taps = L.kh * L.kw;
    // (behind a fused depthwise / hidden layer the tensor this layer "reads" is never materialised: what the kernel reads is THAT layer's input)
    const hp_layer& S = (dw_in_front || head_in_front) ? layers[i - 1] : L;
    const tensor_info& tsrc = *tensors[S.in];
    HP_REQUIRE(S.in_coff % 4 == 0 && S.in_coff + (head_in_front ? S.cin : cin_pad) <= tsrc.cs, HP_ERR_INVALID,
        "layer %zu: channel slice [%d,+%d) not 4-aligned / exceeds the padded stride %d", i, S.in_coff, cin_pad, tsrc.cs);
    const size_t nw = (size_t)L.cout * taps * L.cin;
    const float* w = blob(L.w_off, nw, "weights", i);
    if (!w)
        return HP_ERR_INVALID;
    auto& p = st.set<conv32_launch>(launch_kind::conv32).cp;
    HP_TRY(upload_padded(L.b_off, L.cout, cout_pad, "bias", i, p.bias));
    HP_TRY(upload_prelu(i, cout_pad, p.alpha));
    const std::vector<float> packed = hp::wpack::dense32_rows(w, L.cout, taps, L.cin, cout_pad, cin_pad);
    HP_TRY(upload(packed, p.w));
    p.in = ti.view32(L.in_coff);
    p.H = ti.H, p.W = ti.W, p.OH = g.OH, p.OW = g.OW, p.Cin = cin_pad, p.Cout = L.cout, p.Cout_pad = cout_pad;
    p.KH = L.kh, p.KW = L.kw, p.stride = L.stride, p.dil = L.dil, p.pad_t = g.pt, p.pad_l = g.pl;
    hp::set_geom32(p); // (the kernels' division constants: OW and OH * OW do not change with the call's batch)
    p.dw_w = nullptr, p.dw_dil = 0, p.dw_slope = 1.f, p.dw_hi = __builtin_huge_valf();
    st.flops = 2.0 * opix * L.cout * taps * L.cin;
    st.bytes = (double)ti.H * ti.W * L.cin * 4 + opix * L.cout * 4 + (double)nw * 4;
    if (dw_in_front)
        HP_TRY(lower32_dw_in_front(i, st));
    p.act = L.act, p.act_param = L.act_param;
    p.res = res_view32(L.res), p.res_before_act = L.res_before_act;
    p.out = tensors[L.out]->view32(L.out_coff);
    p.out_f32 = fused_output(i, true, p.out);
    HP_REQUIRE(hp::set_act32(p), HP_ERR_INVALID, "layer %zu: activation %d cannot be fused into a dense conv (use an output post-op)", i, L.act);
    p.B = max_batch, p.npix = p.pick_npix = max_batch * g.OH * g.OW;
    p.w_split = nullptr, p.w_frag = nullptr, p.w_wino = nullptr, p.ovf = ovf_dev, p.dbg = nullptr;
    p.lane_epilogue = switches.lane_epilogue;
    // the weight forms of the kernels beside conv32_kernel: conv32_layer_forms looks at the filled p and decides, the two lowerings pack and upload
    const hp::conv32_forms f = hp::conv32_layer_forms(p, dtype, switches, dw_in_front, tsrc.cs - S.in_coff, L.cin);
    HP_REQUIRE(!dw_in_front || f.kind == hp::C32_DIRECT, HP_ERR_STATE, "layer %zu: fused behind a depthwise layer but not a direct-kernel layer (engine bug)", i);
    HP_TRY(lower32_winograd_forms(i, st, packed, f));
    HP_TRY(lower32_direct_forms(i, st, packed, f));
    // (the launch kind is the picker's: the lowerings above only packed what it asked for)
    st.kind = f.kind == hp::C32_WINO2 ? launch_kind::wino2 : f.kind == hp::C32_DIRECT ? launch_kind::direct : launch_kind::conv32;
    if (head_in_front) // (last: it replaces the payload `p` refers to)
        HP_TRY(lower32_head_in_front(i, st, w));
    return HP_OK;
}

// conv32_direct_kernel's fused form behind depthwise layer i - 1: `in` is that layer's input, its weights ride along as [9][C] + [C]
int hp_engine::lower32_dw_in_front(size_t i, step& st)
{
    const hp_layer &D = layers[i - 1], &L = layers[i];
    auto& p = st.cp32();
    const float* dwf = blob(D.w_off, (size_t)D.cin * 9, "weights", i - 1);
    std::vector<float> dbias;
    if (!dwf || !fetch_padded(D.b_off, D.cin, D.cin, "bias", i - 1, dbias))
        return HP_ERR_INVALID;
    HP_TRY(upload(hp::wpack::dw_taps32_bias(dwf, dbias.data(), D.cin), p.dw_w));
    p.dw_dil = D.dil;
    p.dw_slope = D.act == HP_ACT_NONE ? 1.f : D.act == HP_ACT_LEAKY ? D.act_param : 0.f;
    p.dw_hi = D.act == HP_ACT_RELU6 ? 6.f : __builtin_huge_valf();
    p.in = tensors[D.in]->view32(D.in_coff);
    st.layer = (int)i - 1, st.n_layers = 2;
    // + the depthwise taps; the tensor between the two layers costs no bytes any more
    st.flops += 2.0 * ((double)geos[i].OH * geos[i].OW) * L.cin * 9, st.bytes += (double)L.cin * 10 * 4;
    return HP_OK;
}

// HP_DTYPE_F32: 3 x 3 stride-1 layers in Winograd's F(2 x 2, 3 x 3) form - 16 MFMA products per 2 x 2 output tile and channel pair
// instead of 36 (conv32_winograd.hip; HP_NO_WINOGRAD32=1 is the A/B switch back to the direct kernel).  The step's `flops` stay the
// layer's ALGORITHMIC count (the direct form's 2 * 9 * Cin * Cout per pixel); the MFMA work issued is 16 / 36 of it (bench.py reports both).
// (Never a layer with a depthwise or hidden layer fused in front: those are 1 x 1.)
int hp_engine::lower32_winograd_forms(size_t i, step& st, const std::vector<float>& packed, const hp::conv32_forms& f)
{
    auto& p = st.cp32();
    if (!f.w_wino)
        return HP_OK;
    std::vector<float> wu((size_t)16 * p.Cout_pad * p.Cin);
    hp::conv32_winograd_pack(packed.data(), p.Cout_pad, p.Cin, wu.data());
    HP_TRY(upload(wu, p.w_wino));
    st.bytes += (double)layers[i].cout * 9 * layers[i].cin * 4 * (16.0 / 9 - 1); // (the layer's own weights are counted already)
    return HP_OK;
}

// The layers conv32_direct_kernel covers (square 1 x 1 / 3 x 3, stride 1, whole 32- / 64-channel chunks inside the `room` channels the buffer
// has from the slice's first one) get their weights in fragment order as well: fp32 for HP_DTYPE_F32, fp16 (hi, lo) pairs for HP_DTYPE_F32S
// (every such layer); the others stay on conv32_kernel
// fp32 pipe, measured per layer of LW-OpenPose @ 8 x 46 x 54 (conv32_kernel -> direct, us alone | with a second stream): 3 x 3 128 -> 128
// 72.2 -> 58.7 | 52.6 -> 48.9; the 1 x 1 heads 512 -> 19 / 38 27.9 / 29.3 -> 26.1 / 27.4 | 18.8 / 19.6 -> 17.9 / 18.2; every wider 1 x 1
// layer within +-3 % or worse (64 -> 128 22.9 -> 29.0 paired, 512 -> 512 100 -> 100 alone): 1 x 1 layers wider than 64 padded outputs
// stay on conv32_kernel
// (a 3 x 3 layer the Winograd kernel has taken needs no direct-form fragments: they doubled its weight bytes in HBM)
int hp_engine::lower32_direct_forms(size_t, step& st, const std::vector<float>& packed, const hp::conv32_forms& f)
{
    auto& p = st.cp32();
    if (!f.w_frag)
        return HP_OK;
    const int taps = p.KH * p.KW, cout_pad = p.Cout_pad, cin_s = f.cin_split;
    const std::vector<float> wide = hp::wpack::restride32(packed, taps, cout_pad, p.Cin, cin_s);
    if (f.w_split) {
        // (a BN-folded weight beyond fp16's range has no (hi, lo) split - hi would be inf - and the run-time flag only watches
        // activations: such an engine starts on the fp32 pipe.  ADVICE r5)
        for (float v : wide)
            if (!(std::fabs(v) <= 65504.f) && !split_off)
                split_off = true, ++split_fallbacks;
        std::vector<_Float16> ws(wide.size() * 2);
        hp::conv32_split_pack(wide.data(), taps, cout_pad, cin_s, ws.data());
        HP_TRY(upload(ws, p.w_split));
    }
    // (an HP_DTYPE_F32S engine keeps the fp32 fragments too: what it runs after a value left fp16's range)
    std::vector<float> wf(wide.size());
    hp::conv32_frag_pack(wide.data(), taps, cout_pad, cin_s, wf.data());
    HP_TRY(upload(wf, p.w_frag));
    st.as<conv32_launch>().cin_split = cin_s;
    return HP_OK;
}

// conv32_head_kernel: this layer's epilogue + the hidden layer i - 1 in front of it
int hp_engine::lower32_head_in_front(size_t i, step& st, const float* w)
{
    const hp_layer &A = layers[i - 1], &L = layers[i];
    const tensor_info& tsrc = *tensors[A.in];
    const double opix = (double)geos[i].OH * geos[i].OW;
    const hp::conv32_params second = st.cp32(); // (the other forms the layer had are dropped with the conv32_launch)
    auto& hd = st.set<head32_launch>(launch_kind::head32);
    auto& p = hd.cp = second;
    const size_t nwa = (size_t)A.cout * A.cin, nw = (size_t)L.cout * L.cin;
    const float* wa = blob(A.w_off, nwa, "weights", i - 1);
    if (!wa)
        return HP_ERR_INVALID;
    HP_TRY(upload_padded(A.b_off, A.cout, A.cout, "bias", i - 1, hd.hh.bias1));
    std::vector<float> w1f(nwa);
    hp::conv32_frag_pack(wa, 1, A.cout, A.cin, w1f.data()); // ([1][HID][128] is the blob's own layout: HID rows of 128)
    const int tm2 = hp::pick32::head_tm2(L.cout);
    const std::vector<float> w2p = hp::wpack::padded(w, nw, (size_t)p.Cout_pad * L.cin); // [cout][HID] rows, zero rows up to 32 tm2
    std::vector<float> w2f((size_t)32 * tm2 * L.cin);
    hp::conv32_head_pack(w2p.data(), tm2, L.cin, w2f.data());
    HP_TRY(upload(w1f, hd.hh.w1_frag));
    HP_TRY(upload(w2f, hd.hh.w2_frag));
    hd.hh.HID = A.cout;
    hd.hh.slope1 = A.act == HP_ACT_NONE ? 1.f : A.act == HP_ACT_LEAKY ? A.act_param : 0.f;
    hd.hh.hi1 = A.act == HP_ACT_RELU6 ? 6.f : __builtin_huge_valf();
    p.in = tsrc.view32(A.in_coff);
    st.layer = (int)i - 1, st.n_layers = 2;
    st.flops = 2.0 * opix * ((double)A.cout * A.cin + (double)L.cout * L.cin);
    st.bytes = (double)tsrc.H * tsrc.W * A.cin * 4 + opix * L.cout * 4 + (double)(nwa + nw) * 4;
    return HP_OK;
}

int hp_engine::lower32_dw(size_t i, step& st)
{
    const hp_layer& L = layers[i];
    const tensor_info& ti = *tensors[L.in];
    const geo& g = geos[i];
    const double opix = (double)g.OH * g.OW;
    HP_REQUIRE(L.kh == 3 && L.kw == 3, HP_ERR_INVALID, "layer %zu: depthwise kernels are 3x3", i);
    HP_REQUIRE(L.cin % 4 == 0 && L.in_coff % 4 == 0 && L.out_coff % 4 == 0, HP_ERR_INVALID, "layer %zu: depthwise needs 4-aligned channels", i);
    // (the fp16 path refuses the same set, set_act: a PReLU here would silently run as ReLU - there are no slopes in dw32_params)
    HP_REQUIRE(L.act != HP_ACT_PRELU && L.act != HP_ACT_SIGMOID && L.act != HP_ACT_SOFTPLUS && L.res < 0, HP_ERR_INVALID,
        "layer %zu: activation %d / a residual on a depthwise layer is not supported", i, L.act);
    const float* w = blob(L.w_off, (size_t)L.cin * 9, "weights", i);
    if (!w)
        return HP_ERR_INVALID;
    auto& p = st.set<hp::dw32_params>(launch_kind::dw32);
    HP_TRY(upload(hp::wpack::dw_taps32(w, L.cin), p.w));
    HP_TRY(upload_padded(L.b_off, L.cin, L.cin, "bias", i, p.bias));
    p.in = ti.view32(L.in_coff);
    p.H = ti.H, p.W = ti.W, p.OH = g.OH, p.OW = g.OW, p.C = L.cin, p.stride = L.stride, p.dil = L.dil;
    p.pad_t = g.pt, p.pad_l = g.pl, p.act = L.act, p.act_param = L.act_param;
    hp::set_geom32(p); // (rows per thread and the division constants of the thread index)
    p.out = tensors[L.out]->view32(L.out_coff);
    st.flops = 2.0 * opix * L.cin * 9;
    st.bytes = (double)ti.H * ti.W * L.cin * 4 + opix * L.cin * 4;
    return HP_OK;
}

// ---- fp16 (and int8) engines
int hp_engine::lower16_first(size_t i, step& st)
{
    const hp_layer& L = layers[i];
    auto& p = st.set<hp::first_conv_params>(launch_kind::first16);
    const float* w = nullptr;
    HP_TRY(lower_first(i, st, p, w));
    p.w16 = nullptr;
    if (L.kh == L.kw && (L.kh == 3 || L.kh == 7) && L.cout % 8 == 0 && L.cout <= 64) // the shapes first_conv_f16_kernel has: fp16 fragments beside the fp32 weights
        HP_TRY(upload(hp::wpack::first_conv_frag16(w, L.cout, L.kh), p.w16));
    return HP_OK;
}

int hp_engine::lower16_conv(size_t i, step& st)
{
    const hp_layer& L = layers[i];
    const tensor_info& ti = *tensors[L.in];
    const geo& g = geos[i];
    const double opix = (double)g.OH * g.OW;
    const int cin_pad = round_up(L.cin, 32);
    HP_REQUIRE(L.in_coff % 8 == 0 && L.in_coff + cin_pad <= ti.cs, HP_ERR_INVALID,
        "layer %zu: channel slice [%d,+%d) not 8-aligned / exceeds the padded stride %d", i, L.in_coff, cin_pad, ti.cs);
    const int cout_pad = L.cout > 64 ? round_up(L.cout, 128) : 64;
    const int taps = L.kh * L.kw;
    const size_t nw = (size_t)L.cout * taps * L.cin;
    const float* w = blob(L.w_off, nw, "weights", i);
    if (!w)
        return HP_ERR_INVALID;
    auto& p = st.set<conv16_launch>(launch_kind::conv16).cp;
    HP_TRY(upload_padded(L.b_off, L.cout, cout_pad, "bias", i, p.bias));
    HP_TRY(upload_prelu(i, cout_pad, p.alpha));
    p.in = ti.view(L.in_coff);
    p.H = ti.H, p.W = ti.W, p.OH = g.OH, p.OW = g.OW, p.Cin = cin_pad, p.Cout = L.cout, p.Cout_pad = cout_pad;
    p.KH = L.kh, p.KW = L.kw, p.stride = L.stride, p.dil = L.dil, p.pad_t = g.pt, p.pad_l = g.pl;
    p.act = L.act, p.act_param = L.act_param;
    p.res = res_view(L.res), p.res_before_act = L.res_before_act;
    p.out = tensors[L.out]->view(L.out_coff);
    p.out_f32 = fused_output(i, true, p.out);
    p.dbg = nullptr;
    HP_REQUIRE(hp::set_act(p), HP_ERR_INVALID, "layer %zu: activation %d cannot be fused into a dense conv (use an output post-op)", i, L.act);
    // weights: the launcher says which packing its kernel for this shape reads
    p.B = max_batch, p.npix = max_batch * g.OH * g.OW;
    p.w_layout = hp::conv_weight_layout(p);
    HP_TRY(upload(hp::wpack::dense16(w, L.cout, taps, L.cin, cout_pad, cin_pad, p.w_layout), p.w));
    st.flops = 2.0 * opix * L.cout * taps * L.cin;
    st.bytes = (double)ti.H * ti.W * L.cin * 2 + opix * L.cout * 2 + (double)nw * 2;
    if (dtype == HP_DTYPE_I8 && hp::conv_i8_ok(L.kh, L.kw, L.stride, L.dil))
        HP_TRY(lower16_i8(i, st, w));
    return HP_OK;
}

// HP_DTYPE_I8: the int8 launch beside the layer's fp16 one (st.cp): q_w, its per-channel scales, dq (zeros until apply_int8_scales)
int hp_engine::lower16_i8(size_t i, step& st, const float* w)
{
    const hp_layer& L = layers[i];
    auto& c = st.as<conv16_launch>();
    const auto& p = c.cp;
    const int taps = L.kh * L.kw;
    hp::wpack::i8_rows r = hp::wpack::quantize_rows(w, L.cout, taps, L.cin, p.Cout_pad, p.Cin);
    HP_TRY(upload(r.q, c.q8.w));
    HP_TRY(upload(std::vector<float>(p.Cout_pad, 0.f), c.q8.dq));
    c.i8 = true, c.i8_dq = const_cast<float*>(c.q8.dq), c.q8.inv_a = 0.f;
    c.q8.w_direct = nullptr;
    if (hp::conv_i8_direct_ok(p)) // the same q_w in conv_i8_direct_kernel's fragment order
        HP_TRY(upload(hp::wpack::i8_direct(r.q, taps, p.Cout_pad, p.Cin), c.q8.w_direct));
    i8_sw[i] = std::move(r.s_w);
    return HP_OK;
}

int hp_engine::lower16_dw(size_t i, step& st)
{
    const hp_layer& L = layers[i];
    const tensor_info& ti = *tensors[L.in];
    const geo& g = geos[i];
    const double opix = (double)g.OH * g.OW;
    HP_REQUIRE(L.kh == 3 && L.kw == 3, HP_ERR_INVALID, "layer %zu: depthwise kernels are 3x3", i);
    HP_REQUIRE(L.cin % 8 == 0 && L.in_coff % 8 == 0 && L.out_coff % 8 == 0, HP_ERR_INVALID, "layer %zu: depthwise needs 8-aligned channels", i);
    const float* w = blob(L.w_off, (size_t)L.cin * 9, "weights", i);
    if (!w)
        return HP_ERR_INVALID;
    auto& p = st.set<hp::dw_params>(launch_kind::dw16);
    HP_TRY(upload(hp::wpack::dw_taps16(w, L.cin), p.w));
    HP_TRY(upload_padded(L.b_off, L.cin, L.cin, "bias", i, p.bias));
    p.in = ti.view(L.in_coff);
    p.H = ti.H, p.W = ti.W, p.OH = g.OH, p.OW = g.OW, p.C = L.cin, p.stride = L.stride, p.dil = L.dil;
    p.pad_t = g.pt, p.pad_l = g.pl, p.act = L.act, p.act_param = L.act_param, p.halo = ti.P;
    p.out = tensors[L.out]->view(L.out_coff);
    HP_REQUIRE(hp::dwconv3x3_ok(p), HP_ERR_INVALID, "layer %zu: no depthwise kernel for activation %d at stride %d, dilation %d", i, L.act, L.stride, L.dil);
    st.flops = 2.0 * opix * L.cin * 9;
    st.bytes = (double)ti.H * ti.W * L.cin * 2 + opix * L.cin * 2;
    return HP_OK;
}

// fp16: a two-layer head (1x1 K1 -> 512 -> 1x1 <= 64) as one mlp_head_kernel launch, layers i and i + 1
int hp_engine::lower16_head_pair(size_t i)
{
    const hp_layer &L = layers[i], &Pn = layers[i + 1];
    const tensor_info& ti = *tensors[L.in];
    const double opix = (double)geos[i].OH * geos[i].OW;
    const int K1 = L.cin, HID = L.cout;
    const float* w1f = blob(L.w_off, (size_t)HID * K1, "weights", i);
    const float* w2f = blob(Pn.w_off, (size_t)Pn.cout * HID, "weights", i + 1);
    if (!w1f || !w2f)
        return HP_ERR_INVALID;
    step st;
    st.layer = (int)i, st.op = OP_MLPHEAD, st.n_layers = 2; // (covers layers i and i + 1: the passes below must see every layer a step touches)
    auto& p = st.set<hp::head_params>(launch_kind::head);
    HP_TRY(upload(hp::wpack::dense16(w1f, HID, 1, K1, HID, K1, 1), p.w1));
    HP_TRY(upload_padded(L.b_off, HID, HID, "bias", i, p.b1));
    HP_TRY(upload(hp::wpack::head_w2(w2f, Pn.cout, HID), p.w2));
    p.in = ti.view(L.in_coff);
    p.H = ti.H, p.W = ti.W, p.K1 = K1;
    p.hi1 = L.act == HP_ACT_RELU6 ? 6.f : __builtin_huge_valf();
    HP_TRY(pointwise_params(i + 1, ti.H, ti.W, 64, p.pw)); // (pw.w stays null: the kernel reads w2)
    st.flops = 2.0 * opix * HID * K1 + 2.0 * opix * Pn.cout * HID;
    st.bytes = (double)ti.H * ti.W * K1 * 2 + opix * Pn.cout * 2 + ((double)HID * K1 + (double)Pn.cout * HID) * 2;
    steps.push_back(st);
    return HP_OK;
}

// fp16: a separable block (depthwise 3x3 + 1x1) as one sepconv launch, layers i and i + 1
int hp_engine::lower16_sep_pair(size_t i)
{
    const hp_layer &L = layers[i], &Pn = layers[i + 1];
    const tensor_info& ti = *tensors[L.in];
    const geo& g = geos[i];
    const double opix = (double)g.OH * g.OW;
    const int C = L.cin, cout_pad = round_up(Pn.cout, 128);
    const float* w = blob(L.w_off, (size_t)C * 9, "weights", i);
    const float* pwf = blob(Pn.w_off, (size_t)Pn.cout * C, "weights", i + 1);
    if (!w || !pwf)
        return HP_ERR_INVALID;
    step st;
    st.layer = (int)i, st.op = OP_SEPCONV, st.n_layers = 2;
    auto& p = st.set<hp::sep_params>(launch_kind::sep);
    HP_TRY(upload(hp::wpack::dw_taps16(w, C), p.dw_w));
    HP_TRY(upload_padded(L.b_off, C, C, "bias", i, p.dw_bias));
    HP_TRY(upload(hp::wpack::dense16(pwf, Pn.cout, 1, C, cout_pad, C, 1), p.pw.w));
    p.in = ti.view(L.in_coff);
    p.H = ti.H, p.W = ti.W, p.OH = g.OH, p.OW = g.OW, p.C = C, p.stride = L.stride, p.dil = L.dil;
    p.pad_t = g.pt, p.pad_l = g.pl, p.halo = ti.P;
    {
        hp::conv_params tmp{};
        tmp.act = L.act, tmp.act_param = L.act_param, tmp.alpha = nullptr;
        HP_REQUIRE(hp::set_act(tmp), HP_ERR_INVALID, "layer %zu: unsupported depthwise activation %d", i, L.act);
        p.dw_slope = tmp.act_slope, p.dw_hi = tmp.act_hi;
    }
    HP_TRY(pointwise_params(i + 1, g.OH, g.OW, cout_pad, p.pw));
    HP_REQUIRE(hp::sepconv_variant(p) != 0, HP_ERR_INVALID, "layer %zu: no fused separable kernel for this block (set HP_NO_FUSE=1)", i);
    st.flops = 2.0 * opix * C * 9 + 2.0 * opix * Pn.cout * C;
    st.bytes = (double)ti.H * ti.W * C * 2 + opix * Pn.cout * 2 + (double)Pn.cout * C * 2;
    steps.push_back(st);
    return HP_OK;
}

int hp_engine::plan_splitk()
{
    // ---- split-K scratch: convolutions whose tiles leave CUs idle at this engine's batch (conv_splitk) share one buffer - the
    // schedule is serial on one stream, a convolution's partial sums are consumed by its own second launch
    {
        size_t need = 0;
        for (auto& st : steps) {
            size_t bytes = 0;
            if (st.kind == launch_kind::conv16 && !switches.no_splitk && hp::conv_splitk(st.cp(), &bytes) > 1)
                need = std::max(need, bytes);
        }
        if (need) {
            weight_bufs.push_back(std::make_unique<hp::dev_buf>());
            HP_TRY(weight_bufs.back()->alloc(need));
            void* const d = weight_bufs.back()->p;
            for (auto& st : steps)
                if (st.kind == launch_kind::conv16) {
                    const int ks = hp::conv_splitk(st.cp(), nullptr);
                    if (ks > 1)
                        st.cp().ksplit = ks, st.cp().splitk = (float*)d;
                }
        }
    }
    return HP_OK;
}

int hp_engine::fuse_chains()
{
    const bool f32 = is_f32();
    const bool no_fuse = fuse_off();
    // ---- chains of 128-channel convolutions (LW-OpenPose's CPM / initial / refinement stages, lw_openpose.py:106-191): consecutive
    // steps [1x1 ->] 3x3 -> 3x3 whose intermediates nobody else reads run as ONE launch with the intermediates in LDS
    // (conv_chain.hip).  HP_NO_CHAIN=1 keeps one launch per layer (A/B measurements, and hp_engine_debug_tensor on an intermediate).
    if (!switches.no_chain && !no_fuse && !f32) {
        for (size_t k = 0; k + 1 < steps.size(); ++k) {
            if (!plain_conv(steps[k]) || !plain_conv(steps[k + 1]))
                continue;
            hp::chain_params ch{};
            int n = 0;
            const bool three = k + 2 < steps.size() && plain_conv(steps[k + 2]) && steps[k].cp().KH == 1;
            if (three) {
                const int l0 = steps[k].layer, l1 = steps[k + 1].layer, l2 = steps[k + 2].layer;
                const hp_layer &A = layers[l0], &Bn = layers[l1], &Cn = layers[l2];
                if (Bn.in == A.out && Bn.in_coff == A.out_coff && Cn.in == Bn.out && Cn.in_coff == Bn.out_coff && A.res < 0 && Bn.res < 0
                    && (Cn.res < 0 || Cn.res == A.out) && A.out_coff == 0 && private_to(A.out, l1, l2) && private_to(Bn.out, l2, l2)) {
                    ch.c0 = steps[k].cp(), ch.c1 = steps[k + 1].cp(), ch.c2 = steps[k + 2].cp();
                    ch.has_c0 = 1, ch.res_mode = Cn.res >= 0 ? 3 : 0;
                    n = 3;
                }
            }
            if (!n && steps[k].cp().KH == 3) {
                const int l1 = steps[k].layer, l2 = steps[k + 1].layer;
                const hp_layer &Bn = layers[l1], &Cn = layers[l2];
                if (Cn.in == Bn.out && Cn.in_coff == Bn.out_coff && !(Bn.res >= 0 && Cn.res >= 0) && private_to(Bn.out, l2, l2)
                    && Cn.res != Bn.out) {
                    ch.c1 = steps[k].cp(), ch.c2 = steps[k + 1].cp();
                    ch.has_c0 = 0, ch.res_mode = Bn.res >= 0 ? 1 : Cn.res >= 0 ? 2 : 0;
                    n = 2;
                }
            }
            if (!n || !hp::conv_chain_variant(ch))
                continue;
            step& a = steps[k];
            a.op = OP_CHAIN, a.set<hp::chain_params>(launch_kind::chain) = ch, a.n_layers = n;
            for (int q = 1; q < n; ++q) {
                a.flops += steps[k + q].flops;
                tensors[layers[steps[k + q].layer].in]->elided = true; // allocated (pass 1) but never written
            }
            a.bytes = steps[k].bytes + steps[k + n - 1].bytes; // first layer's input + weights ... last layer's output (approximate)
            steps.erase(steps.begin() + k + 1, steps.begin() + k + n);
        }
    }
    return HP_OK;
}

int hp_engine::fuse_bottlenecks()
{
    const bool f32 = is_f32();
    const bool no_fuse = fuse_off();
    // ---- ResNet bottlenecks (configs[3] / [4]): [3x3 ->] expansion 1x1 (+ shortcut) [-> the NEXT block's reduction 1x1] as one launch
    // (conv_bottleneck.hip).  The reduction may sit one or two steps further down the schedule (behind the next stage's projection
    // shortcut, which reads the same tensor): it has no other input, so it can run here.  HP_NO_BNECK=1 keeps one launch per layer.
    if (!switches.no_bneck && !no_fuse && !f32) {
        for (size_t k = 0; k < steps.size(); ++k) {
            if (!plain_conv(steps[k]))
                continue;
            hp::bneck_params bn{};
            size_t ke = k; // the expansion's step
            if (steps[k].cp().KH == 3 && k + 1 < steps.size() && plain_conv(steps[k + 1]) && steps[k + 1].cp().KH == 1) {
                const hp_layer &A = layers[steps[k].layer], &E = layers[steps[k + 1].layer];
                if (E.in == A.out && E.in_coff == A.out_coff && A.res < 0 && private_to(A.out, steps[k + 1].layer, steps[k + 1].layer)) {
                    bn.c3 = steps[k].cp(), bn.has_c3 = 1;
                    ke = k + 1;
                }
            }
            if (steps[ke].cp().KH != 1 || steps[ke].cp().Cout != 4 * steps[ke].cp().Cin)
                continue;
            bn.ce = steps[ke].cp();
            const hp_layer& E = layers[steps[ke].layer];
            size_t kr = 0; // the reduction's step
            for (size_t j = ke + 1; j < steps.size() && j <= ke + 2 && !kr; ++j) {
                if (!plain_conv(steps[j]) || steps[j].cp().KH != 1 || steps[j].cp().stride != 1)
                    continue;
                const hp_layer& R = layers[steps[j].layer];
                if (R.in != E.out || R.in_coff != E.out_coff || R.res >= 0)
                    continue;
                bool clash = false; // a step in between must not touch the reduction's output tensor
                for (size_t q = ke + 1; q < j; ++q) {
                    const hp_layer& Q = layers[steps[q].layer];
                    clash |= Q.in == R.out || Q.res == R.out || Q.out == R.out || steps[q].n_layers != 1;
                }
                if (!clash)
                    kr = j;
            }
            if (kr)
                bn.cr = steps[kr].cp(), bn.has_cr = 1;
            // the block's shortcut is a projection of the block input that nobody else reads (the first block of a stage at stride 1):
            // computed inside the launch instead of written by one launch and read by the next
            size_t kp = steps.size();
            if (E.res >= 0 && bn.ce.Cin == 64 && E.res_before_act) {
                const bool res_private = private_to(E.res, steps[ke].layer, steps[ke].layer);
                for (size_t j = 0; j < k && kp == steps.size(); ++j) {
                    if (!plain_conv(steps[j]) || layers[steps[j].layer].out != E.res)
                        continue;
                    const hp_layer& P = layers[steps[j].layer];
                    if (steps[j].cp().KH == 1 && steps[j].cp().stride == 1 && P.res < 0 && P.out_coff == 0 && P.act == HP_ACT_NONE && res_private)
                        kp = j;
                }
            }
            const hp::tview res_view = bn.ce.res;
            if (kp < steps.size())
                bn.cp = steps[kp].cp(), bn.has_cp = 1, bn.ce.res = NO_RES;
            // ... and the block's own reduction reads the same block input and feeds only this 3x3: computed on the 3x3's halo tile
            size_t k0 = steps.size();
            if (kp < steps.size() && bn.has_c3) {
                const hp_layer &A3 = layers[steps[k].layer], &P = layers[steps[kp].layer];
                const bool in_private = private_to(A3.in, steps[k].layer, steps[k].layer);
                for (size_t j = 0; j < k && k0 == steps.size(); ++j) {
                    if (!plain_conv(steps[j]) || layers[steps[j].layer].out != A3.in)
                        continue;
                    const hp_layer& R = layers[steps[j].layer];
                    if (steps[j].cp().KH == 1 && steps[j].cp().stride == 1 && R.res < 0 && R.out_coff == 0 && A3.in_coff == 0 && R.in == P.in && R.in_coff == P.in_coff
                        && in_private)
                        k0 = j;
                }
                if (k0 < steps.size())
                    bn.c0 = steps[k0].cp(), bn.has_c0 = 1;
            }
            // the stand-alone kernels of some of these shapes (256 -> 64 on the generic implicit GEMM) read row-major weights: the
            // fused kernel wants them in fragment order
            auto want_layout1 = [&](hp::conv_params& c) { c.w_layout = 1; };
            const int lay3 = bn.c3.w_layout, laye = bn.ce.w_layout, layr = bn.cr.w_layout, layp = bn.cp.w_layout, lay0 = bn.c0.w_layout;
            if (bn.has_c0)
                want_layout1(bn.c0);
            if (bn.has_c3)
                want_layout1(bn.c3);
            want_layout1(bn.ce);
            if (bn.has_cr)
                want_layout1(bn.cr);
            if (bn.has_cp)
                want_layout1(bn.cp);
            // the widest combination the kernel has an instance for: without the reduction (e.g. one to a width it does not serve), then
            // without the projection, then without both
            {
                const int had_cr = bn.has_cr, had_cp = bn.has_cp, had_c0 = bn.has_c0;
                bool ok = false;
                for (int drop = 0; drop < 8 && !ok; ++drop) { // bit 0: without the next reduction, bit 1: without the own reduction, bit 2: without the projection
                    if (((drop & 1) && !had_cr) || ((drop & 2) && !had_c0) || ((drop & 4) && !had_cp))
                        continue;
                    bn.has_cr = had_cr && !(drop & 1), bn.has_cp = had_cp && !(drop & 4), bn.has_c0 = had_c0 && !(drop & 2) && bn.has_cp;
                    bn.ce.res = bn.has_cp ? NO_RES : res_view;
                    ok = hp::bottleneck_variant(bn) != 0;
                }
                if (!ok)
                    continue;
                if (!bn.has_cr)
                    kr = 0;
                if (!bn.has_cp)
                    kp = steps.size();
                if (!bn.has_c0)
                    k0 = steps.size();
            }
            // repack what was uploaded row-major
            auto repack = [&](hp::conv_params& c, int had, int layer) -> int {
                if (had == 1)
                    return HP_OK;
                const hp_layer& L = layers[layer];
                const int taps = L.kh * L.kw;
                const float* w = blob(L.w_off, (size_t)L.cout * taps * L.cin, "weights", (size_t)layer);
                if (!w)
                    return HP_ERR_INVALID;
                return upload(hp::wpack::dense16(w, L.cout, taps, L.cin, c.Cout_pad, c.Cin, 1), c.w);
            };
            if (bn.has_c3)
                HP_TRY(repack(bn.c3, lay3, steps[k].layer));
            HP_TRY(repack(bn.ce, laye, steps[ke].layer));
            if (kr)
                HP_TRY(repack(bn.cr, layr, steps[kr].layer));
            if (bn.has_cp)
                HP_TRY(repack(bn.cp, layp, steps[kp].layer));
            if (bn.has_c0)
                HP_TRY(repack(bn.c0, lay0, steps[k0].layer));
            step& a = steps[k];
            const double fl = (bn.has_c3 ? steps[ke].flops : 0) + (kr ? steps[kr].flops : 0) + (bn.has_cp ? steps[kp].flops : 0) + (bn.has_c0 ? steps[k0].flops : 0);
            const double by = (bn.has_c3 ? steps[ke].bytes : 0) + (kr ? steps[kr].bytes : 0);
            a.op = OP_BNECK, a.set<hp::bneck_params>(launch_kind::bneck) = bn, a.n_layers = 1 + bn.has_c3 + bn.has_cr + bn.has_cp + bn.has_c0;
            a.flops += fl, a.bytes += by;
            if (bn.has_c3)
                tensors[layers[steps[ke].layer].in]->elided = true; // the 3x3's output: allocated (pass 1) but never written
            if (bn.has_cp)
                tensors[E.res]->elided = true; // the projection's output
            if (kr)
                steps.erase(steps.begin() + kr);
            if (bn.has_c3)
                steps.erase(steps.begin() + ke);
            if (bn.has_c0)
                tensors[layers[steps[k].layer].in]->elided = true; // the own reduction's output
            // (the projection and the own reduction sit in front of this step: erase the later one first)
            size_t front[2] = { bn.has_cp ? kp : steps.size(), bn.has_c0 ? k0 : steps.size() };
            if (front[0] < front[1])
                std::swap(front[0], front[1]);
            for (size_t q : front)
                if (q < steps.size()) {
                    steps.erase(steps.begin() + q);
                    --k;
                }
        }
    }
    return HP_OK;
}

int hp_engine::fuse_sep_pairs()
{
    const bool f32 = is_f32();
    const bool no_fuse = fuse_off();
    // ---- the MobileNet stem's separable blocks 32 -> 64 and 64 -> 128 (stride 2) as ONE launch, the 64-channel tensor between them (the
    // largest of the network) in LDS only (sepconv_pair_kernel).  HP_NO_SEPPAIR=1 keeps one launch per block.
    if (!switches.no_seppair && !no_fuse && !f32) {
        for (size_t k = 0; k + 1 < steps.size(); ++k) {
            step &a = steps[k], &b = steps[k + 1];
            if (a.kind != launch_kind::sep || b.kind != launch_kind::sep)
                continue;
            const hp_layer &Pa = layers[a.layer + 1], &Db = layers[b.layer];
            if (Db.in != Pa.out || Db.in_coff != Pa.out_coff)
                continue;
            const hp::seppair_params pp{ a.as<hp::sep_params>(), b.as<hp::sep_params>() };
            // (nobody but block b's depthwise layer reads the tensor in between, block a alone writes it, and it is no network output)
            if (!private_to(Pa.out, b.layer, b.layer) || !hp::seppair_variant(pp))
                continue;
            a.set<sep_pair_launch>(launch_kind::sep_pair) = { pp.a, pp.b }, a.n_layers += b.n_layers;
            a.flops += b.flops;
            a.bytes = a.bytes + b.bytes - 2.0 * (double)pp.a.OH * pp.a.OW * Pa.cout * 2; // the tensor in between is neither written nor read
            tensors[Pa.out]->elided = true; // allocated (pass 1) but never written
            steps.erase(steps.begin() + k + 1);
        }
    }
    return HP_OK;
}

int hp_engine::pair_heads()
{
    const bool f32 = is_f32();
    // sibling heads (conf / paf branch of one stage: same input, same geometry, neither reads the other) share a launch
    if (!switches.no_pair_heads && !f32) {
        for (size_t k = 0; k + 1 < steps.size(); ++k) {
            step &a = steps[k], &b = steps[k + 1];
            if (a.kind != launch_kind::head || b.kind != launch_kind::head)
                continue;
            const hp::head_params x = a.as<hp::head_params>(), y = b.as<hp::head_params>();
            if (x.in.p != y.in.p || x.in.coff != y.in.coff || x.K1 != y.K1 || x.H != y.H || x.W != y.W || x.pw.Cout > 64 || y.pw.Cout > 64)
                continue;
            a.set<head_pair_launch>(launch_kind::head_pair) = { x, y }, a.n_layers += b.n_layers;
            a.flops += b.flops, a.bytes += b.bytes;
            steps.erase(steps.begin() + k + 1);
        }
    }
    return HP_OK;
}

int hp_engine::finish(const hp_engine_desc* d)
{
    HP_REQUIRE(!steps.empty() && (steps[0].kind == launch_kind::first16 || steps[0].kind == launch_kind::first32), HP_ERR_INVALID, "engine: the first layer must be a CONV reading tensor 0");

    HP_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HP_HIP_TRY(hipEventCreate(&ev0));
    HP_HIP_TRY(hipEventCreate(&ev1));
    HP_HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    HP_HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    if (dtype == HP_DTYPE_I8) {
        i8_scale.assign(layers.size(), 0.f);
        for (size_t i = 0; i < layers.size(); ++i)
            if (i8_eligible((int)i))
                i8_scale[i] = -1.f;
        if (d->int8_scales) { // a calibration cache (hp_engine_describe of another engine, hp_engine_load)
            HP_TRY(check_int8_scales(d->int8_scales, d->n_layers, true));
            i8_scale.assign(d->int8_scales, d->int8_scales + d->n_layers);
            for (auto& v : i8_scale)
                v = v < 0.f ? -1.f : v;
        }
        HP_TRY(apply_int8_scales());
    }
    return HP_OK;
}


int hp_engine::check_int8_scales(const float* s, int n, bool allow_uncalibrated) const
{
    HP_REQUIRE(s, HP_ERR_INVALID, "int8 scales: null vector");
    HP_REQUIRE(n == (int)layers.size(), HP_ERR_INVALID, "int8 scales: %d values for %zu layers", n, layers.size());
    for (int i = 0; i < n; ++i) {
        HP_REQUIRE(std::isfinite(s[i]), HP_ERR_INVALID, "int8 scales: layer %d: %g is not finite", i, (double)s[i]);
        const bool uncal = allow_uncalibrated && s[i] == -1.f && i8_eligible(i);
        HP_REQUIRE(s[i] >= 0.f || uncal, HP_ERR_INVALID, "int8 scales: layer %d: negative scale %g", i, (double)s[i]);
        HP_REQUIRE(s[i] <= 0.f || i8_eligible(i), HP_ERR_INVALID,
            "int8 scales: layer %d has no int8 kernel (first layer, depthwise, pooling or an uncovered geometry): its scale must be 0", i);
    }
    return HP_OK;
}

int hp_engine::apply_int8_scales()
{
    for (auto& st : steps) {
        conv16_launch* const c = st.int8();
        if (!c)
            continue;
        const float sa = i8_scale[st.layer];
        const std::vector<float>& s_w = i8_sw[st.layer];
        std::vector<float> dq(c->cp.Cout_pad, 0.f);
        if (sa > 0.f)
            for (size_t c = 0; c < s_w.size(); ++c)
                dq[c] = sa * s_w[c]; // dq[c] = s_a * s_w[c], one fp32 product
        c->q8.inv_a = sa > 0.f ? 1.0f / sa : 0.f;
        HP_HIP_TRY(hipMemcpy(c->i8_dq, dq.data(), dq.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return HP_OK;
}

int hp_engine::ensemble_stage(const uint8_t* dev_src, int n, int scales, bool with_flip, hipStream_t s) const
{
    const size_t bytes = (size_t)n * in_h * in_w * 3;
    if (dev_src)
        HP_HIP_TRY(hipMemcpyAsync(flip_in.p, dev_src, bytes, hipMemcpyDeviceToDevice, s));
    if (scales > 1)
        HP_TRY(hp_scale::launch_stage(flip_in.as<uint8_t>(), flip_in.as<uint8_t>() + bytes, in_w, in_h, n, scale_map_w, scale_map_h, scale_ens.data(),
            scales - 1, scale_bgr, s));
    return with_flip ? hp_hflip_u8c3(flip_in.as<uint8_t>(), flip_in.as<uint8_t>() + scales * bytes, in_w, in_h, scales * n, s) : HP_OK;
}

int hp_engine::ensemble_merge(int n, int scales, bool with_flip, hipStream_t s) const
{
    for (size_t i = 0; i < outputs.size() && with_flip; ++i) {
        const out_info& o = outputs[i];
        HP_TRY(hp_flip_merge(o.buf->as<float>(), scales * n, o.out_c(), o.x.out_h, o.x.out_w, flip[i].perm.data(), flip[i].sign.data(), s));
    }
    for (size_t i = 0; i < outputs.size() && scales > 1; ++i) {
        const out_info& o = outputs[i];
        HP_TRY(hp_scale::launch_merge(o.buf->as<float>(), n, scales, o.out_c(), o.x.out_h, o.x.out_w, scale_tables.as<hp_scale::tap4>(), s));
    }
    return HP_OK;
}

namespace {
// What the graph cache waits for before it destroys an executable: every stream of the device.  An earlier call may have launched on a
// caller's stream, and the caller may have destroyed that stream since, so no remembered list of streams can be waited on.
int sync_device()
{
    HP_HIP_TRY(hipDeviceSynchronize());
    return HP_OK;
}
} // namespace

int hp_engine::drop_graphs() { return graphs.drop(sync_device); }

namespace {
// ---- bind(P, n, b0): a copy of a launch's parameters for frames [b0, b0 + n) of the batch: B (and npix, where the struct has it) for n frames,
// every activation view and out_f32 moved by b0 frames.  One overload per parameter struct, the generic one for those that are alike.
// (b0 > 0 is the second half-batch of hp_engine_set_concurrency, which the fp32 engines have: hp_engine::halves_ok.)
template <typename V> // tview / tview32
V at_frame(V v, int b0)
{
    if (v.p)
        v.p += (long)b0 * v.img * v.cs;
    return v;
}
template <typename P> // conv_params / conv32_params as a member of a fused launch: everything but npix, which those kernels do not read
P frames(P p, int n, int b0)
{
    p.B = n;
    p.in = at_frame(p.in, b0), p.out = at_frame(p.out, b0), p.res = at_frame(p.res, b0);
    if (p.out_f32)
        p.out_f32 += (size_t)b0 * p.Cout * p.OH * p.OW;
    return p;
}
template <typename P> // depthwise, max-pool, up-sampling of both precisions: one input and one output view
P bind(P p, int n, int b0)
{
    p.B = n;
    p.in = at_frame(p.in, b0), p.out = at_frame(p.out, b0);
    return p;
}
template <typename P> // the first convolutions of both precisions read the call's batch (u8 HWC or f32 NCHW, `frame` elements per image)
P bind(P p, const uint8_t* u8, const float* f32, size_t frame, int n, int b0)
{
    p.B = n;
    p.in_u8 = u8 ? u8 + b0 * frame : nullptr, p.in_f32 = f32 ? f32 + b0 * frame : nullptr;
    p.out = at_frame(p.out, b0);
    return p;
}
hp::conv_params bind(hp::conv_params p, int n, int b0)
{
    p = frames(p, n, b0), p.npix = n * p.OH * p.OW;
    return p;
}
hp::conv32_params bind(hp::conv32_params p, int n, int b0)
{
    p = frames(p, n, b0), p.npix = n * p.OH * p.OW;
    return p;
}
hp::sep_params bind(hp::sep_params p, int n, int b0)
{
    p.B = n, p.in = at_frame(p.in, b0);
    p.pw = frames(p.pw, n, b0), p.pw.npix = n * p.OH * p.OW;
    return p;
}
hp::head_params bind(hp::head_params p, int n, int b0)
{
    p.B = n, p.in = at_frame(p.in, b0);
    p.pw = frames(p.pw, n, b0);
    return p;
}
hp::chain_params bind(hp::chain_params p, int n, int b0)
{
    for (hp::conv_params* c : { &p.c0, &p.c1, &p.c2 })
        *c = frames(*c, n, b0);
    return p;
}
hp::bneck_params bind(hp::bneck_params p, int n, int b0)
{
    for (hp::conv_params* c : { &p.c3, &p.ce, &p.cr, &p.cp, &p.c0 })
        *c = frames(*c, n, b0);
    return p;
}
} // namespace

launch_payload hp_engine::bound(const step& st, const uint8_t* u8, const float* f32, int n, int b0) const
{
    const size_t frame = (size_t)in_h * in_w * 3;
    switch (st.kind) {
    case launch_kind::first16: return bind(st.as<hp::first_conv_params>(), u8, f32, frame, n, b0);
    case launch_kind::conv16: {
        conv16_launch c = st.as<conv16_launch>();
        c.cp = bind(c.cp, n, b0);
        if ((c.i8 = i8_on(st))) // (calibration zeroes the scales for a while: not a property of the schedule)
            c.q8.c = c.cp;
        return c;
    }
    case launch_kind::dw16: return bind(st.as<hp::dw_params>(), n, b0);
    case launch_kind::maxpool16:
    case launch_kind::upsample16: return bind(st.as<hp::pool_params>(), n, b0);
    case launch_kind::sep: return bind(st.as<hp::sep_params>(), n, b0);
    case launch_kind::sep_pair: return sep_pair_launch{ bind(st.as<sep_pair_launch>().a, n, b0), bind(st.as<sep_pair_launch>().b, n, b0) };
    case launch_kind::head: return bind(st.as<hp::head_params>(), n, b0);
    case launch_kind::head_pair: return head_pair_launch{ bind(st.as<head_pair_launch>().a, n, b0), bind(st.as<head_pair_launch>().b, n, b0) };
    case launch_kind::chain: return bind(st.as<hp::chain_params>(), n, b0);
    case launch_kind::bneck: return bind(st.as<hp::bneck_params>(), n, b0);
    case launch_kind::first32: return bind(st.as<hp::first_conv32_params>(), u8, f32, frame, n, b0);
    case launch_kind::conv32:
    case launch_kind::wino2:
    case launch_kind::direct: {
        conv32_launch c = st.as<conv32_launch>();
        c.cp = bind(c.cp, n, b0);
        if (st.kind == launch_kind::direct)
            c.cp.Cin = c.cin_split;
        else if (st.kind != launch_kind::conv32)
            c.cp.latency = parts > 1;
        return c;
    }
    case launch_kind::head32: return head32_launch{ bind(st.as<head32_launch>().cp, n, b0), st.as<head32_launch>().hh };
    case launch_kind::dw32: return bind(st.as<hp::dw32_params>(), n, b0);
    case launch_kind::maxpool32:
    case launch_kind::upsample32: return bind(st.as<hp::pool32_params>(), n, b0);
    }
    return {};
}

// The one place that knows which launcher a kind has.  dbg != nullptr: the HP_*_DBG relaunch, the family's debug field set on the bound copy.
int hp_engine::launch(launch_kind kind, launch_payload& b, hipStream_t s, unsigned long long* dbg) const
{
    switch (kind) {
    case launch_kind::first16: HP_HIP_TRY(hp::launch_first_conv(std::get<hp::first_conv_params>(b), s)); break;
    case launch_kind::conv16: {
        auto& c = std::get<conv16_launch>(b);
        c.cp.dbg = dbg;
        HP_HIP_TRY(c.i8 ? hp::launch_conv_i8(c.q8, s) : hp::launch_conv_mfma(c.cp, s));
        break;
    }
    case launch_kind::dw16: HP_HIP_TRY(hp::launch_dwconv3x3(std::get<hp::dw_params>(b), s)); break;
    case launch_kind::maxpool16: HP_HIP_TRY(hp::launch_maxpool(std::get<hp::pool_params>(b), s)); break;
    case launch_kind::upsample16: HP_HIP_TRY(hp::launch_upsample(std::get<hp::pool_params>(b), s)); break;
    case launch_kind::sep:
        std::get<hp::sep_params>(b).pw.dbg = dbg;
        HP_HIP_TRY(hp::launch_sepconv(std::get<hp::sep_params>(b), s));
        break;
    case launch_kind::sep_pair: HP_HIP_TRY(hp::launch_seppair(hp::seppair_params{ std::get<sep_pair_launch>(b).a, std::get<sep_pair_launch>(b).b }, s)); break;
    case launch_kind::head: HP_HIP_TRY(hp::launch_mlp_head(std::get<hp::head_params>(b), s)); break;
    case launch_kind::head_pair: HP_HIP_TRY(hp::launch_mlp_head_pair(std::get<head_pair_launch>(b).a, std::get<head_pair_launch>(b).b, s)); break;
    case launch_kind::chain:
        std::get<hp::chain_params>(b).c2.dbg = dbg;
        HP_HIP_TRY(hp::launch_conv_chain(std::get<hp::chain_params>(b), s));
        break;
    case launch_kind::bneck:
        std::get<hp::bneck_params>(b).ce.dbg = dbg;
        HP_HIP_TRY(hp::launch_bottleneck(std::get<hp::bneck_params>(b), s));
        break;
    case launch_kind::first32: HP_HIP_TRY(hp::launch_first_conv32(std::get<hp::first_conv32_params>(b), switches, s)); break;
    case launch_kind::conv32:
    case launch_kind::wino2:
    case launch_kind::direct: {
        hp::conv32_params& cp = std::get<conv32_launch>(b).cp;
        cp.dbg = dbg;
        HP_HIP_TRY(kind == launch_kind::conv32 ? hp::launch_conv32(cp, switches, s)
                : kind == launch_kind::wino2   ? hp::launch_conv32_winograd(cp, switches, s)
                                               : hp::launch_conv32_direct(cp, on_split_pipe(), s));
        break;
    }
    case launch_kind::head32: HP_HIP_TRY(hp::launch_conv32_head(std::get<head32_launch>(b).cp, std::get<head32_launch>(b).hh, s)); break;
    case launch_kind::dw32: HP_HIP_TRY(hp::launch_dwconv32(std::get<hp::dw32_params>(b), switches, s)); break;
    case launch_kind::maxpool32: HP_HIP_TRY(hp::launch_maxpool32(std::get<hp::pool32_params>(b), s)); break;
    case launch_kind::upsample32: HP_HIP_TRY(hp::launch_upsample32(std::get<hp::pool32_params>(b), s)); break;
    }
    return HP_OK;
}

// hp_layer_time::tile of a bound launch: exactly the struct its launcher gets
int hp_engine::tile_of(launch_kind kind, const launch_payload& b) const
{
    switch (kind) {
    case launch_kind::conv16: {
        const auto& c = std::get<conv16_launch>(b);
        return c.i8 ? hp::conv_i8_tile(c.cp) : hp::conv_mfma_tile(c.cp);
    }
    case launch_kind::sep: return 4000000 + hp::sepconv_variant(std::get<hp::sep_params>(b));
    case launch_kind::sep_pair: return 4000000 + 20;
    case launch_kind::head: return 6000000 + std::get<hp::head_params>(b).K1;
    case launch_kind::head_pair: return 6000000 + std::get<head_pair_launch>(b).a.K1;
    case launch_kind::chain: return 7000000 + hp::conv_chain_variant(std::get<hp::chain_params>(b));
    case launch_kind::bneck: return 9000000 + hp::bottleneck_variant(std::get<hp::bneck_params>(b));
    case launch_kind::conv32: return hp::pick_conv32(std::get<conv32_launch>(b).cp, switches, hp::C32_GEMM, false).tile;
    case launch_kind::wino2: return hp::pick_conv32(std::get<conv32_launch>(b).cp, switches, hp::C32_WINO2, false).tile;
    case launch_kind::direct: return hp::pick_conv32(std::get<conv32_launch>(b).cp, switches, hp::C32_DIRECT, on_split_pipe()).tile;
    case launch_kind::head32: return hp::pick32::head_tile(std::get<head32_launch>(b).hh.HID, std::get<head32_launch>(b).cp.Cout);
    default: return 0; // first convolutions, depthwise, pooling, up-sampling: one form each
    }
}

int hp_engine::step_tile(const step& st, int n) const { return tile_of(st.kind, bound(st, nullptr, nullptr, n, 0)); }

// HP_CONV_DBG / HP_BN_DBG / HP_CHAIN_DBG / HP_SEP_DBG / HP_DIRECT_DBG: which block timeline, if any, the switches ask for on this step, and
// the numbers its text quotes (engine_timeline.hpp).  Kinds without a case have no timeline.
bool hp_engine::timeline_of(const step& st, const launch_payload& b, hp::timeline_kind& kind, hp::timeline_header& hd) const
{
    hd = hp::timeline_header{};
    hd.layer = st.layer;
    switch (st.kind) {
    case launch_kind::conv16: { // the pixel-block GEMM
        const auto& c = std::get<conv16_launch>(b);
        if (c.i8 || !switches.dbg_conv || hp::conv_mfma_tile(c.cp) / 100000 != 52)
            return false;
        kind = hp::timeline_kind::conv, hd.cin = c.cp.Cin, hd.cout = c.cp.Cout, hd.tile = hp::conv_mfma_tile(c.cp);
        return true;
    }
    case launch_kind::bneck:
        kind = hp::timeline_kind::bneck, hd.tile = hp::bottleneck_variant(std::get<hp::bneck_params>(b));
        return switches.dbg_bn;
    case launch_kind::chain:
        kind = hp::timeline_kind::chain, hd.tile = hp::conv_chain_variant(std::get<hp::chain_params>(b));
        return switches.dbg_chain;
    case launch_kind::sep:
        kind = hp::timeline_kind::sep, hd.cin = std::get<hp::sep_params>(b).C;
        return switches.dbg_sep;
    case launch_kind::conv32:
    case launch_kind::wino2:
    case launch_kind::direct: {
        const hp::conv32_params& q = std::get<conv32_launch>(b).cp;
        if (!switches.dbg_direct || (st.kind == launch_kind::conv32 && q.Cin < switches.dbg_min_cin))
            return false;
        kind = st.kind == launch_kind::conv32 ? hp::timeline_kind::conv32
            : st.kind == launch_kind::wino2   ? hp::timeline_kind::wino
                                              : hp::timeline_kind::direct;
        hd.cin = q.Cin, hd.cout = q.Cout, hd.kh = q.KH, hd.kw = q.KW, hd.tile = tile_of(st.kind, b);
        if (st.kind == launch_kind::wino2)
            (void)hp::conv32_winograd_occupancy(q, &hd.blocks_per_cu);
        return true;
    }
    default: return false;
    }
}

// ... the step's kernel launched once more with its block-timeline stamps (s_memtime = shader cycles; the 100 MHz clock) written into a zeroed
// scratch buffer, printed to stderr per launch
int hp_engine::trace_step(const step& st, launch_payload& b, hipStream_t s) const
{
    hp::timeline_kind kind;
    hp::timeline_header hd;
    if (!timeline_of(st, b, kind, hd))
        return HP_OK;
    const size_t words = hp::timeline_words(kind);
    hp::dev_buf buf;
    HP_TRY(buf.alloc(words * 8));
    HP_HIP_TRY(hipMemset(buf.p, 0, words * 8));
    HP_TRY(launch(st.kind, b, s, buf.as<unsigned long long>()));
    HP_HIP_TRY(hipStreamSynchronize(s));
    std::vector<unsigned long long> hv(words);
    HP_HIP_TRY(hipMemcpy(hv.data(), buf.p, words * 8, hipMemcpyDeviceToHost));
    hp::print_timeline(stderr, kind, hd, hv.data());
    return HP_OK;
}

int hp_engine::run_step(const step& st, const uint8_t* u8, const float* f32, int n, hipStream_t s, int b0) const
{
    launch_payload b = bound(st, u8, f32, n, b0);
    HP_TRY(launch(st.kind, b, s, nullptr));
    return trace_step(st, b, s);
}

// two fused fp32 heads in a row that read the same tensor (LW-OpenPose's heat-map and PAF heads of a stage): one grid (conv32_head.hip), where
// the kernel takes the pair at this batch.  Not a build pass: the schedule and the profile rows keep the two heads apart.
int hp_engine::launch_head_pair32(size_t i, int n, int b0, hipStream_t s, bool* done) const
{
    *done = false;
    if (i + 1 >= steps.size() || steps[i].kind != launch_kind::head32 || steps[i + 1].kind != launch_kind::head32)
        return HP_OK;
    const auto &ha = steps[i].as<head32_launch>(), &hb = steps[i + 1].as<head32_launch>();
    const hp::conv32_params a = bind(ha.cp, n, b0), b = bind(hb.cp, n, b0);
    if (!hp::pick32::head_pair_ok(a, b, switches))
        return HP_OK;
    HP_HIP_TRY(hp::launch_conv32_head_pair(a, ha.hh, b, hb.hh, s));
    *done = true;
    return HP_OK;
}

int hp_engine::enqueue_range(const uint8_t* u8, const float* f32, int b0, int n, hipStream_t s) const
{
    for (size_t i = 0; i < steps.size(); ++i) {
        bool paired = false;
        HP_TRY(launch_head_pair32(i, n, b0, s, &paired));
        if (paired)
            ++i;
        else
            HP_TRY(run_step(steps[i], u8, f32, n, s, b0));
    }
    for (auto& o : outputs)
        if (o.fused_layer < 0) {
            const tensor_info& ti = *tensors[o.tensor];
            float* const dst = o.buf->as<float>() + (size_t)b0 * o.out_c() * o.x.out_h * o.x.out_w;
            if (is_f32())
                HP_HIP_TRY(hp::launch_output_transform32(at_frame(ti.view32(o.coff), b0), n, o.H, o.W, o.x, dst, s));
            else
                HP_HIP_TRY(hp::launch_output_transform(ti.view(o.coff), n, o.H, o.W, o.x, dst, s));
        }
    return HP_OK;
}

void hp_engine::fill_row(hp_layer_time* out, int k, int cap, const step& st, int n, float ms) const
{
    if (!out || k >= cap)
        return;
    out[k].layer = st.layer, out[k].op = st.op;
    out[k].tile = step_tile(st, n);
    out[k].ms = ms;
    out[k].flops = st.flops * n, out[k].bytes = st.bytes * n;
}

// One call as csrc/call_plan.hpp plans it (refusals are the caller's); eager and captured calls differ only in how a range is run (`run`)
int hp_engine::run_call(const hp::call_settings& cfg, const hp::call_args& a)
{
    if (hp::reads_in_stage(cfg, a))
        HP_TRY(ensure_in_stage());
    const hp::call_plan p = hp::plan_call(cfg, { in_stage.p, flip_in.p }, a);
    const hipStream_t s = a.stream ? (hipStream_t)a.stream : stream;
    const size_t frame_bytes = (size_t)in_h * in_w * 3 * (p.kind == 1 ? sizeof(float) : 1);
    auto stream_of = [&](int i) { return p.ranges[i].second ? stream2 : s; };
    auto upload = [&](int b0, int cnt, hipStream_t st) -> int { // host frames [b0, b0 + cnt) to the buffer the network reads
        HP_HIP_TRY(hipMemcpyAsync((unsigned char*)p.read + b0 * frame_bytes, (const unsigned char*)p.host_src + b0 * frame_bytes, cnt * frame_bytes, hipMemcpyHostToDevice, st));
        return HP_OK;
    };
    auto range = [&](int i) -> int {
        return enqueue_range(p.kind == 0 ? (const uint8_t*)p.read : nullptr, p.kind == 1 ? (const float*)p.read : nullptr, p.ranges[i].b0, p.ranges[i].cnt, stream_of(i));
    };
    auto bracketed = [&](auto&& inner) -> int { // the ensembles' stage and merge around `inner`, on the call's stream (a.n: the caller's frames)
        if (p.staged)
            HP_TRY(ensemble_stage((const uint8_t*)p.fl_src, a.n, p.scales, p.ensemble, s));
        HP_TRY(inner());
        return p.staged ? ensemble_merge(a.n, p.scales, p.ensemble, s) : HP_OK;
    };
    // capture a range's schedule once per key; replays cost one launch.  A call names ALL its ranges at once: the cache decides about eviction
    // before the first capture, so no executable of this call can be destroyed before it is launched (csrc/graph_cache.hpp), and a call whose
    // keys are cached costs its look-ups.
    hipGraphExec_t exec[2] = { nullptr, nullptr };
    auto capture = [&](int i, hipGraphExec_t* made) -> int {
        hipGraph_t graph = nullptr;
        HP_HIP_TRY(hipStreamBeginCapture(stream_of(i), hipStreamCaptureModeThreadLocal));
        const int rc = p.stage_inside ? bracketed([&] { return range(i); }) : range(i);
        const hipError_t ee = hipStreamEndCapture(stream_of(i), &graph);
        if (rc != HP_OK) {
            if (graph)
                (void)hipGraphDestroy(graph);
            return rc;
        }
        HP_HIP_TRY(ee);
        const hipError_t ie = hipGraphInstantiate(made, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        HP_HIP_TRY(ie);
        return HP_OK;
    };
    if (p.captured)
        HP_TRY(graphs.acquire(p.keys, p.nr, exec, capture, sync_device));
    if (p.host_src && p.staged)
        HP_TRY(upload(0, a.n, s));
    // Two half-batches side by side: frames [0, n0) on `s`, [n0, n) on stream2, which joins `s` again.  The kernels of one half are half as many
    // blocks - what fills the chip is that the halves are never in the same phase (a store-bound launch of one runs under an MFMA-bound launch of
    // the other): 2490 -> 1962 us per synchronous batch of 8 (profiles/r06_half_batch_probe.txt).  Frames are independent and every kernel is
    // batch-invariant bit for bit (tests).  Captured: two graphs on two streams - ONE graph with two branches is replayed branch after branch.
    auto run = [&]() -> int {
        if (p.nr == 2) {
            HP_HIP_TRY(hipEventRecord(ev_fork, s));
            HP_HIP_TRY(hipStreamWaitEvent(stream2, ev_fork, 0));
        }
        for (int i = 0; i < p.nr && p.host_src && !p.staged; ++i) // (the second half's frames cross PCIe under the first half's first layers)
            HP_TRY(upload(p.ranges[i].b0, p.ranges[i].cnt, stream_of(i)));
        for (int i = 0; i < p.nr; ++i)
            if (p.captured)
                HP_HIP_TRY(hipGraphLaunch(exec[i], stream_of(i)));
            else
                HP_TRY(range(i));
        if (p.nr == 2) {
            HP_HIP_TRY(hipEventRecord(ev_join, stream2));
            HP_HIP_TRY(hipStreamWaitEvent(s, ev_join, 0));
        }
        return HP_OK;
    };
    return p.captured && p.stage_inside ? run() : bracketed(run); // (one captured range holds flip and merge itself)
}

hp::engine_switches hp::read_engine_switches()
{
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    auto num = [](const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; };
    engine_switches w;
    w.no_fuse = on("HP_NO_FUSE"), w.no_fuse_head = num("HP_NO_FUSE_HEAD", 0) != 0, w.no_splitk = on("HP_NO_SPLITK");
    w.no_chain = on("HP_NO_CHAIN"), w.no_bneck = on("HP_NO_BNECK"), w.no_seppair = on("HP_NO_SEPPAIR"), w.no_pair_heads = on("HP_NO_PAIR_HEADS");
    w.fuse32 = on("HP_FUSE32"), w.no_fuse32 = on("HP_NO_FUSE32"), w.no_head32 = on("HP_NO_HEAD32"), w.no_arena = on("HP_NO_ARENA");
    w.no_winograd32 = on("HP_NO_WINOGRAD32"), w.wino_tall = num("HP_WINO_TALL", 1) != 0;
    w.wino_nc = num("HP_WINO_NC", 0), w.head_pair32 = num("HP_HEAD_PAIR", 1) != 0;
    w.c32_wk = num("HP_C32_WK", -1), w.c32_bn160 = num("HP_C32_BN160", -1), w.dw32_px = num("HP_DW32_PX", 0);
    w.lane_epilogue = num("HP_LANE_EPILOGUE", 0), w.first_conv_verify = on("HP_FIRST_CONV_VERIFY");
    w.dbg_conv = on("HP_CONV_DBG"), w.dbg_bn = on("HP_BN_DBG"), w.dbg_chain = on("HP_CHAIN_DBG"), w.dbg_sep = on("HP_SEP_DBG");
    w.dbg_direct = on("HP_DIRECT_DBG"), w.dbg_min_cin = num("HP_DIRECT_DBG_MINCIN", 256);
    return w;
}

extern "C" {

int hp_engine_create(hp_engine** out, const hp_engine_desc* desc)
{
    HP_REQUIRE(out && desc, HP_ERR_INVALID, "hp_engine_create: null argument");
    std::unique_ptr<hp_engine> e(new hp_engine());
    e->switches = hp::read_engine_switches();
    try { // descriptions come from files (hp_engine_load, ONNX import): absurd sizes must come back as error codes
        HP_TRY(e->build(desc));
    } catch (const std::exception& ex) {
        HP_REQUIRE(false, HP_ERR_INVALID, "hp_engine_create: %s", ex.what());
    }
    *out = e.release();
    return HP_OK;
}

// ---- serialized engines (reference: tensorrt::save, src/tensorrt.cpp:463-471; tensorrt_serialized + the deserialising
// constructor, include/hyperpose/utility/model.hpp:27-32, src/tensorrt.cpp:225-252).  The file holds what hp_engine_create
// was given - topology, outputs, pre-processing, fp32 weights - so loading rebuilds the identical engine without the model
// source; the packing into kernel layouts happens at load (tens of ms), there is no per-device tuning cache to carry.
namespace {
constexpr char ENGINE_MAGIC[8] = { 'H', 'P', 'E', 'N', 'G', '0', '0', '3' }; // 002: + dtype; 003: + the int8 scale vector
struct engine_file_header {
    char magic[8];
    int32_t layer_size, output_size; // sizeof(hp_layer) / sizeof(hp_output_desc): ABI guard
    int32_t in_w, in_h, max_batch, flip_rb;
    double factor;
    float mean[3], inv_std[3];
    int32_t n_layers, n_outputs;
    uint64_t n_weights;
    int32_t dtype;    // HP_DTYPE_*: TensorRT bakes the builder's precision into the plan it serializes, so does this file
    int32_t n_scales; // 003: n_layers (HP_DTYPE_I8: the per-layer int8 scales follow the weights, -1 = not calibrated) or 0 (002: reserved, 0)
};
} // namespace

int hp_engine_save(const hp_engine* e, const char* path)
{
    HP_REQUIRE(e && path, HP_ERR_INVALID, "hp_engine_save: null argument");
    FILE* f = fopen(path, "wb");
    HP_REQUIRE(f, HP_ERR_INVALID, "hp_engine_save: cannot open %s for writing", path);
    engine_file_header h{};
    memcpy(h.magic, ENGINE_MAGIC, 8);
    h.layer_size = (int32_t)sizeof(hp_layer), h.output_size = (int32_t)sizeof(hp_output_desc);
    h.in_w = e->in_w, h.in_h = e->in_h, h.max_batch = e->max_batch, h.flip_rb = e->flip_rb, h.factor = e->factor;
    for (int c = 0; c < 3; ++c)
        h.mean[c] = e->mean[c], h.inv_std[c] = e->inv_std[c];
    h.n_layers = (int32_t)e->layers.size(), h.n_outputs = (int32_t)e->out_descs.size(), h.n_weights = e->weights_blob.size();
    h.dtype = e->dtype;
    h.n_scales = (int32_t)e->i8_scale.size();
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1;
    ok = ok && fwrite(e->layers.data(), sizeof(hp_layer), e->layers.size(), f) == e->layers.size();
    ok = ok && fwrite(e->out_descs.data(), sizeof(hp_output_desc), e->out_descs.size(), f) == e->out_descs.size();
    ok = ok && fwrite(e->weights_blob.data(), sizeof(float), e->weights_blob.size(), f) == e->weights_blob.size();
    ok = ok && fwrite(e->i8_scale.data(), sizeof(float), e->i8_scale.size(), f) == e->i8_scale.size();
    ok = (fclose(f) == 0) && ok;
    HP_REQUIRE(ok, HP_ERR_INVALID, "hp_engine_save: short write to %s", path);
    return HP_OK;
}

int hp_engine_load(hp_engine** out, const char* path, int max_batch)
{
    HP_REQUIRE(out && path, HP_ERR_INVALID, "hp_engine_load: null argument");
    FILE* f = fopen(path, "rb");
    HP_REQUIRE(f, HP_ERR_INVALID, "hp_engine_load: cannot open %s", path);
    engine_file_header h{};
    std::vector<hp_layer> layers;
    std::vector<hp_output_desc> outs;
    std::vector<float> w, scales;
    // an HPENG001 file (before data_type was honoured) is an 002 file without the trailing (dtype, reserved) pair, and its engine was fp16;
    // an 002 file is an 003 file without scales (its `reserved` word was written as 0)
    constexpr size_t HDR_001 = offsetof(engine_file_header, dtype);
    bool ok = fread(&h, HDR_001, 1, f) == 1;
    if (ok && memcmp(h.magic, "HPENG001", 8) == 0)
        memcpy(h.magic, ENGINE_MAGIC, 8), h.dtype = HP_DTYPE_F16, h.n_scales = 0;
    else {
        ok = ok && fread(reinterpret_cast<char*>(&h) + HDR_001, sizeof(h) - HDR_001, 1, f) == 1;
        if (ok && memcmp(h.magic, "HPENG002", 8) == 0)
            memcpy(h.magic, ENGINE_MAGIC, 8), ok = h.n_scales == 0 && h.dtype != HP_DTYPE_I8;
    }
    ok = ok && memcmp(h.magic, ENGINE_MAGIC, 8) == 0 && h.layer_size == (int32_t)sizeof(hp_layer)
        && h.output_size == (int32_t)sizeof(hp_output_desc) && h.n_layers > 0 && h.n_layers < (1 << 20) && h.n_outputs > 0
        && h.n_outputs < 4096 && h.n_weights < ((uint64_t)1 << 34)
        && (h.dtype == HP_DTYPE_F16 || h.dtype == HP_DTYPE_F32 || h.dtype == HP_DTYPE_F32S || h.dtype == HP_DTYPE_I8)
        && h.n_scales == (h.dtype == HP_DTYPE_I8 ? h.n_layers : 0);
    if (ok) { // the counts must account for the file exactly before anything is allocated from them
        const long at = ftell(f);
        ok = fseek(f, 0, SEEK_END) == 0;
        const long size = ftell(f);
        ok = ok && fseek(f, at, SEEK_SET) == 0
            && (uint64_t)size == (uint64_t)at + (uint64_t)h.n_layers * sizeof(hp_layer) + (uint64_t)h.n_outputs * sizeof(hp_output_desc) + h.n_weights * sizeof(float)
                    + (uint64_t)h.n_scales * sizeof(float);
    }
    if (ok) {
        layers.resize(h.n_layers), outs.resize(h.n_outputs), w.resize(h.n_weights), scales.resize(h.n_scales);
        ok = fread(layers.data(), sizeof(hp_layer), layers.size(), f) == layers.size()
            && fread(outs.data(), sizeof(hp_output_desc), outs.size(), f) == outs.size() && fread(w.data(), sizeof(float), w.size(), f) == w.size()
            && fread(scales.data(), sizeof(float), scales.size(), f) == scales.size();
    }
    fclose(f);
    HP_REQUIRE(ok, HP_ERR_INVALID, "hp_engine_load: %s is not an engine file written by this library version", path);
    hp_engine_desc d{};
    d.in_w = h.in_w, d.in_h = h.in_h, d.max_batch = max_batch > 0 ? max_batch : h.max_batch, d.factor = h.factor, d.flip_rb = h.flip_rb;
    for (int c = 0; c < 3; ++c)
        d.mean[c] = h.mean[c], d.inv_std[c] = h.inv_std[c];
    d.layers = layers.data(), d.n_layers = h.n_layers, d.outputs = outs.data(), d.n_outputs = h.n_outputs, d.weights = w.data(), d.n_weights = w.size();
    d.dtype = h.dtype;
    d.int8_scales = scales.empty() ? nullptr : scales.data();
    return hp_engine_create(out, &d);
}

void hp_engine_destroy(hp_engine* e)
{
    if (!e)
        return;
    (void)hipDeviceSynchronize(); // (not the engine's stream alone: a captured graph may still be running on a caller's stream)
    delete e;
}

int hp_engine_max_batch(const hp_engine* e) { return e ? e->max_batch : HP_ERR_INVALID; }

int hp_engine_describe(const hp_engine* e, hp_engine_desc* d)
{
    HP_REQUIRE(e && d, HP_ERR_INVALID, "hp_engine_describe: null argument");
    d->in_w = e->in_w, d->in_h = e->in_h, d->max_batch = e->max_batch, d->factor = e->factor, d->flip_rb = e->flip_rb;
    for (int c = 0; c < 3; ++c)
        d->mean[c] = e->mean[c], d->inv_std[c] = e->inv_std[c];
    d->layers = e->layers.data(), d->n_layers = (int32_t)e->layers.size();
    d->outputs = e->out_descs.data(), d->n_outputs = (int32_t)e->out_descs.size();
    d->weights = e->weights_blob.data(), d->n_weights = e->weights_blob.size();
    d->dtype = e->dtype;
    d->int8_scales = e->dtype == HP_DTYPE_I8 ? e->i8_scale.data() : nullptr;
    return HP_OK;
}

int hp_engine_dtype(const hp_engine* e) { return e ? e->dtype : HP_ERR_INVALID; }

int hp_engine_input_size(const hp_engine* e, int* w, int* h)
{
    HP_REQUIRE(e && w && h, HP_ERR_INVALID, "hp_engine_input_size: null argument");
    *w = e->in_w, *h = e->in_h;
    return HP_OK;
}

int hp_engine::leave_split()
{
    HP_TRY(drop_graphs());
    split_off = true, ++split_fallbacks;
    *static_cast<volatile unsigned*>(ovf_flag.p) = 0;
    return HP_OK;
}

static int infer_common(hp_engine* e, const hp::call_args& a)
{
    HP_REQUIRE(e && a.input, HP_ERR_INVALID, "hp_engine_infer: null argument");
    if (e->split_overflowed()) // an earlier batch held a value outside fp16's range: from here on the fp32 matrix pipe
        HP_TRY(e->leave_split());
    e->last = a;
    const hp::call_settings cfg = e->call_settings(e->flip_on(), e->use_graph, e->scale_k());
    const hp::call_refusal why = hp::refusal_of(cfg, a);
    HP_REQUIRE(why != hp::CALL_EMPTY, HP_ERR_INVALID, "hp_engine_infer: empty batch");
    // TensorRT builds no kINT8 engine without a calibrator or per-tensor dynamic ranges; here the engine exists and refuses to run
    for (float v : e->i8_scale)
        HP_REQUIRE(v >= 0.f, HP_ERR_STATE,
            "hp_engine_infer: the HP_DTYPE_I8 engine is not calibrated: call hp_engine_calibrate_u8 (calibrate()) or hp_engine_set_int8_scales first");
    // src/tensorrt.cpp:439-443 throws std::logic_error here
    HP_REQUIRE(why != hp::CALL_OVERFLOW, HP_ERR_CAPACITY, "Input batch size overflow: Yours@%d Max@%d", a.n, e->max_batch);
    if (cfg.scales > 1) { // (the flip ensemble's messages below keep their wording while the scale ensemble is off)
        HP_REQUIRE(why != hp::CALL_F32_ENSEMBLE, HP_ERR_STATE, "hp_engine_infer_f32: not available while the scale ensemble%s is on (it is defined on u8 frames: hp_engine_infer_u8)",
            cfg.ensemble ? " (and the flip ensemble)" : "");
        HP_REQUIRE(why != hp::CALL_ENSEMBLE_OVERFLOW, HP_ERR_CAPACITY, "Input batch size overflow: Yours@%d, with the scale ensemble on (K = %d)%s %d network images, Max@%d",
            a.n, cfg.scales, cfg.ensemble ? " and the flip ensemble on" : "", hp::images_of(cfg, a.n), e->max_batch);
    }
    HP_REQUIRE(why != hp::CALL_F32_ENSEMBLE, HP_ERR_STATE, "hp_engine_infer_f32: not available while the flip ensemble is on (it is defined on u8 frames: hp_engine_infer_u8)");
    HP_REQUIRE(why != hp::CALL_ENSEMBLE_OVERFLOW, HP_ERR_CAPACITY, "Input batch size overflow: Yours@%d, with the flip ensemble on %d network images, Max@%d", a.n,
        2 * a.n, e->max_batch);
    return e->run_call(cfg, a);
}

int hp_engine_infer_u8(hp_engine* e, const uint8_t* hwc_bgr, int n, int on_device, void* stream)
{
    HP_REQUIRE(e, HP_ERR_INVALID, "hp_engine_infer_u8: null engine");
    return infer_common(e, { hwc_bgr, n, on_device, 0, stream });
}

int hp_engine_infer_f32(hp_engine* e, const float* nchw, int n, int on_device, void* stream)
{
    HP_REQUIRE(e, HP_ERR_INVALID, "hp_engine_infer_f32: null engine");
    return infer_common(e, { nchw, n, on_device, 1, stream });
}

int hp_engine_synchronize(hp_engine* e)
{
    HP_REQUIRE(e, HP_ERR_INVALID, "null engine");
    HP_HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->last.stream && (hipStream_t)e->last.stream != e->stream) // the newest call ran on the caller's stream: the flag below is its kernels'
        HP_HIP_TRY(hipStreamSynchronize((hipStream_t)e->last.stream));
    if (e->split_overflowed() && e->last.input) {
        // HP_DTYPE_F32S: the batch just finished saw |x| > 65504 somewhere - its outputs are not trustworthy.  Run it again on the fp32
        // pipe before the caller reads them (a host input is copied again from the caller's buffer, which the API keeps valid until the
        // outputs are read)
        HP_TRY(e->leave_split());
        HP_TRY(infer_common(e, e->last));
        HP_HIP_TRY(hipStreamSynchronize(e->last.stream ? (hipStream_t)e->last.stream : e->stream));
    }
    return HP_OK;
}

int hp_engine_split_fallbacks(const hp_engine* e) { return e ? e->split_fallbacks : HP_ERR_INVALID; }

int hp_engine_int8_scales(const hp_engine* e, float* scales, int n)
{
    HP_REQUIRE(e && scales, HP_ERR_INVALID, "hp_engine_int8_scales: null argument");
    HP_REQUIRE(e->dtype == HP_DTYPE_I8, HP_ERR_STATE, "hp_engine_int8_scales: not an HP_DTYPE_I8 engine");
    HP_REQUIRE(n == (int)e->i8_scale.size(), HP_ERR_INVALID, "hp_engine_int8_scales: room for %d values, the engine has %zu layers", n, e->i8_scale.size());
    std::copy(e->i8_scale.begin(), e->i8_scale.end(), scales);
    return HP_OK;
}

int hp_engine_set_int8_scales(hp_engine* e, const float* scales, int n)
{
    HP_REQUIRE(e && scales, HP_ERR_INVALID, "hp_engine_set_int8_scales: null argument");
    HP_REQUIRE(e->dtype == HP_DTYPE_I8, HP_ERR_STATE, "hp_engine_set_int8_scales: not an HP_DTYPE_I8 engine");
    HP_TRY(e->check_int8_scales(scales, n, false));
    HP_TRY(e->drop_graphs()); // a captured graph holds the old kernels and arguments
    e->i8_scale.assign(scales, scales + n);
    return e->apply_int8_scales();
}

int hp_engine_calibrate_u8(hp_engine* e, const uint8_t* hwc_bgr, int n, int on_device)
{
    HP_REQUIRE(e && hwc_bgr, HP_ERR_INVALID, "hp_engine_calibrate_u8: null argument");
    HP_REQUIRE(e->dtype == HP_DTYPE_I8, HP_ERR_STATE, "hp_engine_calibrate_u8: not an HP_DTYPE_I8 engine");
    HP_REQUIRE(n >= 1, HP_ERR_INVALID, "hp_engine_calibrate_u8: no frames");
    HP_TRY(e->drop_graphs());
    const int NL = (int)e->layers.size();
    // every layer in fp16 (scale 0) while the frames run: x is what the fp16 per-layer schedule computes.  A failure leaves the old scales.
    std::vector<float> scales(NL, 0.f);
    struct restore {
        hp_engine* e;
        std::vector<float> old;
        ~restore()
        {
            if (e)
                e->i8_scale = old;
        }
    } guard{ e, e->i8_scale };
    e->i8_scale.assign(NL, 0.f);
    hp::dev_buf amax;
    HP_TRY(amax.alloc((size_t)NL * sizeof(unsigned)));
    HP_HIP_TRY(hipMemsetAsync(amax.p, 0, (size_t)NL * sizeof(unsigned), e->stream));
    const hp::call_settings eager = e->call_settings(false, false); // (calibration ignores the ensemble setting)
    for (int b0 = 0; b0 < n; b0 += e->max_batch) {
        const int cnt = std::min(e->max_batch, n - b0);
        HP_TRY(e->run_call(eager, { hwc_bgr + (size_t)b0 * e->in_h * e->in_w * 3, cnt, on_device, 0, e->stream }));
        for (const auto& st : e->steps) {
            if (!st.int8())
                continue;
            const hp_layer& L = e->layers[st.layer];
            const auto& ti = *e->tensors[L.in];
            HP_HIP_TRY(hp::launch_absmax(ti.view(L.in_coff), cnt, ti.H, ti.W, L.cin, amax.as<unsigned>() + st.layer, e->stream));
        }
        // the next chunk's copy overwrites the staged frames only after this chunk's kernels read them (same stream)
    }
    std::vector<unsigned> bits(NL);
    HP_HIP_TRY(hipStreamSynchronize(e->stream));
    HP_HIP_TRY(hipMemcpy(bits.data(), amax.p, (size_t)NL * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int i = 0; i < NL; ++i)
        if (e->i8_eligible(i)) {
            float a;
            memcpy(&a, &bits[i], sizeof(float));
            // (an fp16 activation that overflowed would give s_a = inf: inv_a = 0, dq = inf, NaN outputs)
            HP_REQUIRE(std::isfinite(a), HP_ERR_INVALID, "hp_engine_calibrate_u8: layer %d: the input of this layer is not finite on the calibration frames (max |x| = %g)", i, (double)a);
            scales[i] = a > 0.f ? a / 127.f : 1.f; // TensorRT's MinMax calibrator: s_a = A / 127
        }
    guard.e = nullptr;
    e->i8_scale = scales;
    return e->apply_int8_scales();
}

int hp_engine_device_bytes(const hp_engine* e, uint64_t bytes[3])
{
    HP_REQUIRE(e && bytes, HP_ERR_INVALID, "hp_engine_device_bytes: null argument");
    bytes[0] = bytes[1] = bytes[2] = 0;
    for (const auto& t : e->tensors)
        if (t)
            bytes[0] += t->buf.bytes;
    for (const auto& a : e->arena)
        bytes[0] += a.mem->bytes;
    for (const auto& w : e->weight_bufs)
        bytes[1] += w->bytes;
    for (const auto& o : e->outputs)
        if (o.buf)
            bytes[2] += o.buf->bytes;
    return HP_OK;
}

int hp_debug_first_conv_verify(unsigned out[4], int reset)
{
    HP_REQUIRE(out, HP_ERR_INVALID, "hp_debug_first_conv_verify: null argument");
    hp::first_conv32_verify_counts(out, reset != 0);
    return HP_OK;
}

int hp_engine_arena_info(const hp_engine* e, uint64_t info[3])
{
    HP_REQUIRE(e && info, HP_ERR_INVALID, "hp_engine_arena_info: null argument");
    info[0] = e->arena.size(), info[1] = 0, info[2] = e->arena_private_bytes;
    for (const auto& a : e->arena)
        info[1] += a.tenants;
    return HP_OK;
}

void* hp_engine_stream(hp_engine* e) { return e ? (void*)e->stream : nullptr; }

int hp_engine_set_concurrency(hp_engine* e, int parts)
{
    HP_REQUIRE(e && (parts == 1 || parts == 2), HP_ERR_INVALID, "hp_engine_set_concurrency: parts must be 1 or 2");
    // HP_DTYPE_F32 / F32S only: the fp16 engine's fused launches take no frame offset.  (A split engine failed this in round 6 until the cause was
    // found in first_conv32_kernel's packed FMAs: DESIGN.md section 7B.8, hyperpose_amd/build.py.)
    if (!e->halves_ok())
        parts = 1;
    if (parts == e->parts)
        return HP_OK;
    HP_TRY(e->drop_graphs()); // (the captured schedules are of the other form)
    if (parts == 2 && !e->stream2)
        HP_HIP_TRY(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
    e->parts = parts;
    return HP_OK;
}

int hp_engine_concurrency(const hp_engine* e) { return e ? e->parts : HP_ERR_INVALID; }

int hp_engine_cached_graphs(const hp_engine* e) { return e ? (int)e->graphs.size() : HP_ERR_INVALID; }

int hp_engine_set_graph(hp_engine* e, int enable)
{
    HP_REQUIRE(e, HP_ERR_INVALID, "null engine");
    e->use_graph = enable != 0;
    return HP_OK;
}

int hp_engine_set_flip_ensemble(hp_engine* e, const hp_flip_output* outs, int n_outs)
{
    HP_REQUIRE(e && n_outs >= 0 && (outs || n_outs == 0), HP_ERR_INVALID, "hp_engine_set_flip_ensemble: null argument");
    const int NO = (int)e->outputs.size();
    std::vector<hp_engine::flip_table> next(n_outs ? NO : 0);
    if (n_outs) {
        HP_REQUIRE(n_outs == NO, HP_ERR_INVALID, "hp_engine_set_flip_ensemble: %d outputs listed, the engine has %d: every output is listed exactly once", n_outs, NO);
        for (int k = 0; k < n_outs; ++k) {
            const int i = outs[k].output;
            HP_REQUIRE(i >= 0 && i < NO, HP_ERR_INVALID, "hp_engine_set_flip_ensemble: entry %d names output %d, the engine has outputs 0 .. %d", k, i, NO - 1);
            HP_REQUIRE(next[i].perm.empty(), HP_ERR_INVALID, "hp_engine_set_flip_ensemble: output %d (%s) is listed twice", i, e->outputs[i].name.c_str());
            HP_REQUIRE(outs[k].perm && outs[k].sign, HP_ERR_INVALID, "hp_engine_set_flip_ensemble: entry %d (output %d) has a null table", k, i);
            const int Cn = e->outputs[i].out_c();
            HP_REQUIRE(Cn >= 1 && Cn <= 256, HP_ERR_INVALID, "hp_engine_set_flip_ensemble: output %d (%s) has %d channels, hp_flip_merge takes 1 .. 256", i,
                e->outputs[i].name.c_str(), Cn);
            for (int c = 0; c < Cn; ++c) {
                HP_REQUIRE(outs[k].perm[c] >= 0 && outs[k].perm[c] < Cn, HP_ERR_INVALID, "hp_engine_set_flip_ensemble: output %d: perm[%d] = %d is outside [0, %d)", i, c,
                    outs[k].perm[c], Cn);
                HP_REQUIRE(outs[k].sign[c] == 1 || outs[k].sign[c] == -1, HP_ERR_INVALID, "hp_engine_set_flip_ensemble: output %d: sign[%d] = %d is neither -1 nor +1", i, c,
                    (int)outs[k].sign[c]);
            }
            next[i].perm.assign(outs[k].perm, outs[k].perm + Cn), next[i].sign.assign(outs[k].sign, outs[k].sign + Cn);
        }
    }
    HP_TRY(e->drop_graphs()); // (the captured schedules are of the other form)
    const size_t need = (size_t)e->max_batch * e->in_h * e->in_w * 3;
    if (n_outs && e->flip_in.bytes < need)
        HP_TRY(e->flip_in.alloc(need));
    e->flip.swap(next);
    return HP_OK;
}

int hp_engine_set_flip_ensemble_coco(hp_engine* e, int enable)
{
    HP_REQUIRE(e, HP_ERR_INVALID, "hp_engine_set_flip_ensemble_coco: null engine");
    if (!enable)
        return hp_engine_set_flip_ensemble(e, nullptr, 0);
    const int NO = (int)e->outputs.size();
    HP_REQUIRE(NO == 2, HP_ERR_INVALID, "hp_engine_set_flip_ensemble_coco: a COCO PAF network has two outputs (conf, paf), this engine has %d", NO);
    const out_info &c = e->outputs[0], &p = e->outputs[1];
    HP_REQUIRE((c.out_c() == HP_COCO_N_PARTS || c.out_c() == HP_COCO_N_PARTS + 1) && p.out_c() == 2 * HP_COCO_N_PAIRS, HP_ERR_INVALID,
        "hp_engine_set_flip_ensemble_coco: outputs %s with %d and %s with %d channels, expected 18 or 19 and 38", c.name.c_str(), c.out_c(), p.name.c_str(), p.out_c());
    HP_REQUIRE(c.x.out_h == p.x.out_h && c.x.out_w == p.x.out_w, HP_ERR_INVALID, "hp_engine_set_flip_ensemble_coco: outputs %s %d x %d and %s %d x %d differ in size",
        c.name.c_str(), c.x.out_h, c.x.out_w, p.name.c_str(), p.x.out_h, p.x.out_w);
    int32_t conf_perm[HP_COCO_N_PARTS + 1], paf_perm[2 * HP_COCO_N_PAIRS];
    int8_t conf_sign[HP_COCO_N_PARTS + 1], paf_sign[2 * HP_COCO_N_PAIRS];
    HP_TRY(hp_flip_tables_coco(c.out_c(), conf_perm, paf_perm, paf_sign));
    std::fill(conf_sign, conf_sign + HP_COCO_N_PARTS + 1, (int8_t)1);
    const hp_flip_output outs[2] = { { 0, conf_perm, conf_sign }, { 1, paf_perm, paf_sign } };
    return hp_engine_set_flip_ensemble(e, outs, 2);
}

int hp_engine_flip_ensemble(const hp_engine* e) { return e ? (int)e->flip_on() : HP_ERR_INVALID; }

int hp_engine_set_scale_ensemble(hp_engine* e, const float* scales, int n_scales, int b, int g, int r)
{
    const char* who = "hp_engine_set_scale_ensemble";
    HP_REQUIRE(e, HP_ERR_INVALID, "%s: null engine", who);
    if (n_scales == 0) {
        HP_TRY(e->drop_graphs()); // (the captured schedules are of the other form)
        e->scale_ens.clear(), e->scale_tables.release();
        return HP_OK;
    }
    HP_TRY(hp_scale::check_scales(who, scales, n_scales));
    HP_REQUIRE(b >= 0 && b <= 255 && g >= 0 && g <= 255 && r >= 0 && r <= 255, HP_ERR_INVALID, "%s: fill (%d, %d, %d) is outside 0 .. 255", who, b, g, r);
    const int NO = (int)e->outputs.size();
    HP_REQUIRE(NO >= 1, HP_ERR_INVALID, "%s: the engine has no outputs", who);
    const int H = e->outputs[0].x.out_h, W = e->outputs[0].x.out_w;
    for (int i = 0; i < NO; ++i) {
        const out_info& o = e->outputs[i];
        HP_REQUIRE(o.x.out_h == H && o.x.out_w == W, HP_ERR_INVALID, "%s: outputs %s %d x %d and %s %d x %d differ in size: the scale ensemble needs one map grid", who,
            e->outputs[0].name.c_str(), W, H, o.name.c_str(), o.x.out_w, o.x.out_h);
        HP_REQUIRE(o.out_c() >= 1 && o.out_c() <= hp_scale::MAX_C, HP_ERR_INVALID, "%s: output %d (%s) has %d channels, the scale merge takes 1 .. %d", who, i,
            o.name.c_str(), o.out_c(), hp_scale::MAX_C);
    }
    HP_REQUIRE(e->in_w % W == 0 && e->in_h % H == 0, HP_ERR_INVALID, "%s: the input %d x %d is not a whole number of map cells of the outputs' %d x %d", who, e->in_w,
        e->in_h, W, H);
    std::vector<hp_scale::tap4> tables(hp_scale::tables_entries(n_scales, H, W));
    HP_TRY(hp_scale::fill_tables(tables.data(), scales, n_scales, H, W));
    HP_TRY(e->drop_graphs()); // (the captured schedules are of the other form; and nothing in flight reads the old tables from here on)
    const size_t need = (size_t)e->max_batch * e->in_h * e->in_w * 3;
    if (e->flip_in.bytes < need)
        HP_TRY(e->flip_in.alloc(need));
    HP_TRY(e->scale_tables.alloc(tables.size() * sizeof(hp_scale::tap4)));
    HP_HIP_TRY(hipMemcpy(e->scale_tables.p, tables.data(), tables.size() * sizeof(hp_scale::tap4), hipMemcpyHostToDevice));
    e->scale_ens.assign(scales, scales + n_scales);
    e->scale_bgr[0] = b, e->scale_bgr[1] = g, e->scale_bgr[2] = r, e->scale_map_w = W, e->scale_map_h = H;
    return HP_OK;
}

int hp_engine_set_scale_ensemble_coco(hp_engine* e, const float* scales, int n_scales)
{
    HP_REQUIRE(e, HP_ERR_INVALID, "hp_engine_set_scale_ensemble_coco: null engine");
    if (n_scales == 0)
        return hp_engine_set_scale_ensemble(e, nullptr, 0, 0, 0, 0);
    const int NO = (int)e->outputs.size();
    HP_REQUIRE(NO == 2, HP_ERR_INVALID, "hp_engine_set_scale_ensemble_coco: a COCO PAF network has two outputs (conf, paf), this engine has %d", NO);
    const out_info &c = e->outputs[0], &p = e->outputs[1];
    HP_REQUIRE((c.out_c() == HP_COCO_N_PARTS || c.out_c() == HP_COCO_N_PARTS + 1) && p.out_c() == 2 * HP_COCO_N_PAIRS, HP_ERR_INVALID,
        "hp_engine_set_scale_ensemble_coco: outputs %s with %d and %s with %d channels, expected 18 or 19 and 38", c.name.c_str(), c.out_c(), p.name.c_str(), p.out_c());
    HP_REQUIRE(c.x.out_h == p.x.out_h && c.x.out_w == p.x.out_w, HP_ERR_INVALID, "hp_engine_set_scale_ensemble_coco: outputs %s %d x %d and %s %d x %d differ in size",
        c.name.c_str(), c.x.out_h, c.x.out_w, p.name.c_str(), p.x.out_h, p.x.out_w);
    return hp_engine_set_scale_ensemble(e, scales, n_scales, 0, 0, 0);
}

int hp_engine_scale_ensemble(const hp_engine* e) { return e ? e->scale_k() : HP_ERR_INVALID; }

int hp_engine_num_outputs(const hp_engine* e) { return e ? (int)e->outputs.size() : HP_ERR_INVALID; }

int hp_engine_output(const hp_engine* e, int i, const char** name, int shape[3], const float** dev)
{
    HP_REQUIRE(e && i >= 0 && i < (int)e->outputs.size(), HP_ERR_INVALID, "hp_engine_output: index %d", i);
    const out_info& o = e->outputs[i];
    if (name)
        *name = o.name.c_str();
    if (shape)
        shape[0] = o.out_c(), shape[1] = o.x.out_h, shape[2] = o.x.out_w;
    if (dev)
        *dev = o.buf->as<float>();
    return HP_OK;
}

int hp_engine_output_to_host(hp_engine* e, int i, int n, float* host)
{
    HP_REQUIRE(e && host && i >= 0 && i < (int)e->outputs.size() && n >= 1 && n <= e->max_batch, HP_ERR_INVALID, "hp_engine_output_to_host: bad argument");
    const out_info& o = e->outputs[i];
    HP_TRY(hp_engine_synchronize(e)); // (an HP_DTYPE_F32S engine re-runs the batch here if a value left fp16's range)
    HP_HIP_TRY(hipMemcpy(host, o.buf->p, (size_t)n * o.out_c() * o.x.out_h * o.x.out_w * sizeof(float), hipMemcpyDeviceToHost));
    return HP_OK;
}

int hp_engine_debug_tensor(hp_engine* e, int tensor, int n, float* host, int shape[3])
{
    HP_REQUIRE(e && tensor > 0 && tensor < (int)e->tensors.size() && e->tensors[tensor]->defined, HP_ERR_INVALID, "hp_engine_debug_tensor: bad tensor %d", tensor);
    HP_REQUIRE(!e->tensors[tensor]->unwritten, HP_ERR_STATE, "hp_engine_debug_tensor: tensor %d exists only as the fp32 network output", tensor);
    HP_REQUIRE(!e->tensors[tensor]->elided, HP_ERR_STATE, "hp_engine_debug_tensor: tensor %d lives only inside a fused separable block (HP_NO_FUSE=1 materialises it)", tensor);
    HP_REQUIRE(e->tensors[tensor]->arena_slot < 0 || e->arena[e->tensors[tensor]->arena_slot].tenants == 1, HP_ERR_STATE,
        "hp_engine_debug_tensor: tensor %d shares its buffer with later tensors of the same geometry (the activation arena); build the engine with HP_NO_ARENA=1 to look at it", tensor);
    const tensor_info& ti = *e->tensors[tensor];
    if (shape)
        shape[0] = ti.C, shape[1] = ti.H, shape[2] = ti.W;
    if (!host)
        return HP_OK;
    HP_REQUIRE(n >= 1 && n <= e->max_batch, HP_ERR_INVALID, "hp_engine_debug_tensor: bad batch");
    hp::dev_buf tmp;
    HP_TRY(tmp.alloc((size_t)n * ti.C * ti.H * ti.W * sizeof(float)));
    hp::out_xform px{};
    px.C = ti.C, px.act = 0, px.shuffle = 1, px.group = 0, px.out_h = ti.H, px.out_w = ti.W, px.scale = 1.f, px.grid = 0;
    if (e->is_f32())
        HP_HIP_TRY(hp::launch_output_transform32(ti.view32(0), n, ti.H, ti.W, px, tmp.as<float>(), e->stream));
    else
        HP_HIP_TRY(hp::launch_output_transform(ti.view(0), n, ti.H, ti.W, px, tmp.as<float>(), e->stream));
    HP_HIP_TRY(hipStreamSynchronize(e->stream));
    HP_HIP_TRY(hipMemcpy(host, tmp.p, tmp.bytes, hipMemcpyDeviceToHost));
    return HP_OK;
}

int hp_engine_debug_raw_tensor(hp_engine* e, int tensor, void* host, size_t cap_bytes, int geom[8])
{
    HP_REQUIRE(e && geom && tensor > 0 && tensor < (int)e->tensors.size() && e->tensors[tensor] && e->tensors[tensor]->defined, HP_ERR_INVALID,
        "hp_engine_debug_raw_tensor: bad tensor %d", tensor);
    const tensor_info& ti = *e->tensors[tensor];
    HP_REQUIRE(!ti.unwritten, HP_ERR_STATE, "hp_engine_debug_raw_tensor: tensor %d exists only as the fp32 network output", tensor);
    HP_REQUIRE(!ti.elided, HP_ERR_STATE, "hp_engine_debug_raw_tensor: tensor %d lives only inside a fused launch (HP_NO_FUSE=1 materialises it)", tensor);
    // (a tensor of the activation arena is NOT refused: what lies in the shared buffer outside the interior is every tenant's padding)
    const bool f32 = e->is_f32();
    const int rows = f32 ? ti.rows32() : ti.H + 2 * ti.P;
    const int esz = f32 ? (int)sizeof(float) : (int)sizeof(__half);
    geom[0] = ti.H, geom[1] = ti.W, geom[2] = ti.C, geom[3] = ti.cs, geom[4] = ti.P, geom[5] = rows, geom[6] = esz, geom[7] = e->max_batch;
    if (!host)
        return HP_OK;
    const size_t bytes = (size_t)e->max_batch * rows * (ti.W + 2 * ti.P) * ti.cs * esz;
    HP_REQUIRE(ti.base<void>() && cap_bytes >= bytes, HP_ERR_INVALID, "hp_engine_debug_raw_tensor: tensor %d takes %zu bytes, the host buffer has %zu", tensor, bytes, cap_bytes);
    HP_TRY(hp_engine_synchronize(e));
    HP_HIP_TRY(hipMemcpy(host, ti.base<void>(), bytes, hipMemcpyDeviceToHost));
    return HP_OK;
}

int hp_engine_profile(hp_engine* e, int n, int iters, hp_layer_time* out, int cap, int* n_out)
{
    HP_REQUIRE(e && n >= 1 && n <= e->max_batch && iters >= 1 && n_out, HP_ERR_INVALID, "hp_engine_profile: bad argument");
    HP_TRY(e->ensure_in_stage());
    const uint8_t* u8 = e->in_stage.as<uint8_t>();
    int k = 0;
    for (const step& st : e->steps) {
        HP_TRY(e->run_step(st, u8, nullptr, n, e->stream)); // warm
        HP_HIP_TRY(hipEventRecord(e->ev0, e->stream));
        for (int it = 0; it < iters; ++it)
            HP_TRY(e->run_step(st, u8, nullptr, n, e->stream));
        HP_HIP_TRY(hipEventRecord(e->ev1, e->stream));
        HP_HIP_TRY(hipEventSynchronize(e->ev1));
        float ms = 0;
        HP_HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        e->fill_row(out, k++, cap, st, n, ms / iters);
    }
    *n_out = k;
    return HP_OK;
}

// Machine time per launch: step k of two engines of the same model launched alternately on their two streams, so that two instances of
// the kernel share the GPU the way two pipes' kernels do; reported = elapsed / (2 * iters).  (A kernel that fills the chip gains nothing
// from the second stream; one that leaves CUs, slots or pipes idle does - the end-to-end rate with several pipes follows this figure.)
int hp_engine_profile_pair(hp_engine* e, hp_engine* f, int n, int iters, hp_layer_time* out, int cap, int* n_out)
{
    HP_REQUIRE(e && f && e != f && n >= 1 && n <= e->max_batch && n <= f->max_batch && iters >= 1 && n_out && e->steps.size() == f->steps.size(),
        HP_ERR_INVALID, "hp_engine_profile_pair: bad argument");
    for (size_t i = 0; i < e->steps.size(); ++i) // the same schedule: step by step the same operation on the same amount of work
        HP_REQUIRE(e->steps[i].op == f->steps[i].op && e->steps[i].layer == f->steps[i].layer && e->steps[i].flops == f->steps[i].flops
                && e->steps[i].bytes == f->steps[i].bytes,
            HP_ERR_INVALID, "hp_engine_profile_pair: the engines' schedules differ at step %zu", i);
    HP_TRY(e->ensure_in_stage());
    HP_TRY(f->ensure_in_stage());
    int k = 0;
    for (size_t i = 0; i < e->steps.size(); ++i) {
        const step &sa = e->steps[i], &sb = f->steps[i];
        HP_TRY(e->run_step(sa, e->in_stage.as<uint8_t>(), nullptr, n, e->stream));
        HP_TRY(f->run_step(sb, f->in_stage.as<uint8_t>(), nullptr, n, f->stream));
        HP_HIP_TRY(hipStreamSynchronize(e->stream));
        HP_HIP_TRY(hipStreamSynchronize(f->stream));
        HP_HIP_TRY(hipEventRecord(e->ev0, e->stream));
        HP_HIP_TRY(hipEventRecord(f->ev0, f->stream));
        for (int it = 0; it < iters; ++it) {
            HP_TRY(e->run_step(sa, e->in_stage.as<uint8_t>(), nullptr, n, e->stream));
            HP_TRY(f->run_step(sb, f->in_stage.as<uint8_t>(), nullptr, n, f->stream));
        }
        HP_HIP_TRY(hipEventRecord(e->ev1, e->stream));
        HP_HIP_TRY(hipEventRecord(f->ev1, f->stream));
        HP_HIP_TRY(hipEventSynchronize(e->ev1));
        HP_HIP_TRY(hipEventSynchronize(f->ev1));
        float m0 = 0, m1 = 0;
        HP_HIP_TRY(hipEventElapsedTime(&m0, e->ev0, e->ev1));
        HP_HIP_TRY(hipEventElapsedTime(&m1, f->ev0, f->ev1));
        e->fill_row(out, k++, cap, sa, n, std::max(m0, m1) / (2 * iters));
    }
    *n_out = k;
    return HP_OK;
}

int hp_engine_profile_sequence(hp_engine* e, int n, int iters, hp_layer_time* out, int cap, int* n_out)
{
    HP_REQUIRE(e && n >= 1 && n <= e->max_batch && iters >= 1 && n_out, HP_ERR_INVALID, "hp_engine_profile_sequence: bad argument");
    HP_TRY(e->ensure_in_stage());
    const uint8_t* u8 = e->in_stage.as<uint8_t>();
    const size_t ns = e->steps.size();
    // one (start, stop) event pair per step; the launch itself records them (hipExtLaunchKernelGGL), so they bracket the
    // kernel's own execution and no packet is inserted between consecutive kernels
    std::vector<hipEvent_t> ev0(ns, nullptr), ev1(ns, nullptr);
    std::vector<double> acc(ns, 0.0);
    int rc = HP_OK;
    for (size_t k = 0; k < ns; ++k)
        if (hipEventCreate(&ev0[k]) != hipSuccess || hipEventCreate(&ev1[k]) != hipSuccess)
            rc = HP_ERR_HIP;
    for (int it = -1; it < iters && rc == HP_OK; ++it) { // it == -1: warm-up pass
        for (size_t k = 0; k < ns && rc == HP_OK; ++k) {
            hp::prof_start = ev0[k], hp::prof_stop = ev1[k];
            rc = e->run_step(e->steps[k], u8, nullptr, n, e->stream);
            hp::prof_start = hp::prof_stop = nullptr;
        }
        if (rc == HP_OK && hipStreamSynchronize(e->stream) != hipSuccess)
            rc = HP_ERR_HIP;
        for (size_t k = 0; k < ns && rc == HP_OK && it >= 0; ++k) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev0[k], ev1[k]) != hipSuccess)
                rc = HP_ERR_HIP;
            acc[k] += ms;
        }
    }
    hp::prof_start = hp::prof_stop = nullptr;
    for (size_t k = 0; k < ns; ++k) {
        if (ev0[k])
            (void)hipEventDestroy(ev0[k]);
        if (ev1[k])
            (void)hipEventDestroy(ev1[k]);
    }
    HP_REQUIRE(rc == HP_OK, rc, "hp_engine_profile_sequence: launch or event failure");
    int k = 0;
    for (const step& st : e->steps) {
        e->fill_row(out, k, cap, st, n, (float)(acc[k] / iters));
        ++k;
    }
    *n_out = k;
    return HP_OK;
}

} // extern "C"
