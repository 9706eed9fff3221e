// pipeline.cpp — hyperpose::stream on the GPU (reference include/hyperpose/stream/stream.hpp:119-390, src/stream.cpp):
// the reference pushes every frame through four CPU threads and three mutex-guarded queues (resize -> inference ->
// parse -> writer) with a host round trip between each; here a batch of host frames is copied once to the device and
// stays there: H2D copy, cv::resize / non_scaling_resize (resize.hip), the conv stack (engine.cpp) and the PAF parser
// (paf_parser.hip) are enqueued back to back on ONE HIP stream of one of `n_pipes` engine+parser pairs, and only the
// humans come back.  Several batches are in flight (one per pipe); results are returned in submission order, like the
// reference's queues.  resume_ratio is applied on the way out when the aspect ratio was kept.
//
// One road from a submitted frame to its network slot.  Frames arrive as 8-bit BGR (hp_pipeline_submit), as YUV 4:2:0 buffers (hp_pipeline_submit_yuv)
// as hp_yuv_image descriptions of any layout, in host or in device memory (hp_pipeline_submit_yuv_images), or as hp_rgb_image descriptions of the packed
// RGB / BGRA-family / grey layouts, again in host or in device memory (hp_pipeline_submit_rgb_images); every submit is
//     admit()            n frames of R slots each fit a batch and a pipe is free (R = 1, or the regions of a frame in tiled mode)
//     check and plan     EVERY frame is checked, and plan_frame() has its upright size and its R regions, before the first copy is enqueued:
//                        a refused batch leaves nothing in the stream
//     upload             upload_blob() (a contiguous host blob -> p.raw at 256-byte offsets, through p.stage unless pinned) or upload_yuv_images()
//                        (planes packed tightly) or upload_rgb_images() (rows packed tightly, in the frame's own layout); all copies first, then all kernels: the stream changes between the copy engine and the
//                        compute queue once per batch, not once per frame
//     one resize call    per frame, and always the general one: hp_resize_oriented_u8c3 / hp_resize_oriented_yuv / hp_resize_rgb, in tiled mode
//                        hp_resize_rois_oriented_u8c3 / hp_resize_rois_oriented_yuv / hp_resize_rois_rgb, with the pipeline's orientation, the frame's tone-map (or null)
//                        and keep_ratio.  Which kernel runs is decided inside those four calls (resize_oriented.hip) and nowhere here: orientation 0
//                        forwards to the un-oriented call, a null tone-map is the SDR call
//     infer_and_parse()  conv stack, parser, and the pipe joins the ring
// The settings only feed that road.  Tiled mode (hp_pipeline_set_tiling): a frame becomes its R regions in R consecutive slots, and hp_pipeline_collect
// maps every region's humans back to the frame and merges them (tiles.cpp).  HDR input (hp_pipeline_set_tonemap): the P010 / I010 frames of
// hp_pipeline_submit_yuv_images get the tone-map, 8-bit frames of the same batch get null.  Upright input (hp_pipeline_set_orientation): the submitted
// frames are STORED frames, and everything behind the resize - letterbox, tiles, resume_ratio, the merge - sees the upright uw x uh frame of plan_frame().
// Flip ensemble (hp_pipeline_set_flip_ensemble): every pipe's engine runs each network-sized slot and its left-right flip and merges the maps
// (flip_ensemble.hip) before the parser reads them; here only the capacity changes: a batch holds pl->capacity() = max_batch / 2 slots.  Scale
// ensemble (hp_pipeline_set_scale_ensemble): the same with K - 1 shrunken copies of every slot (scale_ensemble.hip), max_batch / (K (flip ? 2 : 1)).
// Three things leave the road on purpose:
//     (a) an untiled, un-oriented BGR frame of the network's size needs no kernel: it is copied straight into its slot of p.net, and a run of such
//         frames that is contiguous in pinned host memory goes in ONE copy (the benchmark's path)
//     (b) hp_pipeline_submit_yuv keeps the 4:2:0 kernel of its own (hp_resize_yuv420 / hp_letterbox_yuv420, resize_yuv.hip) and is refused in tiled and
//         in oriented mode
//     (c) all copies first, then all kernels, within a batch - also where (a) mixes direct and resized frames
#include "hp_common.hpp"
#include "parser_host.hpp"
#include "rgb_formats.hpp"
#include "scale_ensemble.hpp"
#include "yuv_formats.hpp"

#include <cstring>
#include <memory>
#include <vector>

namespace {

struct pipe_t {
    hp_engine* eng = nullptr;
    std::unique_ptr<hp::parser_session> parser; // the hyperpose::parser the pipeline ends in (make_parser)
    hipStream_t s = nullptr;
    hp::host_buf stage;     // pinned staging for frames that arrive in pageable memory
    hp::dev_buf raw, net;   // frames as submitted; frames at network size [max_batch][in_h][in_w][3]
    int n = 0;              // frames in flight (0 = free)
    std::vector<int> w, h;
    int regions = 0;        // tiled batch: regions per frame (0 = an untiled batch), p.n / regions frames
    std::vector<hp_roi> roi; // tiled batch: the region of every slot
};

// pinned memory (hp_malloc_host / hipHostMalloc) is copied straight from where it lies; anything else through staging
bool is_pinned(const void* ptr)
{
    hipPointerAttribute_t attr;
    const bool pinned = hipPointerGetAttributes(&attr, ptr) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned)
        (void)hipGetLastError();
    return pinned;
}

} // namespace

struct hp_pipeline {
    int n_pipes = 0, max_batch = 0, in_w = 0, in_h = 0, keep_ratio = 0, kind = HP_PARSER_PAF;
    size_t max_frame_bytes = 0;
    std::vector<pipe_t> pipes;
    int head = 0, tail = 0, inflight = 0; // ring over the pipes
    bool tiled = false;
    hp_tiling tiling{};
    std::vector<hp_human> slot_humans, cand, kept; // tiled collect: the parser's per-slot lists, one frame's candidates, its merged humans
    std::vector<int> slot_n;
    std::vector<int32_t> cand_region;
    int orientation = HP_ORIENT_NONE; // non-zero: submitted frames are stored turned / mirrored, p.w / p.h and the regions are the upright frame's
    hp_tonemap* tonemap = nullptr; // set: 10-bit hp_yuv_image frames are PQ / HLG and are tone-mapped while they are resized
    bool flip_ensemble = false;    // set: every engine runs slot + flipped slot, so a batch holds half as many slots
    std::vector<float> scale_ens;  // set: every engine runs slot + its K - 1 shrunken copies, so a batch holds 1 / K as many slots
    int passes() const { return (int)(1 + scale_ens.size()) * (flip_ensemble ? 2 : 1); } // network images per slot
    int capacity() const { return max_batch / passes(); } // network-sized slots per submit
    std::string note;              // what flip_note() says under the scale ensemble (set_note)
    const char* flip_note() const { return !scale_ens.empty() ? note.c_str() : flip_ensemble ? " / 2: the flip ensemble is on, every frame runs with its flip" : ""; }
    void set_note()
    {
        char b[160];
        std::snprintf(b, sizeof b, " / %d: the scale ensemble (K = %d)%s is on, every frame runs %d times", passes(), (int)(1 + scale_ens.size()),
            flip_ensemble ? " and the flip ensemble" : "", passes());
        note = b;
    }

    // the tone-map of a frame, or null for the SDR path
    const hp_tonemap* tonemap_for(const hp_yuv_image& f) const { return tonemap && hp_yuv::layout_of(f.format)->sample_bytes == 2 ? tonemap : nullptr; }

    ~hp_pipeline()
    {
        for (auto& p : pipes) {
            if (p.s)
                (void)hipStreamSynchronize(p.s);
            p.parser.reset();
            if (p.eng)
                hp_engine_destroy(p.eng);
        }
        hp_tonemap_destroy(tonemap);
    }
};

namespace {

int infer_and_parse(hp_pipeline* pl, pipe_t& p, int n);
int collect_tiled(hp_pipeline* pl, pipe_t& p, hp_human* out, int cap_per_frame, int* n_out, int* n_frames);
int upload_yuv_images(pipe_t& p, const hp_yuv_image* frames, int n, std::vector<hp_yuv_image>& dev);
int upload_rgb_images(pipe_t& p, const hp_rgb_image* frames, int n, std::vector<hp_rgb_image>& dev);

// network-sized slots a frame takes: its regions in tiled mode, one otherwise
int tiled_regions(const hp_pipeline* pl) { return pl->tiled ? pl->tiling.cols * pl->tiling.rows + pl->tiling.with_full : 1; }

// what every submit checks first: n frames of R slots each fit a batch, and a pipe is free
int admit(const hp_pipeline* pl, const char* who, int n)
{
    const int R = tiled_regions(pl);
    if (pl->tiled)
        HP_REQUIRE(n >= 1 && n <= pl->capacity() / R, HP_ERR_CAPACITY, "%s: %d frames of %d regions each > max_batch %d%s (at most %d frames per submit)", who, n,
            R, pl->max_batch, pl->flip_note(), pl->capacity() / R);
    else
        HP_REQUIRE(n >= 1 && n <= pl->capacity(), HP_ERR_CAPACITY, "%s: batch %d > max_batch %d%s", who, n, pl->max_batch, pl->flip_note());
    HP_REQUIRE(pl->inflight < pl->n_pipes, HP_ERR_STATE, "%s: all %d pipes are busy, collect first", who, pl->n_pipes);
    return HP_OK;
}

// Frame i of a batch as everything behind its resize sees it: the upright size in p.w / p.h and, in tiled mode, its R regions in p.roi, planned on
// the upright frame.  (ax, ay) is the stored layout's region alignment; behind a quarter turn the upright x axis is the stored y axis.
int plan_frame(const hp_pipeline* pl, pipe_t& p, int i, int sw, int sh, int ax, int ay)
{
    HP_TRY(hp_oriented_size(pl->orientation, sw, sh, &p.w[i], &p.h[i]));
    if (!pl->tiled)
        return HP_OK;
    if (pl->orientation & 1)
        std::swap(ax, ay);
    const int R = tiled_regions(pl), rc = hp_tile_plan(&pl->tiling, p.w[i], p.h[i], ax, ay, &p.roi[(size_t)i * R], R);
    return rc < 0 ? rc : HP_OK;
}

// One contiguous host blob -> the device, enqueued on p.s: from where it lies when it is pinned, through p.stage otherwise; to `dst`, or (null) to
// p.raw.  `off` is the batch's running offset into p.stage and p.raw, a multiple of 256: it moves on when either slot is in use until the copy has run.
int upload_blob(pipe_t& p, const uint8_t* src, size_t bytes, bool pinned, uint8_t* dst, size_t& off)
{
    if (!pinned) {
        memcpy(p.stage.as<uint8_t>() + off, src, bytes);
        src = p.stage.as<uint8_t>() + off;
    }
    HP_HIP_TRY(hipMemcpyAsync(dst ? dst : p.raw.as<uint8_t>() + off, src, bytes, hipMemcpyHostToDevice, p.s));
    if (!dst || !pinned)
        off += (bytes + 255) & ~(size_t)255;
    return HP_OK;
}

// The one place where the parser's kind is looked at: the hyperpose::parser of `pd` with its constructor arguments (hp_parser_desc, include/hp_hip.h)
// for the network of `ed`.  It reads the engine's outputs by the reference's convention - sorted by name (src/tensorrt.cpp:405) = its argument order.
int make_parser(const hp_parser_desc& pd, const hp_engine_desc& ed, std::unique_ptr<hp::parser_session>& out)
{
    if (pd.kind == HP_PARSER_PAF) {
        hp_paf* h = nullptr;
        HP_TRY(hp_paf_create(&h, pd.thresh[0], pd.thresh[1], pd.res_w, pd.res_h, ed.max_batch));
        out.reset(hp::session_of(h));
    } else if (pd.kind == HP_PARSER_PPN) { // pose_proposal(net_resolution, point_thresh, limb_thresh, mns_thresh)
        hp_ppn* h = nullptr;
        HP_TRY(hp_ppn_create(&h, ed.in_w, ed.in_h, pd.thresh[0], pd.thresh[1], pd.thresh[2], ed.max_batch));
        out.reset(hp::session_of(h));
    } else { // pifpaf(h, w, thresh)
        hp_pifpaf* h = nullptr;
        HP_TRY(hp_pifpaf_create(&h, ed.in_h, ed.in_w, pd.thresh[0], ed.max_batch));
        out.reset(hp::session_of(h));
    }
    HP_REQUIRE(ed.n_outputs == out->engine_outputs(), HP_ERR_INVALID, "hp_pipeline_create: this parser needs a network with exactly %d outputs, the engine has %d",
        out->engine_outputs(), ed.n_outputs);
    return HP_OK;
}

} // namespace

extern "C" {

int hp_pipeline_create(hp_pipeline** out, const hp_engine_desc* desc, int n_pipes, int keep_ratio, float conf_thresh, float paf_thresh,
    size_t max_frame_bytes)
{
    hp_parser_desc pd;
    memset(&pd, 0, sizeof(pd));
    pd.kind = HP_PARSER_PAF;
    pd.thresh[0] = conf_thresh, pd.thresh[1] = paf_thresh;
    pd.res_w = pd.res_h = -1;
    return hp_pipeline_create_ex(out, desc, &pd, n_pipes, keep_ratio, max_frame_bytes);
}

int hp_pipeline_create_ex(hp_pipeline** out, const hp_engine_desc* desc, const hp_parser_desc* parser, int n_pipes, int keep_ratio,
    size_t max_frame_bytes)
{
    HP_REQUIRE(out && desc && parser, HP_ERR_INVALID, "hp_pipeline_create: null argument");
    HP_REQUIRE(n_pipes >= 1 && n_pipes <= 16, HP_ERR_INVALID, "hp_pipeline_create: n_pipes %d", n_pipes);
    HP_REQUIRE(parser->kind >= HP_PARSER_PAF && parser->kind <= HP_PARSER_PIFPAF, HP_ERR_INVALID, "hp_pipeline_create: unknown parser kind %d", parser->kind);
    // HP_DTYPE_F32S is refused here: its guard against values outside fp16's range (|x| > 65504) runs in hp_engine_synchronize /
    // hp_engine_output_to_host, which a pipeline never calls - a batch that overflowed would be parsed and returned as humans with no error
    HP_REQUIRE(desc->dtype != HP_DTYPE_F32S, HP_ERR_INVALID,
        "hp_pipeline_create: HP_DTYPE_F32S engines are for single-stream use (hp_engine_infer_* + hp_engine_synchronize); use HP_DTYPE_F32 or HP_DTYPE_F16 in a pipeline");
    if (desc->dtype == HP_DTYPE_I8) { // every pipe's engine is created calibrated from the same scales: a stream never calibrates by itself
        HP_REQUIRE(desc->int8_scales, HP_ERR_STATE, "hp_pipeline_create: HP_DTYPE_I8 engine without int8 scales: calibrate an engine first (hp_engine_calibrate_u8) and pass its hp_engine_describe");
        for (int i = 0; i < desc->n_layers; ++i)
            HP_REQUIRE(desc->int8_scales[i] >= 0.f, HP_ERR_STATE, "hp_pipeline_create: HP_DTYPE_I8 engine not calibrated (layer %d has scale %g)", i, (double)desc->int8_scales[i]);
    }
    std::unique_ptr<hp_pipeline> pl(new hp_pipeline());
    pl->kind = parser->kind;
    pl->n_pipes = n_pipes, pl->max_batch = desc->max_batch, pl->in_w = desc->in_w, pl->in_h = desc->in_h, pl->keep_ratio = keep_ratio;
    const size_t net_frame = (size_t)desc->in_w * desc->in_h * 3;
    pl->max_frame_bytes = std::max(max_frame_bytes, net_frame);
    pl->pipes = std::vector<pipe_t>(n_pipes);
    for (auto& p : pl->pipes) {
        // engine first, parser second: their streams then alternate over the runtime's hardware queues
        HP_TRY(hp_engine_create(&p.eng, desc));
        HP_TRY(make_parser(*parser, *desc, p.parser));
        p.s = (hipStream_t)hp_engine_stream(p.eng);
        HP_TRY(p.stage.alloc((pl->max_frame_bytes + 256) * desc->max_batch)); // frames are packed at 256-byte offsets
        HP_TRY(p.raw.alloc((pl->max_frame_bytes + 256) * desc->max_batch));
        HP_TRY(p.net.alloc(net_frame * desc->max_batch));
        p.w.assign(desc->max_batch, 0), p.h.assign(desc->max_batch, 0);
        p.roi.assign(desc->max_batch, hp_roi{ 0, 0, 0, 0 });
    }
    *out = pl.release();
    return HP_OK;
}

void hp_pipeline_destroy(hp_pipeline* pl) { delete pl; }

int hp_pipeline_in_flight(const hp_pipeline* pl) { return pl ? pl->inflight : 0; }

int hp_pipeline_set_tiling(hp_pipeline* pl, const hp_tiling* t)
{
    HP_REQUIRE(pl, HP_ERR_INVALID, "hp_pipeline_set_tiling: null pipeline");
    HP_REQUIRE(pl->inflight == 0, HP_ERR_STATE, "hp_pipeline_set_tiling: %d batches are in flight, collect first", pl->inflight);
    if (!t) {
        pl->tiled = false;
        return HP_OK;
    }
    hp_roi probe[64]; // the plan of a frame of the network's size: every rule that does not depend on the frame is checked now
    const int R = hp_tile_plan(t, pl->in_w, pl->in_h, 1, 1, probe, 64);
    if (R < 0)
        return R;
    HP_REQUIRE(R <= pl->max_batch, HP_ERR_CAPACITY, "hp_pipeline_set_tiling: %d regions per frame > max_batch %d", R, pl->max_batch);
    if (!pl->scale_ens.empty()) // (the flip ensemble's message below keeps its wording while the scale ensemble is off)
        HP_REQUIRE(R * pl->passes() <= pl->max_batch, HP_ERR_CAPACITY, "hp_pipeline_set_tiling: %d regions per frame x %d passes (the scale ensemble%s is on) > max_batch %d",
            R, pl->passes(), pl->flip_ensemble ? " and the flip ensemble" : "", pl->max_batch);
    HP_REQUIRE(R <= pl->capacity(), HP_ERR_CAPACITY, "hp_pipeline_set_tiling: %d regions per frame and their flips (the flip ensemble is on) > max_batch %d", R, pl->max_batch);
    HP_REQUIRE(t->min_common >= 1 && t->tol >= 0., HP_ERR_INVALID, "hp_pipeline_set_tiling: min_common %d (>= 1), tol %g (>= 0)", t->min_common, t->tol);
    pl->tiling = *t, pl->tiled = true;
    return HP_OK;
}

int hp_pipeline_set_tonemap(hp_pipeline* pl, const hp_hdr_desc* d)
{
    HP_REQUIRE(pl, HP_ERR_INVALID, "hp_pipeline_set_tonemap: null pipeline");
    HP_REQUIRE(pl->inflight == 0, HP_ERR_STATE, "hp_pipeline_set_tonemap: %d batches are in flight, collect first", pl->inflight);
    hp_tonemap* next = nullptr;
    if (d)
        HP_TRY(hp_tonemap_create(&next, d)); // a refused description leaves the pipeline as it was
    hp_tonemap_destroy(pl->tonemap);
    pl->tonemap = next;
    return HP_OK;
}

int hp_pipeline_set_orientation(hp_pipeline* pl, int orientation)
{
    HP_REQUIRE(pl, HP_ERR_INVALID, "hp_pipeline_set_orientation: null pipeline");
    HP_REQUIRE(orientation >= 0 && orientation <= 7, HP_ERR_INVALID, "hp_pipeline_set_orientation: orientation %d is no HP_ORIENT_* code (0 .. 7)", orientation);
    HP_REQUIRE(pl->inflight == 0, HP_ERR_STATE, "hp_pipeline_set_orientation: %d batches are in flight, collect first", pl->inflight);
    pl->orientation = orientation;
    return HP_OK;
}

int hp_pipeline_set_flip_ensemble(hp_pipeline* pl, int enable)
{
    static const char* const kinds[] = { "HP_PARSER_PAF", "HP_PARSER_PPN", "HP_PARSER_PIFPAF" };
    HP_REQUIRE(pl, HP_ERR_INVALID, "hp_pipeline_set_flip_ensemble: null pipeline");
    HP_REQUIRE(pl->inflight == 0, HP_ERR_STATE, "hp_pipeline_set_flip_ensemble: %d batches are in flight, collect first", pl->inflight);
    HP_REQUIRE(pl->kind == HP_PARSER_PAF, HP_ERR_INVALID, "hp_pipeline_set_flip_ensemble: the flip ensemble is defined for HP_PARSER_PAF pipelines, this one ends in %s",
        kinds[pl->kind]);
    if (enable) {
        const int R = tiled_regions(pl), K = 1 + (int)pl->scale_ens.size();
        if (K > 1) // (the messages below keep their wording while the scale ensemble is off)
            HP_REQUIRE(2 * K * R <= pl->max_batch, HP_ERR_CAPACITY, "hp_pipeline_set_flip_ensemble: %d regions per frame x %d scales (the scale ensemble is on) and their flips > max_batch %d",
                R, K, pl->max_batch);
        HP_REQUIRE(pl->max_batch >= 2, HP_ERR_CAPACITY, "hp_pipeline_set_flip_ensemble: max_batch %d has no room for a frame and its flip", pl->max_batch);
        HP_REQUIRE(!pl->tiled || 2 * R <= pl->max_batch, HP_ERR_CAPACITY, "hp_pipeline_set_flip_ensemble: %d regions per frame (tiling is on) and their flips > max_batch %d", R,
            pl->max_batch);
    }
    for (size_t i = 0; i < pl->pipes.size(); ++i) {
        const int rc = hp_engine_set_flip_ensemble_coco(pl->pipes[i].eng, enable != 0);
        if (rc != HP_OK) { // (every pipe holds the same network: a refusal is the first pipe's, and nothing has changed)
            for (size_t j = 0; j < i; ++j)
                (void)hp_engine_set_flip_ensemble_coco(pl->pipes[j].eng, pl->flip_ensemble);
            return rc;
        }
    }
    pl->flip_ensemble = enable != 0;
    pl->set_note();
    return HP_OK;
}

int hp_pipeline_set_scale_ensemble(hp_pipeline* pl, const float* scales, int n_scales)
{
    static const char* const kinds[] = { "HP_PARSER_PAF", "HP_PARSER_PPN", "HP_PARSER_PIFPAF" };
    HP_REQUIRE(pl, HP_ERR_INVALID, "hp_pipeline_set_scale_ensemble: null pipeline");
    HP_REQUIRE(pl->inflight == 0, HP_ERR_STATE, "hp_pipeline_set_scale_ensemble: %d batches are in flight, collect first", pl->inflight);
    HP_REQUIRE(pl->kind == HP_PARSER_PAF, HP_ERR_INVALID, "hp_pipeline_set_scale_ensemble: the scale ensemble is defined for HP_PARSER_PAF pipelines, this one ends in %s",
        kinds[pl->kind]);
    HP_REQUIRE(n_scales >= 0, HP_ERR_INVALID, "hp_pipeline_set_scale_ensemble: n_scales %d (0 turns the ensemble off, 1 .. 3 extra scales)", n_scales);
    if (n_scales) {
        HP_TRY(hp_scale::check_scales("hp_pipeline_set_scale_ensemble", scales, n_scales));
        const int R = tiled_regions(pl), K = 1 + n_scales, F = pl->flip_ensemble ? 2 : 1;
        HP_REQUIRE(R * K * F <= pl->max_batch, HP_ERR_CAPACITY, "hp_pipeline_set_scale_ensemble: %d region%s per frame x %d scales%s > max_batch %d", R,
            R == 1 ? "" : "s (tiling is on)", K, F == 2 ? " x 2 (the flip ensemble is on)" : "", pl->max_batch);
    }
    for (size_t i = 0; i < pl->pipes.size(); ++i) {
        const int rc = hp_engine_set_scale_ensemble_coco(pl->pipes[i].eng, scales, n_scales);
        if (rc != HP_OK) { // (every pipe holds the same network: a refusal is the first pipe's, and nothing has changed)
            for (size_t j = 0; j < i; ++j)
                (void)hp_engine_set_scale_ensemble_coco(pl->pipes[j].eng, pl->scale_ens.data(), (int)pl->scale_ens.size());
            return rc;
        }
    }
    pl->scale_ens.assign(scales, scales + n_scales);
    pl->set_note();
    return HP_OK;
}

int hp_pipeline_submit(hp_pipeline* pl, const uint8_t* const* frames, const int* widths, const int* heights, int n)
{
    HP_REQUIRE(pl && frames && widths && heights, HP_ERR_INVALID, "hp_pipeline_submit: null argument");
    HP_TRY(admit(pl, "hp_pipeline_submit", n));
    pipe_t& p = pl->pipes[pl->head];
    const int R = tiled_regions(pl);
    const size_t net_frame = (size_t)pl->in_w * pl->in_h * 3;
    std::vector<char> direct(n, 0);
    for (int i = 0; i < n; ++i) { // everything is checked before the first copy is enqueued
        HP_REQUIRE(frames[i] && widths[i] > 0 && heights[i] > 0, HP_ERR_INVALID, "hp_pipeline_submit: frame %d is empty", i);
        HP_REQUIRE((size_t)widths[i] * heights[i] * 3 <= pl->max_frame_bytes, HP_ERR_CAPACITY, "hp_pipeline_submit: frame %d (%dx%d) exceeds max_frame_bytes %zu", i,
            widths[i], heights[i], pl->max_frame_bytes);
        HP_TRY(plan_frame(pl, p, i, widths[i], heights[i], 1, 1));
        // (a) a frame that already has the network's size needs no geometry: cv::resize to the same size is a copy (src/tensorrt.cpp:446-451)
        // and non_scaling_resize at ratio 1 fills the whole target (src/data.cpp:53-69) -> H2D straight into the network's input slot
        // (a stored frame that is turned or mirrored always goes through the oriented kernel, a tiled frame through the regions kernel)
        direct[i] = !pl->tiled && widths[i] == pl->in_w && heights[i] == pl->in_h && pl->orientation == HP_ORIENT_NONE;
    }
    size_t off = 0;
    std::vector<size_t> offs(n);
    for (int i = 0; i < n; ++i) {
        const bool pinned = is_pinned(frames[i]);
        uint8_t* slot = p.net.as<uint8_t>() + (size_t)i * net_frame;
        if (direct[i] && pinned) { // consecutive network-sized frames that are also consecutive in (pinned) host memory go in ONE copy
            int run = 1;
            while (i + run < n && direct[i + run] && frames[i + run] == frames[i] + (size_t)run * net_frame)
                ++run;
            HP_HIP_TRY(hipMemcpyAsync(slot, frames[i], net_frame * run, hipMemcpyHostToDevice, p.s));
            i += run - 1;
            continue;
        }
        offs[i] = off;
        HP_TRY(upload_blob(p, frames[i], (size_t)widths[i] * heights[i] * 3, pinned, direct[i] ? slot : nullptr, off));
    }
    for (int i = 0; i < n; ++i) {
        if (direct[i])
            continue;
        const uint8_t* src = p.raw.as<uint8_t>() + offs[i];
        uint8_t* dst = p.net.as<uint8_t>() + (size_t)i * R * net_frame;
        HP_TRY(pl->tiled ? hp_resize_rois_oriented_u8c3(src, widths[i], heights[i], widths[i] * 3, pl->orientation, &p.roi[(size_t)i * R], R, pl->keep_ratio, 0, 0, 0,
                               dst, pl->in_w, pl->in_h, pl->in_w * 3, net_frame, p.s)
                         : hp_resize_oriented_u8c3(src, widths[i], heights[i], widths[i] * 3, pl->orientation, pl->keep_ratio, 0, 0, 0, dst, pl->in_w, pl->in_h,
                               pl->in_w * 3, p.s));
    }
    return infer_and_parse(pl, p, n * R);
}

int hp_pipeline_submit_yuv(hp_pipeline* pl, int format, const uint8_t* const* frames, const int* widths, const int* heights, int n)
{
    HP_REQUIRE(pl && frames && widths && heights, HP_ERR_INVALID, "hp_pipeline_submit_yuv: null argument");
    HP_REQUIRE(!pl->tiled, HP_ERR_STATE, "hp_pipeline_submit_yuv: not available in tiled mode, submit hp_yuv_image frames with hp_pipeline_submit_yuv_images");
    HP_REQUIRE(pl->orientation == HP_ORIENT_NONE, HP_ERR_STATE,
        "hp_pipeline_submit_yuv: not available while an orientation is set, submit hp_yuv_image frames with hp_pipeline_submit_yuv_images");
    HP_REQUIRE(format == HP_YUV_NV12 || format == HP_YUV_I420, HP_ERR_INVALID, "hp_pipeline_submit_yuv: unknown format %d", format);
    HP_TRY(admit(pl, "hp_pipeline_submit_yuv", n));
    pipe_t& p = pl->pipes[pl->head];
    const size_t net_frame = (size_t)pl->in_w * pl->in_h * 3;
    for (int i = 0; i < n; ++i) { // everything is checked before the first copy is enqueued
        HP_REQUIRE(frames[i] && widths[i] > 0 && heights[i] > 0, HP_ERR_INVALID, "hp_pipeline_submit_yuv: frame %d is empty", i);
        HP_REQUIRE(widths[i] % 2 == 0 && heights[i] % 2 == 0, HP_ERR_INVALID, "hp_pipeline_submit_yuv: frame %d is %d x %d, 4:2:0 frames need even sizes", i,
            widths[i], heights[i]);
        HP_REQUIRE((size_t)widths[i] * heights[i] * 3 / 2 <= pl->max_frame_bytes, HP_ERR_CAPACITY, "hp_pipeline_submit_yuv: frame %d (%dx%d) exceeds max_frame_bytes %zu", i,
            widths[i], heights[i], pl->max_frame_bytes);
    }
    // One copy of the 1.5-byte form per frame (half the bytes of BGR over PCIe); the fused conversion + resize then writes the network's
    // slot - a network-sized frame takes the same road (the kernel converts and nothing else): there is no BGR form of it anywhere to copy
    size_t off = 0;
    std::vector<size_t> offs(n);
    for (int i = 0; i < n; ++i) {
        offs[i] = off, p.w[i] = widths[i], p.h[i] = heights[i];
        HP_TRY(upload_blob(p, frames[i], (size_t)widths[i] * heights[i] * 3 / 2, is_pinned(frames[i]), nullptr, off));
    }
    for (int i = 0; i < n; ++i) {
        const int w = p.w[i], h = p.h[i];
        const size_t luma = (size_t)w * h;
        const uint8_t* raw = p.raw.as<uint8_t>() + offs[i];
        uint8_t* dst = p.net.as<uint8_t>() + (size_t)i * net_frame;
        const uint8_t *u = raw + luma, *v = format == HP_YUV_I420 ? u + luma / 4 : nullptr;
        const int uv_stride = format == HP_YUV_NV12 ? w : w / 2;
        if (pl->keep_ratio)
            HP_TRY(hp_letterbox_yuv420(format, raw, w, u, v, uv_stride, w, h, dst, pl->in_w, pl->in_h, pl->in_w * 3, 0, 0, 0, p.s));
        else
            HP_TRY(hp_resize_yuv420(format, raw, w, u, v, uv_stride, w, h, dst, pl->in_w, pl->in_h, pl->in_w * 3, p.s));
    }
    return infer_and_parse(pl, p, n);
}

int hp_pipeline_submit_yuv_images(hp_pipeline* pl, const hp_yuv_image* frames, int n, int on_device)
{
    HP_REQUIRE(pl && frames, HP_ERR_INVALID, "hp_pipeline_submit_yuv_images: null argument");
    HP_TRY(admit(pl, "hp_pipeline_submit_yuv_images", n));
    pipe_t& p = pl->pipes[pl->head];
    const int R = tiled_regions(pl);
    const size_t net_frame = (size_t)pl->in_w * pl->in_h * 3;
    for (int i = 0; i < n; ++i) { // everything is checked before the first copy is enqueued
        HP_TRY(hp_yuv::validate(&frames[i], "hp_pipeline_submit_yuv_images", on_device != 0));
        HP_REQUIRE(on_device || hp_yuv_packed_bytes(frames[i].format, frames[i].width, frames[i].height) <= pl->max_frame_bytes, HP_ERR_CAPACITY,
            "hp_pipeline_submit_yuv_images: frame %d (%s, %dx%d, %zu bytes) exceeds max_frame_bytes %zu", i, hp_yuv::layout_of(frames[i].format)->name,
            frames[i].width, frames[i].height, hp_yuv_packed_bytes(frames[i].format, frames[i].width, frames[i].height), pl->max_frame_bytes);
        int ax = 1, ay = 1;
        HP_TRY(hp_yuv_roi_alignment(frames[i].format, &ax, &ay));
        HP_TRY(plan_frame(pl, p, i, frames[i].width, frames[i].height, ax, ay));
    }
    std::vector<hp_yuv_image> dev; // each frame as a kernel will read it: the caller's surface, or the tightly packed copy in p.raw
    if (on_device)
        dev.assign(frames, frames + n);
    else
        HP_TRY(upload_yuv_images(p, frames, n, dev));
    for (int i = 0; i < n; ++i) {
        uint8_t* dst = p.net.as<uint8_t>() + (size_t)i * R * net_frame;
        const hp_tonemap* tm = pl->tonemap_for(dev[i]);
        HP_TRY(pl->tiled ? hp_resize_rois_oriented_yuv(&dev[i], tm, pl->orientation, &p.roi[(size_t)i * R], R, pl->keep_ratio, 0, 0, 0, dst, pl->in_w, pl->in_h,
                               pl->in_w * 3, net_frame, p.s)
                         : hp_resize_oriented_yuv(&dev[i], tm, pl->orientation, pl->keep_ratio, 0, 0, 0, dst, pl->in_w, pl->in_h, pl->in_w * 3, p.s));
    }
    return infer_and_parse(pl, p, n * R);
}

int hp_pipeline_submit_rgb_images(hp_pipeline* pl, const hp_rgb_image* frames, int n, int on_device)
{
    const char* who = "hp_pipeline_submit_rgb_images";
    HP_REQUIRE(pl && frames, HP_ERR_INVALID, "%s: null argument", who);
    HP_TRY(admit(pl, who, n));
    pipe_t& p = pl->pipes[pl->head];
    const int R = tiled_regions(pl);
    const size_t net_frame = (size_t)pl->in_w * pl->in_h * 3;
    for (int i = 0; i < n; ++i) { // everything is checked before the first copy is enqueued
        HP_TRY(hp_rgb::validate(&frames[i], who, on_device != 0));
        const size_t bytes = hp_rgb_packed_bytes(frames[i].format, frames[i].width, frames[i].height);
        HP_REQUIRE(on_device || bytes <= pl->max_frame_bytes, HP_ERR_CAPACITY, "%s: frame %d (%s, %dx%d, %zu bytes) exceeds max_frame_bytes %zu", who, i,
            hp_rgb::layout_of(frames[i].format)->name, frames[i].width, frames[i].height, bytes, pl->max_frame_bytes);
        HP_TRY(plan_frame(pl, p, i, frames[i].width, frames[i].height, 1, 1));
    }
    std::vector<hp_rgb_image> dev; // each frame as a kernel will read it: the caller's surface, or the tightly packed copy in p.raw
    if (on_device)
        dev.assign(frames, frames + n);
    else
        HP_TRY(upload_rgb_images(p, frames, n, dev));
    for (int i = 0; i < n; ++i) { // (8-bit SDR frames: the pipeline's tone-map has nothing to act on)
        uint8_t* dst = p.net.as<uint8_t>() + (size_t)i * R * net_frame;
        HP_TRY(pl->tiled ? hp_resize_rois_rgb(&dev[i], pl->orientation, &p.roi[(size_t)i * R], R, pl->keep_ratio, 0, 0, 0, dst, pl->in_w, pl->in_h, pl->in_w * 3,
                               net_frame, p.s)
                         : hp_resize_rgb(&dev[i], pl->orientation, pl->keep_ratio, 0, 0, 0, dst, pl->in_w, pl->in_h, pl->in_w * 3, p.s));
    }
    return infer_and_parse(pl, p, n * R);
}

} // extern "C"

namespace {

// the part of a submit that does not depend on how the frames arrived: p.net holds n network-sized BGR slots (in stream order on p.s)
// -> conv stack -> the pipeline's parser, and the pipe joins the ring of batches in flight (a tiled batch: as n / R frames of R regions)
int infer_and_parse(hp_pipeline* pl, pipe_t& p, int n)
{
    HP_TRY(hp_engine_infer_u8(p.eng, p.net.as<uint8_t>(), n, 1, p.s));
    HP_TRY(p.parser->enqueue_outputs(p.eng, n, p.s));
    p.n = n, p.regions = pl->tiled ? tiled_regions(pl) : 0;
    pl->head = (pl->head + 1) % pl->n_pipes;
    ++pl->inflight;
    return HP_OK;
}

// host frames of hp_pipeline_submit_yuv_images: every frame's planes tightly packed into p.raw (one copy per frame, enqueued on p.s);
// `dev` describes each frame as a kernel will read it there
int upload_yuv_images(pipe_t& p, const hp_yuv_image* frames, int n, std::vector<hp_yuv_image>& dev)
{
    dev.assign(frames, frames + n);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const hp_yuv_image& f = frames[i];
        const hp_yuv::layout& l = *hp_yuv::layout_of(f.format);
        const size_t bytes = hp_yuv_packed_bytes(f.format, f.width, f.height);
        // one contiguous, tightly packed buffer (what hp_pipeline_submit_yuv takes) in pinned memory goes up from where it lies
        bool tight = true;
        size_t at = 0;
        for (int k = 0; k < l.planes; ++k) {
            const size_t row = hp_yuv::row_bytes(l, k, f.width);
            tight = tight && (size_t)f.stride[k] == row && (const uint8_t*)f.plane[k] == (const uint8_t*)f.plane[0] + at;
            dev[i].plane[k] = p.raw.as<uint8_t>() + off + at, dev[i].stride[k] = (int32_t)row;
            at += row * hp_yuv::rows(l, k, f.height);
        }
        const uint8_t* src = (const uint8_t*)f.plane[0];
        if (!tight || !is_pinned(src)) {
            uint8_t* to = p.stage.as<uint8_t>() + off;
            src = to;
            for (int k = 0; k < l.planes; ++k) {
                const size_t row = hp_yuv::row_bytes(l, k, f.width);
                for (int r = 0; r < hp_yuv::rows(l, k, f.height); ++r, to += row)
                    memcpy(to, (const uint8_t*)f.plane[k] + (size_t)r * f.stride[k], row);
            }
        }
        HP_HIP_TRY(hipMemcpyAsync(p.raw.as<uint8_t>() + off, src, bytes, hipMemcpyHostToDevice, p.s));
        off += (bytes + 255) & ~(size_t)255;
    }
    return HP_OK;
}

// host frames of hp_pipeline_submit_rgb_images: every frame's rows tightly packed into p.raw in the frame's own layout (one copy per frame, enqueued
// on p.s; the 256-byte offsets keep the 4-byte layouts aligned); `dev` describes each frame as a kernel will read it there
int upload_rgb_images(pipe_t& p, const hp_rgb_image* frames, int n, std::vector<hp_rgb_image>& dev)
{
    dev.assign(frames, frames + n);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const hp_rgb_image& f = frames[i];
        const size_t row = (size_t)f.width * hp_rgb::layout_of(f.format)->pixel_bytes, bytes = row * f.height;
        const uint8_t* src = (const uint8_t*)f.data;
        if ((size_t)f.stride != row || !is_pinned(src)) {
            uint8_t* to = p.stage.as<uint8_t>() + off;
            for (int r = 0; r < f.height; ++r)
                memcpy(to + (size_t)r * row, src + (size_t)r * f.stride, row);
            src = to;
        }
        dev[i].data = p.raw.as<uint8_t>() + off, dev[i].stride = (int32_t)row;
        HP_HIP_TRY(hipMemcpyAsync(p.raw.as<uint8_t>() + off, src, bytes, hipMemcpyHostToDevice, p.s));
        off += (bytes + 255) & ~(size_t)255;
    }
    return HP_OK;
}

// the first half of every collect: the parser's list of every slot of the batch in pipe p (room for `cap` humans per slot, n_out their counts),
// and the pipe leaves the ring whatever the parser answered
int collect_slots(hp_pipeline* pl, pipe_t& p, hp_human* out, int cap, int* n_out)
{
    const int rc = p.parser->collect(out, cap, n_out);
    p.n = 0, p.regions = 0;
    pl->tail = (pl->tail + 1) % pl->n_pipes;
    --pl->inflight;
    return rc;
}

// hp_pipeline_collect of a tiled batch: the parser's lists of all slots, then per frame resume_ratio per region (keep_ratio), the way back
// to the frame and the merge.  A frame of ONE region has nothing to merge and keeps the parser's order: a 1 x 1 tiling is tiling off.
int collect_tiled(hp_pipeline* pl, pipe_t& p, hp_human* out, int cap_per_frame, int* n_out, int* n_frames)
{
    HP_REQUIRE(cap_per_frame > 0, HP_ERR_INVALID, "hp_pipeline_collect: cap_per_frame %d", cap_per_frame);
    const int slots = p.n, R = p.regions, frames = slots / R, cap = cap_per_frame;
    pl->slot_humans.resize((size_t)slots * cap);
    pl->slot_n.resize(slots);
    hp_human* sh = pl->slot_humans.data();
    int rc = collect_slots(pl, p, sh, cap, pl->slot_n.data());
    *n_frames = frames;
    if (rc != HP_OK && rc != HP_ERR_CAPACITY)
        return rc;
    for (int f = 0; f < frames; ++f) {
        pl->cand.clear(), pl->cand_region.clear();
        for (int r = 0; r < R; ++r) {
            const int slot = f * R + r, cnt = std::min(pl->slot_n[slot], cap);
            hp_human* hs = sh + (size_t)slot * cap;
            const hp_roi& roi = p.roi[slot];
            if (pl->keep_ratio)
                hp_resume_ratio(hs, cnt, roi.w, roi.h, pl->in_w, pl->in_h);
            hp_humans_to_frame(hs, cnt, &roi, p.w[f], p.h[f]);
            pl->cand.insert(pl->cand.end(), hs, hs + cnt);
            pl->cand_region.insert(pl->cand_region.end(), cnt, r);
        }
        int total = (int)pl->cand.size();
        const hp_human* from = pl->cand.data();
        if (R == 1)
            total = pl->slot_n[f]; // the parser's own count, as an untiled collect reports it
        else {
            HP_TRY(hp::merge_humans(pl->cand.data(), pl->cand_region.data(), total, p.w[f], p.h[f], pl->tiling.min_common, pl->tiling.tol, pl->kept));
            total = (int)pl->kept.size(), from = pl->kept.data();
        }
        n_out[f] = total;
        if (out && std::min(total, cap) > 0)
            memcpy(out + (size_t)f * cap, from, sizeof(hp_human) * std::min(total, cap));
        if (total > cap && rc == HP_OK) {
            hp::set_error("hp_pipeline_collect: frame %d has %d humans after the merge, room for %d", f, total, cap);
            rc = HP_ERR_CAPACITY;
        }
    }
    return rc;
}

} // namespace

extern "C" {

int hp_pipeline_collect(hp_pipeline* pl, hp_human* out, int cap_per_frame, int* n_out, int* n_frames)
{
    HP_REQUIRE(pl && n_out && n_frames, HP_ERR_INVALID, "hp_pipeline_collect: null argument");
    HP_REQUIRE(pl->inflight > 0, HP_ERR_STATE, "hp_pipeline_collect: nothing in flight");
    pipe_t& p = pl->pipes[pl->tail];
    if (p.regions)
        return collect_tiled(pl, p, out, cap_per_frame, n_out, n_frames);
    const int n = p.n;
    const int rc = collect_slots(pl, p, out, cap_per_frame, n_out);
    *n_frames = n;
    if ((rc == HP_OK || rc == HP_ERR_CAPACITY) && out && pl->keep_ratio) // (capacity: that frame's list is cut, everything returned is valid)
        for (int i = 0; i < n; ++i) // src/stream.cpp:120-124
            hp_resume_ratio(out + (size_t)i * cap_per_frame, std::min(n_out[i], cap_per_frame), p.w[i], p.h[i], pl->in_w, pl->in_h);
    return rc;
}

} // extern "C"
