/* include/hp_hip.h — C ABI of libhp_hip.so, the MI355X (gfx950) implementation of HyperPose's hot path.
 *
 * HyperPose has no FFI of its own: the boundary of its hot path is a set of C++17 classes
 * (SURVEY.md section 8b).  This header is the thin C layer the north star asks for: the C++ mirror
 * classes in include/hyperpose/ (same names, signatures and error behaviour as the reference headers)
 * are implemented purely on top of these entry points, and any other host language can bind them
 * directly (INTEGRATION.md shows the ctypes / C++ stubs).
 *
 * Conventions: plain pointers and sizes only; opaque handles; every function returns HP_OK (0) or a
 * negative HP_ERR_* code and never throws or exits across the ABI; hp_last_error() returns a
 * thread-local description of the last failure.  One handle is used by one thread at a time (same rule
 * as the reference: include/hyperpose/stream/stream.hpp:139-144, openpifpaf_postprocessor.hpp:23-26).
 * "dev" pointers are HIP device pointers on the device given to hp_init(); "host" pointers are
 * ordinary (ideally pinned) host memory.
 */
#ifndef HP_HIP_H
#define HP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HP_OK 0
#define HP_ERR_INVALID (-1)   /* bad argument / shape */
#define HP_ERR_HIP (-2)       /* a HIP runtime call failed */
#define HP_ERR_CAPACITY (-3)  /* a fixed-capacity device list overflowed (peaks, candidates, humans, batch) */
#define HP_ERR_STATE (-4)     /* call order violated (e.g. collect without enqueue; shape changed after first call) */
#define HP_ERR_NO_DEVICE (-5) /* no gfx950 device visible */

#define HP_COCO_N_PARTS 18 /* include/hyperpose/utility/human.hpp:10 */
#define HP_COCO_N_PAIRS 19 /* include/hyperpose/utility/human.hpp:11 */

/* hyperpose::body_part_t / human_t (include/hyperpose/utility/human.hpp:14-31), same 292-byte layout
 * (has_value is the reference's `bool` widened to its 4-byte slot: 0 or 1). */
typedef struct hp_body_part {
    int32_t has_value;
    float x, y, score;
} hp_body_part;

typedef struct hp_human {
    hp_body_part parts[HP_COCO_N_PARTS];
    float score;
} hp_human;

/* peak_info (src/post_process.hpp:126-131) and connection (src/paf.cpp:7-13) — exposed only for the
 * stage-wise parity taps below. */
typedef struct hp_peak {
    int32_t part_id;
    int32_t x, y;
    float score;
    int32_t id;
} hp_peak;

typedef struct hp_conn {
    int32_t pair_id;
    int32_t cid1, cid2;
    float score;
} hp_conn;

/* ---- runtime ------------------------------------------------------------------------------------ */
int hp_init(int device);            /* hipSetDevice(device) for the calling thread; checks the arch is gfx950 */
int hp_device_count(void);          /* number of visible HIP devices, or a negative HP_ERR_* */
const char* hp_last_error(void);    /* thread-local, never NULL */
const char* hp_version(void);

/* Device memory helpers so that a host language needs no HIP binding of its own. */
int hp_malloc(void** dev, size_t nbytes);
int hp_free(void* dev);
int hp_malloc_host(void** host, size_t nbytes); /* pinned */
int hp_free_host(void* host);
int hp_memcpy_h2d(void* dev, const void* host, size_t nbytes);
int hp_memcpy_d2h(void* host, const void* dev, size_t nbytes);
int hp_device_synchronize(void);
/* Everything enqueued on `waiter` after this call starts only after everything enqueued on `signaler` before it has
 * finished (hipEventRecord + hipStreamWaitEvent).  Lets a parser run on its own stream behind its engine, the way the
 * reference's stream pipeline hands a batch from its inference thread to its parser thread (stream.hpp:139-190). */
int hp_stream_wait_stream(void* waiter, void* signaler);

/* ---- multi-GPU: frames shard over the GPUs of a node, one process per GPU, no steady-state collective.  The one
 * collective is the start-up broadcast of the weight blob over RCCL / xGMI.  Rendezvous: rank 0 calls hp_dist_unique_id and hands the
 * 128 bytes to the other ranks by whatever channel launched them (a file, an environment variable, MPI, a TCP store);
 * every rank then calls hp_dist_init after hp_init(device).  librccl.so is loaded on first use. */
#define HP_DIST_ID_BYTES 128
typedef struct hp_comm hp_comm;
int hp_dist_unique_id(char id[HP_DIST_ID_BYTES]);
int hp_dist_init(hp_comm** out, int rank, int world, const char id[HP_DIST_ID_BYTES]);
void hp_dist_destroy(hp_comm* c);
/* host_weights [n]: read on `root`, overwritten on every other rank (ncclBroadcast through a device buffer) */
int hp_dist_broadcast_weights(hp_comm* c, float* host_weights, size_t n, int root);
/* contiguous split of a global batch over the ranks: rank r processes frames [start, start + count) */
void hp_dist_shard(int total_frames, int rank, int world, int* start, int* count);

/* ---- pre-processing: replaces hyperpose::nhwc_images_append_nchw_batch (src/data.cpp:21-51) -------
 * u8 HWC (BGR) frames [n,h,w,3] -> f32 CHW [n,3,h,w], value = (float)((double)u8 * factor), channel
 * order {2,1,0} when flip_rb.  Both pointers are device pointers; `stream` is a hipStream_t (NULL = default). */
int hp_preproc_u8hwc_to_f32nchw(const uint8_t* dev_hwc, int n, int h, int w, double factor, int flip_rb,
                                float* dev_nchw, void* stream);

/* ---- stream front-end geometry (reference: cv::resize at src/stream.cpp:93,101 and hyperpose::non_scaling_resize,
 * include/hyperpose/utility/data.hpp:67, src/data.cpp:53-69; resume_ratio, include/hyperpose/utility/human.hpp:44-58).
 * Images are 8-bit BGR HWC in DEVICE memory, row strides in bytes; results equal OpenCV's INTER_LINEAR bit for bit
 * (restated in oracle/resize_oracle.cpp; parity unpinned: no OpenCV in the build image). */
int hp_resize_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, uint8_t* dev_dst, int dw, int dh, int dst_stride,
                   void* stream);
/* non_scaling_resize: aspect-preserving resize into the top-left corner, the rest filled with (b, g, r) */
int hp_letterbox_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, uint8_t* dev_dst, int dw, int dh, int dst_stride,
                      int b, int g, int r, void* stream);
void hp_letterbox_inner(int sw, int sh, int dw, int dh, int* inner_w, int* inner_h); /* size of the resized region */
/* resume_ratio on n humans in place (host memory): undo the letterbox for (src = frame size, dst = network size) */
void hp_resume_ratio(hp_human* humans, int n, int src_w, int src_h, int dst_w, int dst_h);

/* ---- video frames as decoders deliver them: YUV 4:2:0 in DEVICE memory -> the same 8-bit BGR HWC result as "convert the whole frame
 * with cv::cvtColor(COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420), then hp_resize_u8c3 / hp_letterbox_u8c3", bit for bit, in one kernel
 * (hyperpose_amd/csrc/resize_yuv.hip).  Conversion is OpenCV's 8-bit fixed-point BT.601 limited-range form, chroma replicated over its
 * 2 x 2 luma pixels (restated from the constants; parity unpinned: no OpenCV in the build image).  Planes are addressed by separate
 * pointers and byte strides, so decoder surfaces with padded pitch work.  Width and height must be even (HP_ERR_INVALID otherwise).
 *   HP_YUV_NV12  Y plane (sh rows), dev_u = ONE plane of sh/2 rows of sw/2 interleaved (U, V) byte pairs; dev_v is ignored
 *   HP_YUV_I420  Y plane, dev_u and dev_v = two planes of sh/2 rows of sw/2 bytes, both with row stride uv_stride
 * (these two entry points take the two 8-bit 4:2:0 layouts at BT.601 limited range; every other layout, depth, matrix and range goes
 * through hp_yuv_image below) */
enum { HP_YUV_NV12 = 0, HP_YUV_I420 = 1,
       HP_YUV_P010 = 2,   /* 4:2:0, semi-planar, 16-bit little-endian words, the sample in the HIGH 10 bits (value = word >> 6) */
       HP_YUV_I010 = 3,   /* 4:2:0, three planes, 16-bit words, the sample in the LOW 10 bits (value = word & 1023): yuv420p10le */
       HP_YUV_NV16 = 4,   /* 4:2:2, Y plane + interleaved (U, V) plane of full height, half width */
       HP_YUV_I422 = 5,   /* 4:2:2, three planes */
       HP_YUV_YUY2 = 6,   /* 4:2:2 packed, bytes Y0 U Y1 V */
       HP_YUV_UYVY = 7,   /* 4:2:2 packed, bytes U Y0 V Y1 */
       HP_YUV_I444 = 8 }; /* 4:4:4, three planes */
int hp_resize_yuv420(int format, const uint8_t* dev_y, int y_stride, const uint8_t* dev_u, const uint8_t* dev_v, int uv_stride,
                     int sw, int sh, uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream);
int hp_letterbox_yuv420(int format, const uint8_t* dev_y, int y_stride, const uint8_t* dev_u, const uint8_t* dev_v, int uv_stride,
                        int sw, int sh, uint8_t* dev_dst, int dw, int dh, int dst_stride, int b, int g, int r, void* stream);

/* ---- one description of a video frame: layout (above), colour matrix, range, size, planes.  hp_resize_yuv / hp_letterbox_yuv are the
 * fused conversion + resize for every combination (hyperpose_amd/csrc/resize_yuv_formats.hip); the output is always 8-bit BGR HWC and
 * equals "convert the whole frame, then hp_resize_u8c3 / hp_letterbox_u8c3" bit for bit.  Chroma is replicated over the luma pixels it
 * covers (no interpolation).  With Y, U, V the d-bit samples (d = 8, or 10 for P010 / I010 - converted at their own precision):
 *     u = U - c_off   v = V - c_off   yy = max(0, Y - y_off) * CY + (1 << 19)
 *     B = sat8((yy + CUB*u) >> 20)   G = sat8((yy + CVG*v + CUG*u) >> 20)   R = sat8((yy + CVR*v) >> 20)
 * where the seven integers are what hp_yuv_coefficients returns: OpenCV's constants for (BT601, LIMITED, 8 bits) - so NV12 / I420 give
 * the bytes of hp_resize_yuv420 and YUY2 / UYVY those of cv::cvtColor(COLOR_YUV2BGR_YUY2 / _UYVY) - and otherwise the rounded 2^20
 * multiples of the matrix's terms (non-constant-luminance forms).  Sizes: 4:2:0 needs even width and height, 4:2:2 an even width, 4:4:4
 * any size >= 1; a stride must cover a row of its plane (every plane has its own: the U and the V plane of a planar frame may differ in
 * pitch); planes and strides of the 16-bit formats must be even wherever the kernel reads them (device planes).  A violation is
 * HP_ERR_INVALID with a message that names the format, and nothing is launched.  A P016 buffer is accepted as P010 (low six bits ignored). */
enum { HP_YUV_BT601 = 0, HP_YUV_BT709 = 1, HP_YUV_BT2020 = 2 };
enum { HP_YUV_LIMITED = 0, HP_YUV_FULL = 1 };
typedef struct hp_yuv_image {
    int32_t format, matrix, range, width, height;
    const void* plane[3];      /* Y (or the packed plane), U or UV, V; unused entries NULL */
    int32_t stride[3];         /* row strides in BYTES: decoder surfaces with padded pitch work */
} hp_yuv_image;
int hp_resize_yuv(const hp_yuv_image* src /* planes in DEVICE memory */, uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream);
int hp_letterbox_yuv(const hp_yuv_image* src, uint8_t* dev_dst, int dw, int dh, int dst_stride, int b, int g, int r, void* stream);
/* the integer table a (matrix, range, depth) selects: out = { y_off, c_off, CY, CUB, CUG, CVG, CVR }; depth 8 or 10 (host only) */
int hp_yuv_coefficients(int matrix, int range, int depth, int32_t out[7]);
/* bytes of one tightly packed frame of this format (planes back to back, no row padding); 0 for an invalid format or size */
size_t hp_yuv_packed_bytes(int format, int width, int height);
/* the one statement of a layout's geometry: returns the number of planes of `format` (0 = unknown format) and, for plane k of a
 * width x height frame, the bytes of one row without padding and the number of rows (both 0 for a k or a size the layout cannot hold);
 * either pointer may be NULL (host only) */
int hp_yuv_plane_layout(int format, int k, int width, int height, size_t* row_bytes, int* rows);

/* ---- regions and tiles: inference on overlapping tiles of a frame much larger than the network's input ("sliced inference"), so that
 * small people keep enough pixels (hyperpose_amd/csrc/resize_rois.hip, tiles.cpp; DESIGN.md 1.1 "Regions and tiles").
 *
 * hp_resize_rois_*: n regions (1 .. 64, a HOST array) of one DEVICE frame to n slots of dev_dst, slot i at dev_dst + i * slot_stride, in
 * ceil(n / 16) launches; the call only enqueues.  Slot i holds, byte for byte, what hp_resize_u8c3 / hp_resize_yuv (keep_ratio == 0) or
 * hp_letterbox_u8c3 / hp_letterbox_yuv with (b, g, r) (keep_ratio != 0) give on region i cut out into a frame of its own (the w x h
 * sub-image; for YUV the sub-planes of every plane, same matrix, range and depth): mode and letterbox inner size are picked per region,
 * taps clamp at the region's edges and no pixel outside a region is read.  Bytes of dev_dst beyond dw * 3 in a row and beyond dh rows in
 * a slot are not written.  HP_ERR_INVALID, nothing launched and dev_dst untouched: n outside 1 .. 64; a region empty or not inside the
 * frame; for YUV a region whose x / w (y / h) is no multiple of the layout's alignment (hp_yuv_roi_alignment; the message names the
 * format and the region); slot_stride < dh * dst_stride; whatever hp_resize_yuv rejects for the frame itself. */
typedef struct hp_roi { int32_t x, y, w, h; } hp_roi; /* source pixels, inside the frame */
int hp_resize_rois_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, const hp_roi* rois /* host */, int n, int keep_ratio,
                        int b, int g, int r, uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream);
int hp_resize_rois_yuv(const hp_yuv_image* src /* device planes */, const hp_roi* rois, int n, int keep_ratio, int b, int g, int r,
                       uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream);
/* host only: what a region's x and w (ax) and y and h (ay) must be multiples of: 4:2:0 -> 2, 2; 4:2:2 planar and packed -> 2, 1; I444 -> 1, 1 */
int hp_yuv_roi_alignment(int format, int* ax, int* ay);

/* The tile planner, the way back and the merge: host only, plain C++, deterministic; integers and IEEE doubles, no fused operations.
 *
 * hp_tile_plan, per axis (W the frame's size, c the tile count, a the alignment, o = align_up(overlap, a): the overlap asked for, rounded
 * up to the alignment so that tiles which may only start at multiples of a still share at least `overlap` pixels):
 *     tw  = min(W, align_up(ceil_div(W + (c - 1) * o, c), a))
 *     x_i = align_down(i * (W - tw) / (c - 1), a)  (integer division; 0 when c == 1),  x_{c-1} = W - tw
 * so the tiles cover the frame exactly and neighbours share at least `overlap` pixels wherever tw < W.  Regions are written row-major
 * (all tiles of the first row of tiles, left to right, then the next row), after the whole frame when with_full.  Returns the region
 * count; HP_ERR_INVALID for W % a != 0 (either axis), counts < 1, a negative overlap or cols * rows + with_full > 64; HP_ERR_CAPACITY
 * when cap is smaller than the count (nothing is written).
 *
 * hp_humans_to_frame: humans normalised to a region (after hp_resume_ratio(region size -> network size) when letterboxed, exactly as for
 * a whole frame) -> normalised to the frame: for every part with has_value,  x = (float)((roi.x + (double)x * roi.w) / frame_w),  y
 * likewise.  For a region equal to the frame this is the identity on every float (x * W is exact in a double, and so is the quotient).
 *
 * hp_humans_merge: in[i] (frame coordinates) came from region region_of[i] (0 .. 63).  A part is present when has_value != 0; its pixel
 * position is px = (double)x * frame_w, py = (double)y * frame_h.  Candidates are taken by human score descending, then region
 * ascending, then index ascending, and walked once with a kept list K (empty at first).  Candidate c fuses into the first k of K, in
 * kept order, for which  (1) k holds no contribution from c's region yet (two people the parser separated inside one tile are never
 * fused),  (2) the parts present in both number m >= min_common,  (3) sum_j d_j <= tol * m * max(s(k), s(c)),  where d_j =
 * sqrt(dx * dx + dy * dy) of common part j (summed by ascending part index) and s(h) = max(max px - min px, max py - min py) over h's
 * present parts; the right side is evaluated as (tol * m) * max.  Fusing: a part k lacks is copied from c; where both have it the
 * higher part score wins and a tie keeps k's; k keeps its human score and gains c's region; later candidates see the fused k.  A
 * candidate that fuses nowhere is appended to K.  Returns the number kept, written to out in kept order; HP_ERR_CAPACITY when that
 * exceeds cap (the first cap are written); HP_ERR_INVALID for a region outside 0 .. 63, min_common < 1 or a tol that is negative or NaN.
 * Defaults of the mirrors (a product decision, no part of the contract): min_common = 3, tol = 0.08 - two detections are one person
 * when at least three joints coincide to within 8 % of the larger one's extent on average. */
#define HP_TILING_DEFAULT_MIN_COMMON 3
#define HP_TILING_DEFAULT_TOL 0.08
typedef struct hp_tiling {
    int32_t cols, rows;            /* >= 1, cols*rows + with_full <= 64 */
    int32_t overlap_x, overlap_y;  /* pixels two neighbouring tiles share at least */
    int32_t with_full;             /* 1: the whole frame is region 0, the tiles follow row-major */
    int32_t min_common; double tol;/* merge rule above */
} hp_tiling;
int hp_tile_plan(const hp_tiling* t, int frame_w, int frame_h, int ax, int ay, hp_roi* out, int cap); /* returns the region count */
void hp_humans_to_frame(hp_human* humans, int n, const hp_roi* roi, int frame_w, int frame_h);
int hp_humans_merge(const hp_human* in, const int32_t* region_of, int n, int frame_w, int frame_h, int min_common, double tol,
                    hp_human* out, int cap); /* returns the count kept */

/* ---- HDR video in: PQ (SMPTE ST 2084) and HLG (BT.2100) 10-bit frames - HDR10 / HLG as a Main10 decoder hands them out, P010 or I010 with the BT.2020
 * matrix - tone-mapped to the network's 8-bit sRGB BGR input inside the fused resize (hyperpose_amd/csrc/resize_yuv_hdr.hip; the rule is stated once in
 * csrc/tonemap.hpp and DESIGN.md 1.1).  hp_yuv_image does not grow: the HDR description travels beside it.  Per source pixel, with Y, U, V the 10-bit
 * samples and k = hp_yuv_coefficients(matrix, range, 10), everything int32 with arithmetic shifts:
 *   1. R'G'B' at 10 bits    u = U - c_off, v = V - c_off, yy = max(0, Y - y_off) * CY + (1 << 17);  E_B = sat10((yy + CUB*u) >> 18),
 *                           E_G = sat10((yy + CVG*v + CUG*u) >> 18), E_R = sat10((yy + CVR*v) >> 18), sat10 clamps to [0, 1023]; full scale is 1020 (255 * 4)
 *   2. SDR linear light     L_c = A[E_c] per channel, A[i] = rint(65535 * tm(nits(min(i, 1020) / 1020.0))), uint16 [1024]
 *                           PQ:  nits(e) = 10000 * EOTF_ST2084(e) (m1 = 2610/16384, m2 = 128 * 2523/4096, c1 = 3424/4096, c2 = 32 * 2413/4096, c3 = 32 * 2392/4096)
 *                           HLG: nits(e) = 1000 * invOETF_BT2100(e)^1.2 (a = 0.17883277, b = 0.28466892, c = 0.55991073): the system gamma of a 1000 cd/m2
 *                                display applied PER CHANNEL - an approximation of BT.2100's OOTF, which scales R, G, B by a power of their luminance
 *                           tm(L): x = L / white_nits, p = peak_nits / white_nits, tm = min(1, x * (1 + x / (p * p)) / (1 + x)): extended Reinhard, applied
 *                                per channel (not on luminance, so saturated highlights desaturate), monotone, tm(peak_nits) = 1
 *   3. primaries            when to_bt709:  (R, G, B) = clamp((M * (L_R, L_G, L_B) + 2048) >> 12, 0, 65535), M = rint(4096 * M_2020->709), M_2020->709 =
 *                           inv(RGB709->XYZ) * RGB2020->XYZ from the two sets of chromaticities and D65 in double:
 *                           M = { 6801, -2407, -298,  -510, 4640, -34,  -74, -412, 4582 }, every row sums to 4096 (greys stay grey)
 *   4. sRGB bytes           c8 = O[value >> 4], O[j] = rint(255 * sRGB_OETF((16 * j + 7.5) / 65535.0)), uint8 [4096]
 * and the output equals, byte for byte, "convert the whole frame to 8-bit BGR by this rule (hp_tonemap_convert_host), then hp_resize_u8c3 /
 * hp_letterbox_u8c3": conversion happens per tap, the resize arithmetic is the one every other feed has.  The defaults below are a product decision
 * (BT.2408 reference white, a 1000 cd/m2 grade), no part of the contract.  HP_ERR_INVALID, with a message that names the argument, and nothing launched:
 * a transfer other than HP_TRC_PQ / HP_TRC_HLG; peak_nits or white_nits not finite, or not 0 < white_nits <= peak_nits <= 10000; an 8-bit layout given to
 * a *_hdr call (the message names the format); a null handle; whatever the SDR twin of the call refuses. */
enum { HP_TRC_PQ = 1, HP_TRC_HLG = 2 };
#define HP_HDR_DEFAULT_PEAK 1000.0f
#define HP_HDR_DEFAULT_WHITE 203.0f
typedef struct hp_hdr_desc {
    int32_t transfer, to_bt709; /* HP_TRC_*; to_bt709 != 0: step 3 (BT.2020 primaries -> BT.709), 0: the channels are taken as they are */
    float peak_nits, white_nits;
} hp_hdr_desc;
/* host only: the ONE statement of the three tables (as hp_yuv_coefficients is of the matrix); m is row-major, the identity * 4096 when to_bt709 == 0 */
int hp_tonemap_tables(const hp_hdr_desc* d, uint16_t lin[1024], int32_t m[9], uint8_t out[4096]);
/* the handle owns the tables in device memory (6 KiB), immutable after create; destroy waits for the device */
typedef struct hp_tonemap hp_tonemap;
int hp_tonemap_create(hp_tonemap** out, const hp_hdr_desc* d);
void hp_tonemap_destroy(hp_tonemap* t);
/* the HDR twins of hp_resize_yuv / hp_letterbox_yuv / hp_resize_rois_yuv for P010 / I010 frames: same argument rules, they only enqueue */
int hp_resize_yuv_hdr(const hp_yuv_image* src /* device planes */, const hp_tonemap* t, uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream);
int hp_letterbox_yuv_hdr(const hp_yuv_image* src, const hp_tonemap* t, uint8_t* dev_dst, int dw, int dh, int dst_stride, int b, int g, int r, void* stream);
int hp_resize_rois_yuv_hdr(const hp_yuv_image* src, const hp_tonemap* t, const hp_roi* rois, int n, int keep_ratio, int b, int g, int r,
                           uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream);
/* the whole-frame conversion in plain C++, no device: a P010 / I010 frame in HOST memory (any address, any stride that covers a row) -> 8-bit BGR HWC */
int hp_tonemap_convert_host(const hp_yuv_image* host_frame, const hp_hdr_desc* d, uint8_t* bgr, int stride);

/* ---- upright input: frames that are STORED turned and / or mirrored (the container's display matrix, EXIF orientation 1 .. 8, a ceiling camera) read
 * upright inside the fused resize - no rotation pass over the full-resolution surface (hyperpose_amd/csrc/resize_oriented.hip, orientation.cpp;
 * DESIGN.md 1.1 "Orientation").  The ONE definition:
 *
 * Orientation code HP_ORIENT_*, 0 .. 7:  code = q + 4 * m,  q = quarter turns CLOCKWISE that bring the stored picture upright (0, 1, 2, 3 = 0, 90,
 * 180, 270 degrees),  m = 1 when the stored picture is mirrored left-right FIRST, before the turn.  With the stored frame S of sw x sh, the
 * upright frame U is uw x uh = sw x sh for even q and sh x sw for odd q, and with S'(x, y) = S(m ? sw-1-x : x, y):
 *     q = 0:  U(ux, uy) = S'(ux, uy)                 q = 1:  U(ux, uy) = S'(uy, sh-1-ux)
 *     q = 2:  U(ux, uy) = S'(sw-1-ux, sh-1-uy)       q = 3:  U(ux, uy) = S'(sw-1-uy, ux)
 * (numpy: np.rot90(S[:, ::-1] if m else S, k=-q)).  EXIF orientations 1 .. 8 are the codes { 0, 4, 2, 6, 7, 1, 5, 3 } (hp_orientation_from_exif).
 *
 * Contract of every feed (8-bit BGR, every SDR hp_yuv_image layout, PQ / HLG 10-bit with a tone-map): an oriented call writes, byte for byte, what
 * the existing pipeline gives in three steps - 1. convert the whole stored frame to 8-bit BGR by that feed's own rule, 2. orient it by the map above
 * (hp_orient_u8c3_host), 3. hp_resize_u8c3 (keep_ratio == 0) / hp_letterbox_u8c3 with (b, g, r) (keep_ratio != 0) from uw x uh.  The definition is in
 * the BGR domain on purpose: a turned 4:2:2 frame is not a 4:2:2 frame, and chroma stays replicated over the luma pixels it covers in the STORED
 * frame.  Mode (linear / 2 x 2 area / copy) and the letterbox inner size come from (uw, uh).
 *
 * The device calls only enqueue.  tm == NULL: an SDR frame; otherwise a P010 / I010 PQ / HLG frame ("HDR video in" above).  The region calls take
 * regions in UPRIGHT coordinates; slot i equals the per-frame oriented result on the upright cut-out, and every other rule is hp_resize_rois_*'s
 * (1 .. 64 regions, ceil(n / 16) launches, bytes outside a slot's dw * 3 x dh untouched).  The YUV alignment (hp_yuv_roi_alignment) applies to the
 * STORED rectangle of a region (hp_orient_roi): for odd q an upright x, w must be multiples of ay and y, h of ax.  Orientation 0 forwards to the
 * existing call: the same kernels, bytes and refusals.  HP_ERR_INVALID, with a message that names the argument, and nothing launched: an
 * orientation outside 0 .. 7; whatever the un-oriented twin refuses; an 8-bit layout passed with a tone-map. */
enum { HP_ORIENT_NONE = 0, HP_ORIENT_CW90 = 1, HP_ORIENT_180 = 2, HP_ORIENT_CW270 = 3,
       HP_ORIENT_HFLIP = 4, HP_ORIENT_HFLIP_CW90 = 5, HP_ORIENT_HFLIP_180 = 6 /* = a vertical flip */, HP_ORIENT_HFLIP_CW270 = 7 /* = a transpose */ };
int hp_resize_oriented_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, int orientation, int keep_ratio, int b, int g, int r,
                            uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream);
int hp_resize_oriented_yuv(const hp_yuv_image* src /* device planes */, const hp_tonemap* tm /* NULL = SDR */, int orientation, int keep_ratio,
                           int b, int g, int r, uint8_t* dev_dst, int dw, int dh, int dst_stride, void* stream);
int hp_resize_rois_oriented_u8c3(const uint8_t* dev_src, int sw, int sh, int src_stride, int orientation, const hp_roi* rois /* host, upright */, int n,
                                 int keep_ratio, int b, int g, int r, uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream);
int hp_resize_rois_oriented_yuv(const hp_yuv_image* src, const hp_tonemap* tm, int orientation, const hp_roi* rois, int n, int keep_ratio,
                                int b, int g, int r, uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream);
/* Host only, plain C++, no device.  All return HP_OK or HP_ERR_INVALID (an orientation outside 0 .. 7, an empty frame, a null pointer, a stride
 * smaller than a row, a region that is empty or not inside the upright frame). */
int hp_oriented_size(int orientation, int sw, int sh, int* uw, int* uh);
int hp_orientation_from_exif(int exif); /* the code (>= 0) of EXIF orientation 1 .. 8, or HP_ERR_INVALID */
/* the stored rectangle that an upright region covers (same pixel count, w and h swapped for odd q) */
int hp_orient_roi(const hp_roi* upright, int orientation, int sw, int sh, hp_roi* stored);
/* the materialised upright BGR frame (uw x uh, rows dst_stride bytes apart; padding bytes are not written): the definition above, the reference of
 * the tests and the fallback of a caller without a device */
int hp_orient_u8c3_host(const uint8_t* src, int sw, int sh, int src_stride, int orientation, uint8_t* dst, int dst_stride);
/* Humans between the two frames, in place, on NORMALISED coordinates (hp_overlay_draw_* paints into the stored frame): only parts with has_value are
 * touched, scores stay, fp32 exactly as written.  to_stored != 0, upright (u, v) -> stored (x, y):
 *     q = 0: (x', y') = (u, v)   q = 1: (v, 1.0f-u)   q = 2: (1.0f-u, 1.0f-v)   q = 3: (1.0f-v, u);   then x = m ? 1.0f-x' : x',  y = y'
 * to_stored == 0 is the inverse, stored (x, y) -> upright (u, v):  x' = m ? 1.0f-x : x,  y' = y,  then
 *     q = 0: (u, v) = (x', y')   q = 1: (1.0f-y', x')   q = 2: (1.0f-x', 1.0f-y')   q = 3: (y', 1.0f-x')
 * 1.0f - (1.0f - t) rounds, so a round trip need not return the same float (it does for every t that is a multiple of 2^-24 in [0, 1]). */
int hp_humans_orient(hp_human* humans, int n, int orientation, int to_stored);

/* ---- packed RGB and grey frames: what sources other than a video decoder deliver - screen and window capture, compositors, canvases and 4-channel
 * pictures (4-byte pixels), PIL / imageio / PPM pictures (RGB order), IR and machine-vision cameras (grey) - read by the fused resize where they lie,
 * with a stride, in host or device memory: no repack on the CPU (hyperpose_amd/csrc/resize_rgb.hip, rgb_formats.hpp; DESIGN.md 1.1 "Packed RGB and grey
 * frames").  A type of its own: the codes are not hp_yuv_image formats.  The ONE rule:
 *     memory order is as the name reads: HP_RGB_BGRA32 is bytes B, G, R, A; HP_RGB_ARGB32 is A, R, G, B; HP_RGB_RGB24 is R, G, B
 *     the fourth byte of the 4-byte layouts (alpha or padding) is ignored: no premultiplication, no blend
 *     HP_RGB_GRAY8 gives B = G = R = the sample
 *     any width and height >= 1;  stride (bytes) >= width * pixel bytes
 *     where a kernel reads the plane where it lies (the device calls, on_device submits), `data` and `stride` of the 4-byte layouts must be multiples
 *     of 4: a pixel is fetched as one aligned word.  Host frames are re-packed bytewise and have no such rule
 * A violation is HP_ERR_INVALID with a message that names the layout ("HP_RGB_BGRA32" ...) and the offending quantity, and nothing is launched.
 * hp_rgb_to_bgr_host is the definition: the whole frame as 8-bit BGR.
 *
 * Contract of the device calls: for every layout, size, orientation code 0 .. 7, keep_ratio and (b, g, r) the bytes written equal what
 * hp_resize_oriented_u8c3 (hp_resize_rgb) / hp_resize_rois_oriented_u8c3 (hp_resize_rois_rgb) give on hp_rgb_to_bgr_host(src); the other arguments and
 * the refusals (orientation outside 0 .. 7, n outside 1 .. 64, a region outside the upright frame, a short slot_stride, ...) are theirs, bytes of
 * dev_dst those calls leave alone are left alone, and the region alignment is 1 x 1 for every layout.  An HP_RGB_BGR24 image gives the bytes of the
 * _u8c3 entry points on the same buffer.  No byte outside width * pixel bytes of a row is read.  The calls only enqueue. */
enum { HP_RGB_BGR24 = 0, HP_RGB_RGB24 = 1, HP_RGB_BGRA32 = 2, HP_RGB_RGBA32 = 3, HP_RGB_ARGB32 = 4, HP_RGB_ABGR32 = 5, HP_RGB_GRAY8 = 6 };
typedef struct hp_rgb_image {
    int32_t format, width, height;
    const void* data;
    int32_t stride; /* bytes */
} hp_rgb_image;
int hp_resize_rgb(const hp_rgb_image* src /* data in DEVICE memory */, int orientation, int keep_ratio, int b, int g, int r, uint8_t* dev_dst, int dw,
                  int dh, int dst_stride, void* stream);
int hp_resize_rois_rgb(const hp_rgb_image* src, int orientation, const hp_roi* rois /* host, upright */, int n, int keep_ratio, int b, int g, int r,
                       uint8_t* dev_dst, int dw, int dh, int dst_stride, size_t slot_stride, void* stream);
/* Host only.  Bytes of one pixel (0 for an unknown format); bytes of one tightly packed frame (0 for an invalid format or size) */
int hp_rgb_pixel_bytes(int format);
size_t hp_rgb_packed_bytes(int format, int width, int height);
/* the whole HOST frame as 8-bit BGR, rows bgr_stride bytes apart (>= width * 3; padding bytes are not written): the definition above */
int hp_rgb_to_bgr_host(const hp_rgb_image* src, uint8_t* bgr, int bgr_stride);

/* ---- encoder hand-off: a packed RGB or grey frame as the frame a video encoder takes - any hp_yuv_image layout, in the matrix, range and bit depth the
 * stream is tagged with, padded to the size the encoder needs - converted on the device (hyperpose_amd/csrc/to_yuv.hip; the rule is stated once in
 * to_yuv.hpp and DESIGN.md 1.1 "Encoder hand-off").  The forward counterpart of hp_resize_yuv; the annotators below (hp_overlay_*, hp_redact_*,
 * hp_mapview_*) work on the result as on a decoder's surface: capture -> hp_rgb_to_yuv -> redact / maps / skeletons -> encoder, all on the device.
 *   coefficients  hp_yuv_forward_coefficients: kr, kb of the matrix, kg = 1 - kr - kb, d = 8 or 10, S = 18, float64;
 *                 LIMITED ys = 219 2^(d-8) / 255, cs = 224 2^(d-8) / 255, y_off = 16 2^(d-8), c_off = 128 2^(d-8); FULL ys = cs = (2^d - 1) / 255,
 *                 y_off = 0, c_off = 2^(d-1);  YR = rint(kr ys 2^S), YB = rint(kb ys 2^S), YG = rint(ys 2^S) - YR - YB;
 *                 UB = rint(0.5 cs 2^S), UR = -rint(kr / (2 (1 - kb)) cs 2^S), UG = -UB - UR;  VR = rint(0.5 cs 2^S),
 *                 VB = -rint(kb / (2 (1 - kr)) cs 2^S), VG = -VR - VB;  out = { y_off, c_off, YR, YG, YB, UR, UG, UB, VR, VG, VB }
 *   pixel         R, G, B as hp_rgb_to_bgr_host defines them;  Y = clip((YR R + YG G + YB B + (y_off << 18) + (1 << 17)) >> 18)
 *   chroma        one sample covers n = 1 (4:4:4), 2 (4:2:2) or 4 (4:2:0) luma pixels, Rs, Gs, Bs their sums (the box mean; no co-sited filter):
 *                 U = clip((UR Rs + UG Gs + UB Bs + n ((c_off << 18) + (1 << 17))) >> (18 + log2 n)), V likewise; clip to [0, 2^d - 1]; all int32.
 *                 A grey pixel gives exactly c_off; against hp_yuv_colours' float rule a sample differs by at most 1 code value
 *   padding       dst may be larger than src: output pixel (x, y) takes source pixel (min(x, sw - 1), min(y, sh - 1)) (edge replication), for odd
 *                 captures going to 4:2:0 and for an encoder's alignment (1080 -> 1088); hp_yuv_padded_size gives such a size
 *   samples       where hp_yuv_image's layouts put them; 16-bit layouts store value << shift (P010: 6, I010: 0), the other bits zero
 * No byte of dst outside the samples of its width x height is written (row padding included), no byte of src outside width * pixel bytes of a row is
 * read.  src and dst must not overlap: that is the caller's responsibility and is not checked.  HP_ERR_INVALID, with a message that names the layout
 * and the quantity, nothing launched and dst untouched: whatever hp_resize_yuv rejects for an image (dst: format, matrix, range, a size the layout
 * cannot hold, a null plane, a short stride, odd planes / strides of the 16-bit layouts on the device), whatever the hp_rgb_image rules reject (src),
 * dst narrower or lower than src, dst wider or higher than 8192.  No resize, no orientation, no HDR transfer, no alpha. */
int hp_rgb_to_yuv(const hp_rgb_image* src /* data in DEVICE memory */, const hp_yuv_image* dst /* planes in DEVICE memory, WRITTEN */, void* stream);
/* the same bytes on frames in HOST memory (plain C++, written bytewise: the definition of the device call; no device needed) */
int hp_rgb_to_yuv_host(const hp_rgb_image* src, const hp_yuv_image* dst);
/* host only: the integer table above for a matrix / range / depth (8 or 10) */
int hp_yuv_forward_coefficients(int matrix, int range, int depth, int32_t out[11]);
/* host only: the smallest size >= width x height (both 1 .. 8192) whose sides are multiples of `align` (1 .. 256) and of what the layout needs */
int hp_yuv_padded_size(int format, int width, int height, int align, int* padded_width, int* padded_height);

/* ---- writing back: the skeletons of a frame's humans painted into a DEVICE-resident frame, 8-bit BGR or any hp_yuv_image layout in the frame's
 * own colour space and bit depth (hyperpose_amd/csrc/overlay.hip) - the last stage of the reference's stream, draw_human + writer
 * (src/stream.cpp:114-147), for frames that never leave the device.  The picture is defined by exact integer rules, stated once in
 * hyperpose_amd/csrc/overlay.hpp and DESIGN.md 1.1 (it is NOT cv::line / cv::circle's anti-alias-free raster, and says so):
 *   primitives   per human, in order: limbs pair_id 0..18 whose two parts are present, as capsules, then parts 0..17, as discs; a part is present
 *                when has_value and x, y are finite; points are int(x * w), int(y * h) in fp32; T = thickness when > 0 (<= 16384), else the
 *                reference's max(1, int(sqrtf((e - w) * (s - n) * (w * h))) / 32) per human; a primitive with a point outside [-8192, 16383] is
 *                dropped; a disc has (x1, y1) = (x0, y0)
 *   coverage     int64, p = (x - x0, y - y0), d = (x1 - x0, y1 - y0), L = d.d, s = p.d.  capsule: L == 0 or s <= 0: 4 p.p <= T^2; s >= L:
 *                4 (p - d).(p - d) <= T^2; else 4 (p.x d.y - p.y d.x)^2 <= T^2 L.  disc: p.p <= T^2.  The last covering primitive wins.
 *   samples      w = nearbyint(opacity * 256); a covered sample becomes (c * w + old * (256 - w) + 128) >> 8 (w == 256: c); a chroma sample is written
 *                when any of the 1 x 1 / 2 x 1 / 2 x 2 pixels it covers is, with the colour of the last primitive covering any of them; nothing
 *                else is read or written (row padding included).  YUV colours: hp_yuv_colours.
 * The handle owns pinned staging slots and device lists for up to max_humans humans per call; a draw call only ENQUEUES on `stream` (NULL = the
 * default stream) and does not wait for the previous call.  Frames follow hp_resize_yuv's rules (sizes per layout, strides cover a row, even
 * planes / strides for the 16-bit layouts); also HP_ERR_INVALID, with a message that names the format and nothing launched: opacity outside
 * (0, 1], n > max_humans, width or height over 8192.  n == 0 is HP_OK and launches nothing. */
typedef struct hp_overlay hp_overlay;
typedef struct hp_overlay_prim {
    int32_t kind; /* 0 capsule, 1 disc */
    int32_t x0, y0, x1, y1, t;
    int32_t colour; /* 0..18 */
    int32_t human;
} hp_overlay_prim;
int hp_overlay_create(hp_overlay** out, int max_humans);
void hp_overlay_destroy(hp_overlay* o);
/* host only: the primitive list; returns the count (or a negative HP_ERR_*), writes at most cap entries */
int hp_overlay_primitives(const hp_human* humans, int n, int w, int h, int thickness, hp_overlay_prim* out, int cap);
/* host only: the 19 colours of draw_human as d-bit (Y, U, V) for a matrix / range / depth (8 or 10): Y' = Kr R + Kg G + Kb B on [0, 1],
 * Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)), float64; limited: Y = nearbyint((16 + 219 Y') 2^(d-8)), C = nearbyint((128 + 224 Cx) 2^(d-8));
 * full: Y = nearbyint(Y' (2^d - 1)), C = nearbyint(2^(d-1) + Cx (2^d - 1)); clipped to [0, 2^d - 1] */
int hp_yuv_colours(int matrix, int range, int depth, int32_t out[19][3]);
/* device frames, written in place; humans in host memory, already in the FRAME's normalised coordinates (after resume_ratio) */
int hp_overlay_draw_u8c3(hp_overlay* o, uint8_t* dev_bgr, int w, int h, int stride, const hp_human* humans, int n, float opacity, int thickness,
                         void* stream);
int hp_overlay_draw_yuv(hp_overlay* o, const hp_yuv_image* frame /* planes in DEVICE memory, WRITTEN */, const hp_human* humans, int n, float opacity,
                        int thickness, void* stream);
/* the same picture on frames in HOST memory (plain C++, the integer rules above; no device needed) */
int hp_overlay_draw_u8c3_host(uint8_t* bgr, int w, int h, int stride, const hp_human* humans, int n, float opacity, int thickness);
int hp_overlay_draw_yuv_host(const hp_yuv_image* frame, const hp_human* humans, int n, float opacity, int thickness);
/* Drawing on HDR frames.  hp_yuv_colours paints "red" at the code for 10 000 cd/m2 of a PQ frame; hp_yuv_colours_hdr gives draw_human's 19 colours as
 * graphics white at white_nits (BT.2408), 10-bit (Y, U, V), all in float64 then nearbyint: sRGB EOTF of c / 255 per channel; when to_bt709 the inverse
 * of the (unrounded) primaries matrix above, clipped at 0; times white_nits; the inverse PQ EOTF of nits / 10000, or for HLG (nits / 1000)^(1 / 1.2)
 * followed by the HLG OETF; then the Y'CbCr formulas of hp_yuv_colours at depth 10.  peak_nits takes no part.  Host only.
 * hp_overlay_set_transfer: d == NULL means SDR (the default).  While set, hp_overlay_draw_yuv uses that table on the 10-bit layouts (8-bit frames and
 * BGR are painted as before); hp_overlay_draw_yuv_host_hdr is the host twin (d == NULL: hp_overlay_draw_yuv_host).  The kernels are the same: colours
 * are a host table packed into the primitives. */
int hp_yuv_colours_hdr(int matrix, int range, const hp_hdr_desc* d, int32_t out[19][3]);
int hp_overlay_set_transfer(hp_overlay* o, const hp_hdr_desc* d);
int hp_overlay_draw_yuv_host_hdr(const hp_yuv_image* frame, const hp_hdr_desc* d, const hp_human* humans, int n, float opacity, int thickness);

/* ---- redaction: the heads or the whole persons of a frame made unrecognisable in a DEVICE-resident frame before it is encoded, stored or shown,
 * 8-bit BGR or any hp_yuv_image layout (hyperpose_amd/csrc/redact.hip) - the write-back counterpart of the overlay.  The picture is defined by
 * exact integer rules, stated once in hyperpose_amd/csrc/redact.hpp and DESIGN.md 1.1 "Redaction":
 *   regions      RECT covers the pixels of [x0, x1] x [y0, y1], inclusive (x0 <= x1, y0 <= y1); DISC has centre (x0, y0) and radius x1 >= 0, y1 == 0;
 *                coordinates in [-8192, 16383], radii in [0, 16384]; `human` is informational (-1 for a caller's own region - a licence plate, a screen)
 *   from humans  hp_redact_regions: points are int(x * w), int(y * h) in fp32, a part is present when has_value, x and y are finite and the point lies
 *                in [-8192, 16383]^2; m = nearbyint(margin * 256), margin in (0, 8].  Head disc per human: over the present parts among nose, eyes, ears
 *                (0, 14 .. 17; none: no disc) the bounding box lo, hi gives the centre floor((lo + hi) / 2) and e = its longer side; nk = isqrt(|neck -
 *                nose|^2), sh = isqrt(|shoulder - shoulder|^2) >> 1 where present, else 0; r = min(16384, max(1, (max(e, nk, sh, 1) * m + 128) >> 8)).
 *                HP_REDACT_HEAD: that disc.  HP_REDACT_BODY: first a RECT, the bounding box of ALL present parts grown by p = max(1, (its longer side *
 *                m + 1024) >> 11) and clamped into the coordinate range, then the head disc.
 *   cells        `cell` even, 2 .. 128, grid anchored at pixel (0, 0), edge cells partial.  A cell is hit when any region reaches it: a RECT that
 *                intersects it; a DISC with dx * dx + dy * dy <= r * r (int64) for d = centre - the centre clamped into the cell.  A union: order and
 *                overlap do not matter.  A hit cell is rewritten whole, every sample of every plane in it; nothing else is written (row padding included).
 *   effect       HP_REDACT_PIXELATE: each of B, G, R / Y, U, V becomes (sum + cnt / 2) / cnt over that channel's samples in the cell, on code values
 *                (P010: word >> 6, stored << 6; I010: word & 1023).  HP_REDACT_BLACK: BGR 0; Y = 16 << (d - 8) limited, 0 full; U = V = 1 << (d - 1).
 * The handle owns pinned staging slots and device lists for up to max_regions regions per call; a call only ENQUEUES one launch on `stream` (NULL =
 * the default stream) and does not wait for the previous call.  Frames follow hp_resize_yuv's rules, width and height at most 8192.  HP_ERR_INVALID,
 * with a message that names the format or the offending value, nothing launched and the frame untouched: cell odd or outside 2 .. 128, an unknown
 * effect or kind, a region outside the ranges above, n > max_regions, margin outside (0, 8].  n == 0 is HP_OK and launches nothing. */
enum { HP_REDACT_RECT = 0, HP_REDACT_DISC = 1 };
enum { HP_REDACT_HEAD = 0, HP_REDACT_BODY = 1 };
enum { HP_REDACT_PIXELATE = 0, HP_REDACT_BLACK = 1 };
typedef struct hp_redact_region {
    int32_t kind, x0, y0, x1, y1, human;
} hp_redact_region;
typedef struct hp_redact hp_redact;
int hp_redact_create(hp_redact** out, int max_regions);
void hp_redact_destroy(hp_redact* r);
/* host only: the regions of a frame's humans, in order; returns the count (or a negative HP_ERR_*), writes at most cap entries (at most 2 per human) */
int hp_redact_regions(const hp_human* humans, int n, int w, int h, int what, float margin, hp_redact_region* out, int cap);
/* device frames, rewritten in place; regions in host memory, in the frame's pixels */
int hp_redact_u8c3(hp_redact* r, uint8_t* dev_bgr, int w, int h, int stride, const hp_redact_region* regions, int n, int effect, int cell, void* stream);
int hp_redact_yuv(hp_redact* r, const hp_yuv_image* frame /* planes in DEVICE memory, WRITTEN */, const hp_redact_region* regions, int n, int effect,
                  int cell, void* stream);
/* the same picture on frames in HOST memory (plain C++, the integer rules above; no device needed) */
int hp_redact_u8c3_host(uint8_t* bgr, int w, int h, int stride, const hp_redact_region* regions, int n, int effect, int cell);
int hp_redact_yuv_host(const hp_yuv_image* frame, const hp_redact_region* regions, int n, int effect, int cell);

/* ---- map view: what the network itself produced - confidence maps, part-affinity fields - colour-mapped, up-sampled and blended into a DEVICE-
 * resident frame, 8-bit BGR or any hp_yuv_image layout in the frame's own matrix, range and bit depth (hyperpose_amd/csrc/mapview.hip): do the maps
 * light up on the people?  The third annotator, and the dense one: it rewrites the whole region.  The picture is defined by exact rules, stated once
 * in hyperpose_amd/csrc/mapview.hpp and DESIGN.md 1.1 "Map view":
 *   index plane  the frame's maps [C][mh][mw] (fp32) -> uint8 [mh][mw], fp32 without fused operations, channels c_k = c0 + k * c_step, k < cn.
 *                HP_MAPVIEW_MAX: m = 0; per channel: if (v > m) m = v (NaN and negatives leave m alone).  HP_MAPVIEW_FIELD: channel pairs (c_k,
 *                c_k + 1) are (x, y) of a vector field; e = ax * ax + ay * ay; if (e > m2) m2 = e; m = sqrt(m2) correctly rounded.  Then
 *                t = m * gain; t = t < 1.f ? t : 1.f; q = (int)rintf(t * 255.f).
 *   taps         hp_mapview_taps, host doubles: the frame covers the fraction `cover` in (0, 1] of the m cells of an axis (hp_mapview_cover: iw /
 *                (double)dw of hp_letterbox_inner for a letter-boxed slot, else 1).  For U upright pixels scale = (cover * m) / U, s = (u + 0.5) *
 *                scale - 0.5; s < 0: {0, 0, 0}; else i = floor(s): { min(i, m - 1), min(i + 1, m - 1), (int)nearbyint((s - i) * 2048) } - the
 *                half-pixel convention of the parser's up-sampling, so a blob lies under the key point drawn from it.
 *   pixel index  int32: top = p[y0][x0] * (2048 - wx) + p[y0][x1] * wx, bot the same on row y1, idx = (top * (2048 - wy) + bot * wy + (1 << 21)) >> 22.
 *   geometry     roi in stored pixels inside the frame (has_roi == 0: the whole frame); with the HP_ORIENT_* code's (swap, flip_x, flip_y) and a
 *                stored pixel (lx, ly) local to the w x h roi: a = flip_x ? w - 1 - lx : lx, b = flip_y ? h - 1 - ly : ly, (ux, uy) = swap ? (b, a) :
 *                (a, b); the x table has swap ? h : w entries over mw with cover_x, the y table the other count over mh with cover_y.
 *   palette      256 entries (R, G, B, A) in [0, 255].  hp_mapview_palette: float64, t = i / 255, nearbyint(255 * clamp01(c)); JET r = 1.5 - |4t - 3|,
 *                g = 1.5 - |4t - 2|, b = 1.5 - |4t - 1|; HEAT r = 3t, g = 3t - 1, b = 3t - 2; GREY r = g = b = t; A = 255 (ALPHA_CONSTANT) or i
 *                (ALPHA_SCALED).  A YUV frame: each entry through hp_yuv_colours' formulas at the frame's matrix / range / depth
 *                (hp_mapview_palette_yuv: out = (Y, U, V, A)).  SDR formulas only: a PQ / HLG frame gets them at depth 10, graphics white is out of scope.
 *   samples      W = nearbyint(opacity * 256), opacity in (0, 1]; w = (W * A[idx] + 127) / 255; a B / G / R or luma sample with w > 0 becomes
 *                (c * w + old * (256 - w) + 128) >> 8 on code values (P010: word >> 6, stored << 6; I010: & 1023); a chroma sample takes the largest
 *                idx among its 1 x 1 / 2 x 1 / 2 x 2 pixels that lie in the roi and blends U and V with that idx's weight; weight 0 or no pixel in
 *                the roi: the sample keeps its value.  No byte outside the roi's samples is read or written (row padding included).
 * The bilinear rule above is the only up-sampling; there is no blur.  The handle owns pinned staging slots and device slots (palette, the two tap
 * tables, the index plane) for maps of up to max_map_cells cells; a draw call only ENQUEUES on `stream` (NULL = the default stream): one copy, two
 * launches, one event.  `maps` is a DEVICE pointer laid out as hp_engine_output's [frame][C][mh][mw] and must stay valid until the stream has run
 * the call.  Frames follow hp_resize_yuv's rules, width and height at most 8192.  HP_ERR_INVALID, with a message that names the value, nothing
 * launched and the frame untouched: opacity outside (0, 1]; gain not finite or <= 0; a cover outside (0, 1]; cn < 1 or c_step < 1; a channel (FIELD:
 * a pair's second channel) >= C; mh * mw > max_map_cells; frame < 0; an unknown mode or orientation; a roi empty or not inside the frame; a
 * palette value outside [0, 255]. */
enum { HP_MAPVIEW_MAX = 0, HP_MAPVIEW_FIELD = 1 };
enum { HP_MAPVIEW_JET = 0, HP_MAPVIEW_HEAT = 1, HP_MAPVIEW_GREY = 2 };
enum { HP_MAPVIEW_ALPHA_CONSTANT = 0, HP_MAPVIEW_ALPHA_SCALED = 1 };
typedef struct hp_mapview_desc {
    const float* maps;              /* [frames][C][mh][mw], fp32 */
    int32_t C, mh, mw;
    int32_t frame;                  /* which frame of the batch */
    int32_t c0, cn, c_step, mode;   /* the channel choice; HP_MAPVIEW_MAX or HP_MAPVIEW_FIELD */
    float gain;
    double cover_x, cover_y;        /* hp_mapview_cover */
    int32_t orientation;            /* HP_ORIENT_*: how the frame is stored */
    hp_roi roi;                     /* stored pixels; read when has_roi != 0 */
    int32_t has_roi;
} hp_mapview_desc;
typedef struct hp_mapview hp_mapview;
int hp_mapview_create(hp_mapview** out, int max_map_cells);
void hp_mapview_destroy(hp_mapview* v);
/* host only.  cover: the fractions of the network's input a frame_w x frame_h (upright) frame fills, and so of the maps' cells */
int hp_mapview_cover(int frame_w, int frame_h, int in_w, int in_h, int keep_ratio, double cover[2]);
int hp_mapview_taps(int U, int m, double cover, int32_t (*out)[3]); /* U entries (i0, i1, weight); U in 1 .. 8192, m in 1 .. 65535 */
int hp_mapview_palette(int kind, int alpha_mode, int32_t out[256][4]);
int hp_mapview_palette_yuv(const int32_t rgba[256][4], int matrix, int range, int depth, int32_t out[256][4]);
/* device frames, written in place */
int hp_mapview_draw_u8c3(hp_mapview* v, uint8_t* dev_bgr, int w, int h, int stride, const hp_mapview_desc* d, const int32_t palette[256][4],
                         float opacity, void* stream);
int hp_mapview_draw_yuv(hp_mapview* v, const hp_yuv_image* frame /* planes in DEVICE memory, WRITTEN */, const hp_mapview_desc* d,
                        const int32_t palette[256][4], float opacity, void* stream);
/* the same picture with maps and frame in HOST memory (plain C++, the rules above; no device needed); hp_mapview_index_host: the index plane
 * alone, mh * mw bytes */
int hp_mapview_draw_u8c3_host(uint8_t* bgr, int w, int h, int stride, const hp_mapview_desc* d, const int32_t palette[256][4], float opacity);
int hp_mapview_draw_yuv_host(const hp_yuv_image* frame, const hp_mapview_desc* d, const int32_t palette[256][4], float opacity);
int hp_mapview_index_host(const hp_mapview_desc* d, uint8_t* out);
/* tests: synchronises the device, then copies the index plane of the handle's last draw call (at most cap bytes); returns its size in cells */
int hp_mapview_debug_plane(hp_mapview* v, uint8_t* out, int cap);

/* ---- hyperpose::parser::paf (include/hyperpose/operator/parser/paf.hpp:17-93, src/paf.cpp) -------- */
typedef struct hp_paf hp_paf;

/* paf::paf(conf_thresh, paf_thresh, resolution_size) (paf.hpp:27).  res_w/res_h = -1 keeps the reference's
 * lazy default `cv::Size(dim1*4, dim2*4)` of the first processed tensor (src/paf.cpp:314-315, including its
 * swapped naming: width = 4*rows, height = 4*cols).  max_batch sizes the device scratch. */
int hp_paf_create(hp_paf** out, float conf_thresh, float paf_thresh, int res_w, int res_h, int max_batch);
void hp_paf_destroy(hp_paf* p);
int hp_paf_set_conf_thresh(hp_paf* p, float thresh); /* paf::set_conf_thresh, src/paf.cpp:382 */
int hp_paf_set_paf_thresh(hp_paf* p, float thresh);  /* paf::set_paf_thresh,  src/paf.cpp:377 */

/* paf::process(conf, paf) (src/paf.cpp:300-375) for n frames at once.
 *   conf [n, J, rows, cols], paf [n, 2L, rows, cols], fp32, contiguous; shapes WITHOUT batch dim as in
 *   feature_map_t::shape() (include/hyperpose/utility/data.hpp:22-23).  on_device != 0: device pointers.
 *   out: host array [n * cap_per_frame]; n_out: host array [n] receiving the human count of every frame.
 * Blocks until the result is on the host.  The first call fixes the shapes (reference: lazy one-shot
 * allocation, src/paf.cpp:321-332; a later call with other shapes returns HP_ERR_STATE instead of UB). */
int hp_paf_process_batch(hp_paf* p, int n, const float* conf, const int conf_shape[3], const float* paf,
                         const int paf_shape[3], int on_device, hp_human* out, int cap_per_frame, int* n_out);

void* hp_paf_stream(hp_paf* p); /* hipStream_t the parser owns (used when enqueue is given stream = NULL) */
/* Asynchronous halves of the same call for pipelines: enqueue launches the kernels and the D2H copy of the
 * humans on `stream` (NULL = the parser's own stream) and returns at once; collect waits for that batch. */
int hp_paf_enqueue(hp_paf* p, int n, const float* dev_conf, const int conf_shape[3], const float* dev_paf,
                   const int paf_shape[3], void* stream);
int hp_paf_collect(hp_paf* p, hp_human* out, int cap_per_frame, int* n_out);

/* Stage-wise parity taps (valid after a completed process/collect): the peak list (post_process.hpp:171-193
 * order) and the per-limb connections (src/paf.cpp:252-270 order) of one frame of the last batch. */
int hp_paf_debug_peaks(hp_paf* p, int frame, hp_peak* out, int cap, int* n);
int hp_paf_debug_conns(hp_paf* p, int frame, hp_conn* out, int cap, int* n);
/* The up-sampled (resize_area) and the smoothed (GaussianBlur) confidence maps [J,res_h,res_w] of ONE frame,
 * host pointers, either output may be NULL (tests only; the production kernels never materialise them). */
int hp_paf_debug_maps(hp_paf* p, const float* host_conf, const int conf_shape[3], float* host_up, float* host_smoothed);
/* The restatement of libstdc++'s std::sort that all three parsers share (csrc/libstdcxx_sort.hpp), run on the device as
 * std::sort(first, last, std::greater<connection_candidate>) (src/paf.cpp:249: the order of equal scores is whatever that algorithm
 * leaves) on n scores given in generation order; host_order[i] = index of the element that ends at position i; *used_heap = 1
 * when the introsort depth limit was hit and the heap-sort fall-back ran (tests only). */
int hp_paf_debug_sort(const float* host_scores, int n, int* host_order, int* used_heap);

/* ---- hyperpose::parser::pose_proposal (include/hyperpose/operator/parser/proposal_network.hpp:17-81,
 * src/pose_proposal.cpp).  GPU: threshold + box decode + per-class NMS + limb-candidate gather; host: the
 * order-dependent tail (limb selection, hash merge, filter) on the compacted lists. */
typedef struct hp_ppn hp_ppn;
/* pose_proposal(net_resolution, point_thresh = 0.10, limb_thresh = 0.05, mns_thresh = 0.3), proposal_network.hpp:26 */
int hp_ppn_create(hp_ppn** out, int net_w, int net_h, float point_thresh, float limb_thresh, float nms_thresh, int max_batch);
void hp_ppn_destroy(hp_ppn* p);
int hp_ppn_set_thresholds(hp_ppn* p, float point_thresh, float limb_thresh, float nms_thresh); /* set_{point,limb,nms}_thresh */
/* pose_proposal::process (src/pose_proposal.cpp:68-337) for n frames: tensors[7] = {conf_point, conf_iou, x, y, w, h,
 * edge}, each batch-major contiguous ([n,K,gh,gw] x6, [n,E,nh,nw,gh,gw]); conf_shape = {K,gh,gw}, edge_shape =
 * {E,nh,nw,gh,gw}; on_device != 0: device pointers.  out: host [n*cap_per_frame]; n_out: host [n]. */
int hp_ppn_process_batch(hp_ppn* p, int n, const float* const tensors[7], const int conf_shape[3], const int edge_shape[5],
                         int on_device, hp_human* out, int cap_per_frame, int* n_out);
/* Asynchronous halves (same contract as hp_paf_enqueue / hp_paf_collect): enqueue launches the extraction kernel on `stream`
 * (NULL = the parser's own), which writes its compacted lists straight into pinned host memory, and returns at once; collect waits
 * for that batch and runs the order-dependent tail of its frames on the library's host worker pool. */
void* hp_ppn_stream(hp_ppn* p);
int hp_ppn_enqueue(hp_ppn* p, int n, const float* const dev_tensors[7], const int conf_shape[3], const int edge_shape[5], void* stream);
int hp_ppn_collect(hp_ppn* p, hp_human* out, int cap_per_frame, int* n_out);
/* Per frame of the last collected batch: 0 = assembled on the device (ppn_assemble_kernel); bits 4 / 8 / 16 = the device tail declined
 * the frame (more than 2048 skeleton fragments / 8192 hash entries / 2048 humans) and the same statements ran on the host; bits 1 / 2 = a
 * list of the extract kernel overflowed (HP_ERR_CAPACITY); -1 = HP_PPN_HOST_TAIL=1 (tests: every frame on the host). */
int hp_ppn_decode_flags(hp_ppn* p, int* flags, int n);

/* ---- hyperpose::parser::pifpaf (include/hyperpose/operator/parser/pifpaf.hpp:8-26, src/pifpaf.cpp,
 * src/pifpaf_decoder/openpifpaf_postprocessor.cpp).  GPU: PIF cell compaction, seed and CAF scoring with the
 * hi-res confidence map evaluated on demand (never materialised), and the decoder itself - seed-ordered greedy grow, occupancy,
 * soft-NMS, the 17 -> 18 key-point remap - as one wavefront per frame (pp_decode_kernel).  A frame the device decoder cannot finish
 * (capacity, or a score too close to a float rounding boundary to be libm-independent) is decoded by the host tail from the packed
 * lists; HP_PIFPAF_HOST_TAIL=1 sends every frame there. */
typedef struct hp_pifpaf hp_pifpaf;
int hp_pifpaf_create(hp_pifpaf** out, int net_h, int net_w, float thresh, int max_batch); /* pifpaf(int h, int w, float thresh = 0.1) */
void hp_pifpaf_destroy(hp_pifpaf* p);
/* pifpaf::process(paf, pif) (src/pifpaf.cpp:7 — the .cpp argument order): paf [n,19,9,fh,fw], pif [n,17,5,fh,fw]. */
int hp_pifpaf_process_batch(hp_pifpaf* p, int n, const float* paf, const float* pif, int fh, int fw, int on_device,
                            hp_human* out, int cap_per_frame, int* n_out);
/* Asynchronous halves: enqueue = the five kernels + the packed lists written into pinned host memory, on `stream` (NULL = the
 * parser's own) and the device decoder behind them, humans written into pinned memory; collect = wait, copy out, and the host tail
 * (worker pool) for the frames the device decoder declined. */
void* hp_pifpaf_stream(hp_pifpaf* p);
int hp_pifpaf_enqueue(hp_pifpaf* p, int n, const float* dev_paf, const float* dev_pif, int fh, int fw, void* stream);
int hp_pifpaf_collect(hp_pifpaf* p, hp_human* out, int cap_per_frame, int* n_out);
/* Per frame of the last collected batch: 0 = decoded on the device, -1 = host tail by configuration, > 0 = why the device decoder
 * handed the frame to the host tail (1 annotations > 256, 2 soft-NMS extent, 8 seeds, 16 frontier / more than 256 list entries inside
 * one search box, 32 rounding, 64 declined by the HP_PIFPAF_DECLINE_ODD test hook; 4 is no longer produced: it meant that the sort of
 * the annotation scores ran out of introsort depth, which the device now heap-sorts as libstdc++ does, and remains only as the guard
 * for a stack overflow that cannot happen). */
int hp_pifpaf_decode_flags(const hp_pifpaf* p, int* flags, int n);

/* ---- hyperpose::dnn engine: replaces dnn::tensorrt (include/hyperpose/operator/dnn/tensorrt.hpp:33-141,
 * src/tensorrt.cpp).  The network is a static list of layers over numbered tensors (tensor 0 = the input
 * image); weights are one fp32 blob in the layouts below.  TensorRT's UFF/ONNX parsing is replaced by the
 * built-in topology builders (hp_model_*) that restate hyperpose/Model/<arch>.py, and by hp_model_from_onnx
 * (SURVEY.md 8f-1).  Activations live in HBM as NHWC fp16 (fp32 accumulate on MFMA); network outputs are
 * fp32 NCHW, the layout of feature_map_t. */
enum { HP_OP_CONV = 1, HP_OP_DWCONV = 2, HP_OP_MAXPOOL = 3,
       HP_OP_UPSAMPLE = 4 }; /* integer up-scaling by `stride` (UpSampling2d of the MobilenetSmall backbone, hyperpose/Model/backbones.py:325,339; ONNX
                              * Resize / Upsample): kh = 0 nearest (source = floor(dst / scale)), kh = 1 bilinear with half-pixel centres
                              * (tf.image.resize / align_corners = False); cin == cout, no weights, no activation */
enum { HP_ACT_NONE = 0, HP_ACT_RELU = 1, HP_ACT_RELU6 = 2, HP_ACT_LEAKY = 3, HP_ACT_PRELU = 4, HP_ACT_SIGMOID = 5, HP_ACT_SOFTPLUS = 6 };

typedef struct hp_layer {
    int32_t op;              /* HP_OP_* */
    int32_t in, in_coff;     /* tensor read (0 = network input) and its first channel */
    int32_t res;             /* residual tensor (its channels [0, cout)) added in the epilogue, or -1.  HP_OP_CONV only: hp_engine_create refuses a
                              * residual on a depthwise / pooling / up-sampling layer (HP_ERR_INVALID) - their kernels have no such epilogue.  It also
                              * refuses a depthwise layer no kernel serves: PReLU / sigmoid / softplus, or (fp16 / int8 engines) stride 2 with dilation 2 */
    int32_t res_before_act;  /* 1: act(conv + res) (ResNet); 0: act(conv) + res (LW-OpenPose blocks) */
    int32_t out, out_coff;   /* tensor written and its first channel (concat by offset) */
    int32_t cin, cout;
    int32_t kh, kw, stride, dil; /* padding is TF "SAME" (out = ceil(in/stride), extra pad bottom/right) unless pad_explicit */
    int32_t act;             /* HP_ACT_* applied after bias (BatchNorm is folded into w/bias by the caller) */
    float act_param;         /* LeakyReLU slope */
    int64_t w_off;           /* float offset in the blob: CONV [cout][kh][kw][cin]; DWCONV [c][kh][kw] */
    int64_t b_off;           /* bias [cout], or -1 for zeros */
    int64_t alpha_off;       /* PReLU slopes [cout], or -1 */
    int32_t pad_explicit;    /* 1: pad[] = {top, left, bottom, right} as in an ONNX Conv / MaxPool `pads` attribute,
                              * out = floor((in + pad_before + pad_after - ((k-1)*dil+1)) / stride) + 1; 0: TF "SAME" */
    int32_t pad[4];
} hp_layer;

typedef struct hp_output_desc {
    char name[48];           /* outputs are returned sorted by name (src/tensorrt.cpp:405) */
    int32_t tensor, coff, channels; /* channel range of the fp16 tensor that feeds this output */
    int32_t act;             /* element-wise op while converting to fp32 NCHW (HP_ACT_NONE / SIGMOID / SOFTPLUS), all channels */
    /* optional transforms used by the PoseProposal / PifPaf heads (all zero = plain conversion): */
    int32_t shuffle;         /* 2: pixel_shuffle(x, 2) (hyperpose/Model/pifpaf/utils.py:371-379): C/4 channels, 2H x 2W */
    int32_t group;           /* > 0: output channels come in groups of `group` components with per-component ops: */
    uint32_t sigmoid_mask;   /*      bit k set -> sigmoid on component k   (pif conf, paf conf) */
    uint32_t softplus_mask;  /*      bit k set -> softplus on component k  (pif / paf scales)   */
    int32_t out_h, out_w;    /* crop of the (shuffled) map, 0 = keep (PifPaf: 2*25 = 50 -> 49) */
    float scale;             /* y = (op(v) + grid term) * scale; 0 means 1 (PoseProposal restore_coor, model.py:111-119) */
    int32_t grid;            /* 1: add the column index, 2: add the row index before scaling */
} hp_output_desc;

/* Arithmetic of the engine.  HP_DTYPE_F16: fp16 storage, fp16 MFMA products, fp32 accumulation - the fast path (data_type::kHALF).
 * HP_DTYPE_F32: fp32 storage and fp32 matrix-pipe arithmetic, one launch per layer - what data_type::kFLOAT, the reference's default,
 * promises: outputs agree with an fp32 evaluation of the graph to ~1e-5 relative (tests/test_engine_fp32_gpu.py).
 * HP_DTYPE_F32S ("split"): the HP_DTYPE_F32 engine - fp32 storage, fp32 accumulation, same launches - with the products of its dense
 * 1 x 1 / 3 x 3 stride-1 layers formed on the fp16 matrix pipe: x = hi + 2^-11 lo with hi, lo fp16, a b = hi hi + 2^-11 (hi lo + lo hi),
 * every partial product exact in the fp32 accumulator, ~2^-22 relative per product (csrc/conv32_direct.hip).  Opt-in; an activation beyond
 * fp16's range (|x| > 65504) makes the engine re-run the batch on the fp32 pipe and stay there (hp_engine_split_fallbacks counts).
 * HP_DTYPE_I8 (data_type::kINT8): post-training quantization in TensorRT's form on the HP_DTYPE_F16 engine's per-layer schedule (no fusions).
 * Every dense convolution that does not read the network input and whose geometry the int8 kernel covers (1 x 1 stride 1 | 2, 3 x 3 stride
 * 1 | 2 dilation 1 | 2, 7 x 7 stride 1) may run on the int8 matrix pipe: weights symmetric per output channel (s_w[c] = max |w| / 127,
 * q_w = clamp(rint(w / s_w[c]), -127, 127)), activations with one scale per layer input (q_x = clamp(rint(x * (1 / s_a)), -127, 127), computed
 * while the kernel stages its fp16 input), exact int32 sums, v = (float)acc * (s_a * s_w[c]) + bias[c], then the fp16 engine's epilogue.
 * Activations between layers stay fp16 NHWC.  The per-layer scale vector (hp_engine_int8_scales) says what runs where: > 0 int8 with that
 * s_a, 0 the layer's fp16 kernel, -1 eligible but not calibrated - an engine with a -1 entry does not infer (HP_ERR_STATE) until
 * hp_engine_calibrate_u8 (TensorRT's MinMax rule: s_a = max |x| / 127 over the calibration frames, x from the same engine in fp16) or
 * hp_engine_set_int8_scales (a calibration cache) fills it.  An engine with every scale 0 is bit-identical to the HP_DTYPE_F16 engine built
 * with HP_NO_FUSE=1. */
enum { HP_DTYPE_F16 = 0, HP_DTYPE_F32 = 1, HP_DTYPE_F32S = 2, HP_DTYPE_I8 = 3 };

typedef struct hp_engine_desc {
    int32_t in_w, in_h, max_batch;   /* tensorrt(..., cv::Size input_size, int max_batch_size = 8, ...) */
    double factor;                   /* tensorrt.hpp:49: every input element is multiplied by factor (default 1/255) */
    int32_t flip_rb;                 /* BGR -> RGB (default true) */
    float mean[3], inv_std[3];       /* in-graph input normalisation of VGG19 / PifPaf, applied after factor */
    const hp_layer* layers;
    int32_t n_layers;
    const hp_output_desc* outputs;
    int32_t n_outputs;
    const float* weights;            /* host fp32 blob */
    size_t n_weights;
    int32_t dtype;                   /* HP_DTYPE_F16 (0, the zero-initialised default), HP_DTYPE_F32, HP_DTYPE_F32S or HP_DTYPE_I8: the reference's data_type
                                      * argument (include/hyperpose/operator/dnn/tensorrt.hpp:14-21,48; src/tensorrt.cpp:327,353) */
    const float* int8_scales;        /* HP_DTYPE_I8: n_layers per-layer activation scales (see HP_DTYPE_I8; -1 = not calibrated), or NULL for an
                                      * uncalibrated engine; ignored by the other dtypes.  hp_engine_describe fills it (NULL for the other dtypes). */
} hp_engine_desc;

typedef struct hp_engine hp_engine;
int hp_engine_create(hp_engine** out, const hp_engine_desc* desc);
void hp_engine_destroy(hp_engine* e);
int hp_engine_max_batch(const hp_engine* e);                  /* tensorrt::max_batch_size() */
/* The description the engine was created from (topology, outputs, pre-processing, fp32 weights), as pointers INTO the engine, valid
 * while it lives: lets a stream (hp_pipeline_create_ex) replicate an engine that came from a file (ONNX, serialized) - the reference's
 * stream shares ONE engine between its stages (include/hyperpose/stream/stream.hpp:136), the GPU pipeline keeps one per batch in flight. */
int hp_engine_describe(const hp_engine* e, hp_engine_desc* out);
int hp_engine_input_size(const hp_engine* e, int* w, int* h); /* tensorrt::input_size() */

/* tensorrt::inference(std::vector<cv::Mat>) with network-sized frames (src/tensorrt.cpp:436-461): n u8 HWC BGR
 * frames [n,in_h,in_w,3]; the u8->f32 conversion of src/data.cpp:21-51 is fused into the first layer.
 * n > max_batch returns HP_ERR_CAPACITY (the reference throws std::logic_error, :439-443).  The call only
 * ENQUEUES on `stream` (NULL = the engine's own stream); outputs stay in device memory. */
int hp_engine_infer_u8(hp_engine* e, const uint8_t* hwc_bgr, int n, int on_device, void* stream);
/* tensorrt::inference(const std::vector<float>&, size_t) (src/tensorrt.cpp:364-434): n f32 NCHW frames, no
 * scaling / channel swap. */
int hp_engine_infer_f32(hp_engine* e, const float* nchw, int n, int on_device, void* stream);
int hp_engine_synchronize(hp_engine* e);
void* hp_engine_stream(hp_engine* e); /* hipStream_t of the engine */
int hp_engine_set_graph(hp_engine* e, int enable); /* replay the schedule from a captured hipGraph (default on) */
/* The captured graphs are cached per (frames of the call, input pointer, u8 / f32 entry, first frame): a host batch is keyed by the engine's
 * staging buffer, a device batch by the caller's pointer; with hp_engine_set_concurrency(2) a batch holds two entries, one per half.  The cache
 * holds at most HP_ENGINE_GRAPH_CACHE_BOUND entries.  A call whose graphs are cached costs its look-ups and the launches.  A call that needs a
 * capture that no longer fits empties the cache first: ONE hipDeviceSynchronize() (every stream of the device, the caller's included), then the
 * call's captures, and afterwards one capture for every other (frames, pointer) the caller comes back to.  A caller that cycles more device
 * buffers than the bound / 2 (two halves) or the bound pays that on every round; one that stays below never does.  Changing a setting that
 * changes the schedule (concurrency, flip ensemble, int8 scales, calibration) empties the cache in the same way; hp_engine_set_graph keeps it.
 * hp_engine_cached_graphs: the number of entries now. */
#define HP_ENGINE_GRAPH_CACHE_BOUND 64
int hp_engine_cached_graphs(const hp_engine* e);
/* parts = 2: every batch of >= 2 frames runs as two half-batches side by side, the second on an internal stream that forks from and joins the
 * call's stream (HP_DTYPE_F32 / F32S engines; an fp16 engine keeps one stream and hp_engine_concurrency() says so) - for a caller that keeps ONE batch in flight, as the reference's synchronous
 * tensorrt::inference does (src/tensorrt.cpp:364-434): the two halves fill each other's idle phases.  Outputs are bit-identical to parts = 1.
 * Callers that overlap several batches on several engines (hp_pipeline_*) keep 1. */
int hp_engine_set_concurrency(hp_engine* e, int parts);
int hp_engine_concurrency(const hp_engine* e);

/* Outputs, sorted by name.  shape[] receives the non-batch dims (C,H,W), dev the fp32 NCHW device buffer
 * [max_batch][C][H][W] of which the first n frames are valid after the last inference completed. */
int hp_engine_num_outputs(const hp_engine* e);
int hp_engine_output(const hp_engine* e, int i, const char** name, int shape[3], const float** dev);
/* Serialized engines: tensorrt::save (include/hyperpose/operator/dnn/tensorrt.hpp:121-123, src/tensorrt.cpp:463-471) and the
 * tensorrt_serialized constructor (include/hyperpose/utility/model.hpp:27-32, src/tensorrt.cpp:225-252).  The file carries the
 * topology, outputs, pre-processing and fp32 weights the engine was created from; max_batch <= 0 keeps the saved one. */
int hp_engine_save(const hp_engine* e, const char* path);
int hp_engine_load(hp_engine** out, const char* path, int max_batch);
int hp_engine_output_to_host(hp_engine* e, int i, int n, float* host); /* synchronises, then D2H */
/* Read back an internal fp16 NHWC tensor as fp32 NCHW [n][C][H][W] (layer-wise parity tests only). */
int hp_engine_debug_tensor(hp_engine* e, int tensor, int n, float* host, int shape[3]);
/* The tensor's whole buffer as it lies in HBM (write-footprint tests only): [max_batch][rows][W + 2P][cs] elements, halo, separator rows
 * and pad channels included, all max_batch images whatever the last batch was.  geom = { H, W, C, cs, P, rows per image (H + 2P; fp32
 * engines: made even when P > 0), bytes per element (2: fp16, also in HP_DTYPE_I8 engines, 4: fp32), max_batch }.  host == NULL: the
 * geometry only.  Synchronises the engine first.  Tensors of the activation arena are shown too (the buffer then holds its last tenant);
 * HP_ERR_STATE for a tensor that is never materialised (fused away, or only the fp32 network output), HP_ERR_INVALID for a bad id. */
int hp_engine_debug_raw_tensor(hp_engine* e, int tensor, void* host, size_t cap_bytes, int geom[8]);

/* Per-layer device time (ms, averaged over iters) measured with HIP events on the engine stream for batch n:
 * the numbers the roofline report is built from.  flops = 2*MACs of the layer for that batch. */
typedef struct hp_layer_time {
    int32_t layer, op, tile; /* tile = BM*1000+BN for MFMA convs, 0 otherwise */
    float ms;
    double flops, bytes;     /* algorithmic FLOPs and compulsory HBM bytes (inputs + weights + outputs once) */
} hp_layer_time;
int hp_engine_profile(hp_engine* e, int n, int iters, hp_layer_time* out, int cap, int* n_out);
/* Same table, but measured IN SEQUENCE: the whole schedule runs `iters` times in order and every launch records its own begin /
 * end timestamps (hipExtLaunchKernelGGL start / stop events: the numbers rocprofv3's kernel trace reports, no packets added
 * between the kernels), so every kernel sees the cache state it sees in a real inference.  The back-to-back form above
 * re-runs one layer with its weights warm in L2 and reads ~10-15 % faster for the weight-heavy 3x3 layers. */
int hp_engine_profile_sequence(hp_engine* e, int n, int iters, hp_layer_time* out, int cap, int* n_out);
/* Machine time per launch: step k of two engines of the same model launched alternately on their two streams (two instances of the
 * kernel share the GPU as two pipes' kernels do); ms = elapsed / (2 * iters).  tools/profile_layers.py --pair. */
int hp_engine_profile_pair(hp_engine* e, hp_engine* other, int n, int iters, hp_layer_time* out, int cap, int* n_out);

/* ---- built-in topologies (restating hyperpose/Model/<arch>.py) --------------------- */
typedef struct hp_model hp_model;
/* arch: "lw_openpose_mobilenet" (MobilenetDilated + LightWeightOpenPose, backbones.py:177-229,
 * openpose/model/lw_openpose.py), "lw_openpose_vggtiny" (backbones.py:343-391), "openpose_vgg19"
 * (backbones.py:447-509, openpose/model/openpose.py), ... see hp_model_archs(). */
int hp_model_build(hp_model** out, const char* arch, int in_w, int in_h);
void hp_model_destroy(hp_model* m);
const char* hp_model_archs(void);                       /* comma-separated list */
int hp_model_layers(const hp_model* m, const hp_layer** layers, int* n);
int hp_model_outputs(const hp_model* m, const hp_output_desc** outs, int* n);
size_t hp_model_num_weights(const hp_model* m);
int hp_model_preproc(const hp_model* m, float mean[3], float inv_std[3]);
double hp_model_flops_per_frame(const hp_model* m);     /* 2*MACs of all CONV/DWCONV layers */
/* Deterministic synthetic weights (there is no network to fetch the released models): He-normal conv
 * kernels from a counter-based generator keyed by (seed, layer, index), small biases, PReLU slopes 0.25. */
int hp_model_init_weights(const hp_model* m, uint64_t seed, float* blob, size_t n);
/* ONNX import: what nvonnxparser does for dnn::tensorrt(const onnx&, cv::Size, ...) (include/hyperpose/operator/dnn/tensorrt.hpp:53-62,
 * include/hyperpose/utility/model.hpp:23-25, src/tensorrt.cpp:162-223).  The file / buffer is a serialized ONNX ModelProto with ONE
 * input of 3 channels (N,3,H,W, 3,H,W, or N,H,W,3 followed by a Transpose); in_w x in_h is the caller's input size as in the reference
 * (0,0 = take the static size stored in the graph).  Supported operators and how they are lowered onto hp_layer: see the header of
 * hyperpose_amd/csrc/onnx_import.cpp; anything else returns HP_ERR_INVALID with the node and operator named in hp_last_error().
 * The model owns the imported weights: pass weights = NULL to hp_engine_create_from_model, or read them with hp_model_weights. */
int hp_model_from_onnx(hp_model** out, const void* data, size_t size, int in_w, int in_h);
int hp_model_from_onnx_file(hp_model** out, const char* path, int in_w, int in_h);
int hp_model_weights(const hp_model* m, const float** blob, size_t* n); /* blob = NULL for built-in topologies */
int hp_model_input_size(const hp_model* m, int* w, int* h);
/* Convenience: build an engine for a topology with blob weights (NULL = the model's own, imported models only). */
int hp_engine_create_from_model(hp_engine** out, const hp_model* m, int max_batch, double factor, int flip_rb,
                                const float* weights, size_t n_weights);
/* the same with the arithmetic chosen (HP_DTYPE_*); hp_engine_create_from_model is the HP_DTYPE_F16 form */
int hp_engine_create_from_model_dtype(hp_engine** out, const hp_model* m, int max_batch, double factor, int flip_rb,
                                      const float* weights, size_t n_weights, int dtype);
int hp_engine_dtype(const hp_engine* e); /* HP_DTYPE_* of an engine (serialized engines carry theirs) */
/* HP_DTYPE_I8 engines (HP_ERR_STATE for the other dtypes).  Calibration: n network-sized u8 HWC BGR frames (any n: the engine runs them in
 * max_batch chunks, synchronously, every layer in fp16); every eligible layer's scale becomes max |x| / 127 of its input channels over the valid
 * pixels of all frames (1 where that maximum is 0) - independent of frame order and chunking.  Setting scales imports a calibration cache:
 * n == the layer count, every value finite and >= 0, > 0 only on eligible layers (HP_ERR_INVALID otherwise).  Both drop the captured graphs. */
int hp_engine_calibrate_u8(hp_engine* e, const uint8_t* hwc_bgr, int n, int on_device);
int hp_engine_int8_scales(const hp_engine* e, float* scales, int n);
int hp_engine_set_int8_scales(hp_engine* e, const float* scales, int n);
/* HP_DTYPE_F32S engines: how many times the engine left the split kernels for the fp32 pipe because an activation did not fit fp16's
 * range (0 or 1: it does not go back); 0 for the other types */
int hp_engine_split_fallbacks(const hp_engine* e);
/* HBM the engine holds for its max_batch, in bytes: bytes[0] activation tensors (with their zero halos), bytes[1] packed weights in every
 * form its kernels read (fragment orders, the Winograd U matrices of an HP_DTYPE_F32 engine ...), bytes[2] the fp32 NCHW network outputs */
int hp_engine_device_bytes(const hp_engine* e, uint64_t bytes[3]);
/* The activation arena of an HP_DTYPE_F32 / F32S engine (tensors of one geometry take turns in the fewest buffers their lifetimes in the schedule
 * allow; HP_NO_ARENA=1 at creation: one allocation per tensor): info = { buffers, tensors living in them, bytes the same tensors would take with one
 * allocation each }.  All zero for engines without an arena. */
int hp_engine_arena_info(const hp_engine* e, uint64_t info[3]);
/* Diagnostic (HP_FIRST_CONV_VERIFY=1 at launch time): the fp32 first-layer kernel re-reads its staged weights and input patch from LDS after computing and
 * compares them with global memory; out = { patch words that differed, weight words that differed, blocks checked, 0 } since the last reset. */
int hp_debug_first_conv_verify(unsigned out[4], int reset);

/* ---- flip ensemble: the network runs on every frame and on its left-right flip; the flipped maps are flipped back - left and right channels
 * swapped, the x component of the part-affinity fields negated - and the two sets of maps are averaged on the device, before parsing
 * (hyperpose_amd/csrc/flip_ensemble.hip; the definition is stated once in csrc/flip_ensemble.hpp and DESIGN.md 1.1 "Flip ensemble").  Off by
 * default; while off, nothing here is launched.
 *
 * hp_hflip_u8c3: n packed u8 HWC frames (rows of w * 3 bytes, frames w * h * 3 bytes apart), dst[i][y][x][c] = src[i][y][w-1-x][c]; src and dst
 * must not overlap (dst == src + n * w * h * 3 is the expected use); any w >= 1.  The device call only enqueues.
 *
 * hp_flip_merge: dev_maps holds at least 2n maps [C][H][W], contiguous, fp32: n frames, then the maps of their flips.  For f < n, in place,
 *     a = maps[f][c][y][x]   b = maps[n+f][perm[c]][y][W-1-x]   maps[f][c][y][x] = sign[c] > 0 ? 0.5f * (a + b) : 0.5f * (a - b)
 * Maps n .. 2n-1 and everything behind them are not written.  perm and sign are HOST tables of C entries, read before the call returns (they go
 * to the kernel by value).  HP_ERR_INVALID, with a message that names the argument, and nothing launched: C outside 1 .. 256, a perm[c] outside
 * [0, C), a sign[c] other than -1 / +1, n, H or W below 1.  Because a + b == b + a and 0.5f * (a - b) == -(0.5f * (b - a)) bit for bit, the
 * ensemble E of a frame-invariant network is exactly equivariant when perm is an involution and sign[perm[c]] == sign[c]:
 *     E(flip(x))[perm[c]](W-1-p) * sign[c] == E(x)[c](p)
 * in every bit but the sign of a zero: where a == b a negated channel holds +0 on one side and -0 on the other.
 * The *_host twins are the same statements in plain C++ (no device), same evaluation order.
 *
 * hp_flip_tables_coco (host only): the tables of a COCO PAF network, derived from the part pairs and PAF channel pairs the PAF parser reads:
 * parts swap 2-5, 3-6, 4-7, 8-11, 9-12, 10-13, 14-15, 16-17 (0, 1 and a background channel 18 stay: conf_channels is 18 or 19, conf_perm has
 * that many entries, the confidence signs are all +1); the mirror of limb k is the limb of the mirrored parts, paf_perm maps its x / y channel to
 * the mirror's x / y channel and paf_sign is -1 on the x channels (the even ones). */
int hp_hflip_u8c3(const uint8_t* dev_src, uint8_t* dev_dst, int w, int h, int n, void* stream);
int hp_hflip_u8c3_host(const uint8_t* src, uint8_t* dst, int w, int h, int n);
int hp_flip_merge(float* dev_maps, int n, int C, int H, int W, const int32_t* perm, const int8_t* sign /* host tables */, void* stream);
int hp_flip_merge_host(float* maps, int n, int C, int H, int W, const int32_t* perm, const int8_t* sign);
int hp_flip_tables_coco(int conf_channels /* 18 or 19 */, int32_t* conf_perm, int32_t paf_perm[38], int8_t paf_sign[38]);
/* The engine's side.  While the ensemble is on, hp_engine_infer_u8(e, frames, n, ..) takes 1 <= n with 2n <= max_batch (HP_ERR_CAPACITY beyond,
 * the message gives both numbers; hp_engine_max_batch is unchanged): the engine copies the n frames into a buffer of its own, writes their flips
 * behind them (hp_hflip_u8c3), runs its unchanged schedule on the 2n frames and hp_flip_merge on every output - on the call's stream, inside the
 * captured graph when graphs are on (hp_engine_set_concurrency(2): flip and merge are launched around the two half-batch graphs, the merge behind
 * the join).  Afterwards the first n frames of every output are the ensemble (hp_engine_output_to_host(.., n, ..)).  hp_engine_infer_f32 returns
 * HP_ERR_STATE; hp_engine_calibrate_u8 and hp_engine_profile* run the plain schedule.  The setters copy the tables, synchronise and drop the
 * captured graphs; every engine output must be listed exactly once (HP_ERR_INVALID otherwise); n_outs == 0 turns the ensemble off, which restores
 * the engine exactly.  The COCO form needs exactly two outputs (sorted by name: conf with 18 or 19 channels, paf with 38) of equal H x W
 * (HP_ERR_INVALID, the message says what it found).  Another skeleton: pass its own tables. */
typedef struct hp_flip_output {
    int32_t output;           /* index as in hp_engine_output */
    const int32_t* perm;
    const int8_t* sign;       /* that output's C entries each */
} hp_flip_output;
int hp_engine_set_flip_ensemble(hp_engine* e, const hp_flip_output* outs, int n_outs); /* n_outs == 0: off */
int hp_engine_set_flip_ensemble_coco(hp_engine* e, int enable);
int hp_engine_flip_ensemble(const hp_engine* e); /* 0 / 1 */

/* ---- scale ensemble: the network runs on every frame and on K - 1 shrunken copies of it; the maps of every copy are resampled back to the map
 * grid and the K sets of maps are averaged on the device, before parsing (hyperpose_amd/csrc/scale_ensemble.hip; the definition is stated once in
 * csrc/scale_ensemble.hpp and DESIGN.md 1.1 "Scale ensemble").  Scales above 1 are tiles' job ("regions and tiles" above).
 *
 * The caller gives K - 1 extra scales (1 <= K - 1 <= 3), each a float in (0, 1]; scale 0 is the frame as it is.  For a network with input
 * in_w x in_h and maps of W x H cells (in_w % W == 0, in_h % H == 0), scale s keeps the map region mw = max(1, (int)floor((double)s * W + 0.5)),
 * mh likewise, and shrinks the slot's content to iw = mw * (in_w / W), ih = mh * (in_h / H): the scale is rounded to whole map cells.
 *
 * hp_scale_stage_u8c3: n packed network-sized u8 HWC slots (w x h) -> the n_scales * n slots of the extra scales, scale-major: slot (k, i) at index
 * (k - 1) * n + i of dst is slot i resized into its top-left iw_k x ih_k - byte for byte what hp_resize_u8c3 of the slot into a tight iw_k x ih_k
 * image gives - and the rest filled with (b, g, r), each 0 .. 255.  src and dst must not overlap.  One launch; the device call only enqueues.
 * HP_ERR_INVALID (the message names the sizes or the argument): w or h not a multiple of map_w / map_h, n_scales outside 1 .. 3, a scale outside
 * (0, 1] or not finite, n * n_scales above 65535.
 *
 * hp_scale_tables (host only): for each of the W destination columns the four source columns idx[x][0..3] and weights wgt[x][0..3] of OpenCV's
 * bicubic (A = -0.75) from a valid region of mw columns (1 <= mw <= W), fp32:
 *     fx = (float)((x + 0.5) * ((double)mw / W) - 0.5); sx = (int)floorf(fx); fx -= sx
 *     c0 = ((A*(fx+1) - 5*A)*(fx+1) + 8*A)*(fx+1) - 4*A;  c1 = ((A+2)*fx - (A+3))*fx*fx + 1
 *     c2 = ((A+2)*(1-fx) - (A+3))*(1-fx)*(1-fx) + 1;      c3 = 1.f - c0 - c1 - c2
 * columns sx-1 .. sx+2, each clamped to [0, mw-1].  At mw == W the weights are exactly (0, 1, 0, 0) on column x.  The same function serves rows.
 * Parity with OpenCV itself is unpinned (no OpenCV to compare with; tests/scale_ref.py restates the coefficients), as for the front-end resize.
 *
 * hp_scale_merge: dev_maps holds K * n maps [C][H][W], contiguous, fp32, scale-major (the n frames, then the n frames at scales[0], ...); scales has
 * K - 1 HOST entries.  For f < n, in place, with no fused operation:
 *     acc = maps[f][c][y][x]
 *     for k = 1 .. K-1:  row_r = ((wx0*p[r][0] + wx1*p[r][1]) + wx2*p[r][2]) + wx3*p[r][3]  (r = 0 .. 3; p = maps[k*n + f][c] at the tables' rows
 *                        and columns: only the valid mh_k x mw_k region is read);  acc = acc + (((wy0*row_0 + wy1*row_1) + wy2*row_2) + wy3*row_3)
 *     maps[f][c][y][x] = acc * (1.0f / (float)K)
 * Maps n .. K*n-1 and everything behind them are not written.  The tables are too large for kernel arguments: the stand-alone call uploads them
 * the first time it sees a (device, H, W, scales) and keeps that copy for the life of the process, never writing it again (so that first call
 * synchronises the device and cannot be captured in a graph; later ones only enqueue).  HP_ERR_INVALID, with a message that names the argument,
 * and nothing launched: K outside 2 .. 4, a scale outside (0, 1] or not finite, C outside 1 .. 256, H or W below 1, H * W over 2^31 - 1, n outside
 * 1 .. 65535.  The *_host twins are the same statements in plain C++ (no device), same evaluation order and the same resize_pixel. */
int hp_scale_stage_u8c3(const uint8_t* dev_src, uint8_t* dev_dst, int w, int h, int n, int map_w, int map_h, const float* scales, int n_scales, int b,
                        int g, int r, void* stream);
int hp_scale_stage_u8c3_host(const uint8_t* src, uint8_t* dst, int w, int h, int n, int map_w, int map_h, const float* scales, int n_scales, int b,
                             int g, int r);
int hp_scale_tables(int W, int mw, int32_t idx[][4], float wgt[][4]);
int hp_scale_merge(float* dev_maps, int n, int K, int C, int H, int W, const float* scales /* K - 1, host */, void* stream);
int hp_scale_merge_host(float* maps, int n, int K, int C, int H, int W, const float* scales);
/* The engine's side.  While the ensemble is on, hp_engine_infer_u8(e, frames, n, ..) takes 1 <= n with K * n <= max_batch - 2 * K * n with the flip
 * ensemble on as well - (HP_ERR_CAPACITY beyond, the message gives all the numbers; hp_engine_max_batch is unchanged): the engine copies the n
 * frames into its staging buffer (the flip ensemble's), writes their shrunken copies behind them (hp_scale_stage_u8c3), with the flip ensemble the
 * flips of all K n slots behind those (hp_hflip_u8c3), runs its unchanged schedule, hp_flip_merge over the K n slots if the flip ensemble is on, and
 * the scale merge of the n frames on every output - on the call's stream, inside the captured graph when graphs are on (with two half-batch graphs:
 * around the fork and the join).  Afterwards the first n frames of every output are the ensemble.  hp_engine_infer_f32 returns HP_ERR_STATE;
 * hp_engine_calibrate_u8 and hp_engine_profile* run the plain schedule.  The setter checks, computes and uploads the tables, synchronises and drops
 * the captured graphs; every output must have the same W x H with in_w % W == 0 and in_h % H == 0 and 1 .. 256 channels (HP_ERR_INVALID, the
 * message names the sizes); (b, g, r) fills the shrunken slots (each 0 .. 255; the reference pads with 0).  n_scales == 0 turns the ensemble off,
 * which restores the engine exactly.  The COCO form checks two outputs of 18 or 19 and of 38 channels of equal size, as its flip twin does, and
 * fills with 0.  hp_engine_scale_ensemble returns K, 1 while off.  No perm and no sign: confidences and unit-vector fields do not change under
 * scaling (PifPaf's and PoseProposal's outputs do: PAF networks only). */
int hp_engine_set_scale_ensemble(hp_engine* e, const float* scales, int n_scales, int b, int g, int r); /* n_scales == 0: off */
int hp_engine_set_scale_ensemble_coco(hp_engine* e, const float* scales, int n_scales);
int hp_engine_scale_ensemble(const hp_engine* e); /* K, 1 while off */

/* ---- hyperpose::stream on the GPU (reference include/hyperpose/stream/stream.hpp:119-390, src/stream.cpp:60-147): host frames of
 * any size in, humans out, in submission order.  Each submit copies one batch (<= max_batch frames, 8-bit BGR HWC, packed rows) to
 * the device and enqueues resize (keep_ratio = 0: cv::resize; 1: non_scaling_resize + resume_ratio on the way out) -> conv stack ->
 * PAF parser on the stream of the next free engine+parser pair; `n_pipes` batches can be in flight.  Frames in pinned memory
 * (hp_malloc_host) are copied from where they lie, others through a pinned staging buffer.  The network must have the two PAF
 * outputs (conf, paf).  max_frame_bytes bounds width*height*3 of a submitted frame. */
typedef struct hp_pipeline hp_pipeline;
/* which hyperpose::parser the pipeline ends in, with that parser's constructor arguments:
 *   HP_PARSER_PAF     thresh = {conf_thresh, paf_thresh}, res_w / res_h = resolution_size (-1 = default)     paf.hpp:27
 *   HP_PARSER_PPN     thresh = {point_thresh, limb_thresh, nms_thresh}; net_resolution = the engine's input size   proposal_network.hpp:26
 *   HP_PARSER_PIFPAF  thresh = {thresh}; (h, w) = the engine's input size                                    pifpaf.hpp:10 */
enum { HP_PARSER_PAF = 0, HP_PARSER_PPN = 1, HP_PARSER_PIFPAF = 2 };
typedef struct hp_parser_desc {
    int32_t kind;
    float thresh[3];
    int32_t res_w, res_h;
} hp_parser_desc;
int hp_pipeline_create_ex(hp_pipeline** out, const hp_engine_desc* desc, const hp_parser_desc* parser, int n_pipes, int keep_ratio,
                          size_t max_frame_bytes);
/* the PAF form of hp_pipeline_create_ex */
int hp_pipeline_create(hp_pipeline** out, const hp_engine_desc* desc, int n_pipes, int keep_ratio, float conf_thresh,
                       float paf_thresh, size_t max_frame_bytes);
void hp_pipeline_destroy(hp_pipeline* p);
/* HP_ERR_STATE when all pipes are busy (collect first) */
int hp_pipeline_submit(hp_pipeline* p, const uint8_t* const* frames, const int* widths, const int* heights, int n);
/* The same for YUV 4:2:0 frames (format = HP_YUV_NV12 / HP_YUV_I420): every frame is ONE contiguous, tightly packed buffer of
 * width*height*3/2 bytes (Y plane, then the UV plane or the U and V planes), width and height even.  One H2D copy of the 1.5-byte form per
 * frame, then the fused conversion + resize writes the network's slot (network-sized frames get the conversion alone).  max_frame_bytes
 * bounds width*height*3/2 here.  BGR and YUV submits may alternate on one pipeline; hp_pipeline_collect does not tell them apart. */
int hp_pipeline_submit_yuv(hp_pipeline* p, int format, const uint8_t* const* frames, const int* widths, const int* heights, int n);
/* The same for frames described by hp_yuv_image (any layout, matrix and range; the frames of one batch may differ in all of them and in
 * size).  on_device == 0: the planes are HOST pointers; each frame's planes are packed without row padding and go up as ONE copy of
 * hp_yuv_packed_bytes() bytes (straight from where they lie if the frame is one contiguous pinned buffer), max_frame_bytes bounds that
 * number (HP_ERR_CAPACITY).  on_device != 0: the planes are DEVICE pointers on the pipeline's device and nothing is copied - the fused
 * kernel reads the surface where it lies; the surfaces must be complete when this call is made (the kernels run on the pipeline's own
 * stream and wait for nobody) and must not be written until that batch has been collected; max_frame_bytes does not apply.  Host planes
 * are re-packed byte by byte, so the even-address / even-stride rule of the 16-bit formats holds for device planes only. */
int hp_pipeline_submit_yuv_images(hp_pipeline* p, const hp_yuv_image* frames, int n, int on_device);
/* The same for packed RGB and grey frames ("packed RGB and grey frames" above; the frames of one batch may differ in layout and size).
 * on_device == 0: `data` is a HOST pointer; each frame goes up ONCE in its own form, hp_rgb_packed_bytes() bytes - from where it lies when it is
 * tight and pinned, otherwise row by row through the pipe's staging - and max_frame_bytes bounds that number (HP_ERR_CAPACITY; the message names
 * layout, size and bytes).  on_device != 0: `data` is a DEVICE pointer and nothing is copied; the rules of device planes above hold (complete at the
 * call, not written until the batch is collected, max_frame_bytes does not apply) and so does the multiple-of-4 rule of the 4-byte layouts.  Then ONE
 * hp_resize_rgb / hp_resize_rois_rgb per frame: tiling (alignment 1 x 1), orientation and both ensembles work as for every other feed.  These are
 * 8-bit SDR frames: a tone-map set on the pipeline does not apply to them.  RGB, YUV and BGR submits may alternate with several batches in flight. */
int hp_pipeline_submit_rgb_images(hp_pipeline* p, const hp_rgb_image* frames, int n, int on_device);
/* waits for the OLDEST batch in flight; out[i * cap_per_frame + j], n_out[i] for i < *n_frames */
int hp_pipeline_collect(hp_pipeline* p, hp_human* out, int cap_per_frame, int* n_out, int* n_frames);
int hp_pipeline_in_flight(const hp_pipeline* p);
/* Tiled mode ("regions and tiles" above); t == NULL turns it off (the default), HP_ERR_STATE while batches are in flight, HP_ERR_CAPACITY when
 * R = cols * rows + with_full exceeds max_batch.  With tiling on, every frame of hp_pipeline_submit and hp_pipeline_submit_yuv_images (host or
 * device planes) becomes its R regions - planned for the frame's own size and its layout's alignment - in R consecutive slots of the batch,
 * written by ONE hp_resize_rois_* call per frame; a submit carries at most max_batch / R frames (HP_ERR_CAPACITY beyond that) and
 * hp_pipeline_submit_yuv returns HP_ERR_STATE.  hp_pipeline_collect parses all slots and, per frame, applies hp_resume_ratio per region (when the
 * aspect ratio is kept), hp_humans_to_frame and hp_humans_merge(min_common, tol): *n_frames counts frames and the humans are in the frame's
 * normalised coordinates, ready for hp_overlay_draw_*.  A frame of one region (1 x 1 tiles, no whole frame) has nothing to merge and keeps the
 * parser's order: it is returned exactly as with tiling off.  Every parser kind works: the tail is shared. */
int hp_pipeline_set_tiling(hp_pipeline* p, const hp_tiling* t);
/* HDR input ("HDR video in" above); d == NULL turns it off (the default), HP_ERR_STATE while batches are in flight.  While set, every P010 / I010 frame
 * of hp_pipeline_submit_yuv_images - host or device planes, tiled or not - goes through hp_resize_yuv_hdr / hp_letterbox_yuv_hdr / hp_resize_rois_yuv_hdr
 * with the tables of d; 8-bit frames of the same batch take the SDR path unchanged.  The pipeline owns its hp_tonemap. */
int hp_pipeline_set_tonemap(hp_pipeline* p, const hp_hdr_desc* d);
/* Upright input ("upright input" above); orientation 0 turns it off (the default), HP_ERR_STATE while batches are in flight, HP_ERR_INVALID outside
 * 0 .. 7.  While a non-zero orientation is set, every frame of hp_pipeline_submit and hp_pipeline_submit_yuv_images - host or device planes, tiled or
 * not, tone-mapped or not - is a STORED frame and goes through hp_resize_oriented_* / hp_resize_rois_oriented_*; tiles are planned on (uw, uh) with the
 * alignment pair swapped for odd q; hp_pipeline_collect returns humans normalised to the UPRIGHT frame (hp_resume_ratio and the tile merge use
 * (uw, uh); hp_humans_orient(.., to_stored = 1) takes them to the stored frame for hp_overlay_draw_*).  hp_pipeline_submit_yuv returns HP_ERR_STATE
 * while a non-zero orientation is set, as it does in tiled mode. */
int hp_pipeline_set_orientation(hp_pipeline* p, int orientation);
/* Flip ensemble ("flip ensemble" above): enable != 0 turns hp_engine_set_flip_ensemble_coco on for every pipe's engine, 0 turns it off (the default).
 * HP_ERR_STATE while batches are in flight; HP_ERR_INVALID for a pipeline whose parser is not HP_PARSER_PAF (the message names the kind).  While on,
 * a submit carries at most max_batch / 2 frames - tiled, max_batch / (2R) frames, and 2R <= max_batch is required by whichever of this call and
 * hp_pipeline_set_tiling comes second (HP_ERR_CAPACITY).  The flip is taken of the NETWORK-SIZED slot - after resize, letterbox, colour conversion,
 * tone-map, orientation and tile cut - so the letterbox padding stays where the maps expect it; every submit call works unchanged, the parser runs on
 * the merged maps and hp_pipeline_collect is unchanged. */
int hp_pipeline_set_flip_ensemble(hp_pipeline* p, int enable);
/* Scale ensemble ("scale ensemble" above): n_scales extra scales turn hp_engine_set_scale_ensemble_coco on for every pipe's engine, n_scales == 0 turns
 * it off (the default).  HP_ERR_STATE while batches are in flight; HP_ERR_INVALID for a pipeline whose parser is not HP_PARSER_PAF (the message names
 * the kind).  While on, a submit carries at most max_batch / (K * (flip ? 2 : 1)) frames - tiled, R times fewer, and R * K * (flip ? 2 : 1) <= max_batch
 * is required by whichever of this call, hp_pipeline_set_flip_ensemble and hp_pipeline_set_tiling comes last (HP_ERR_CAPACITY).  A refused call
 * leaves every pipe as it was.  The scale is taken of the NETWORK-SIZED slot, as the flip is; every submit call works unchanged. */
int hp_pipeline_set_scale_ensemble(hp_pipeline* p, const float* scales, int n_scales);

#ifdef __cplusplus
}
#endif
#endif /* HP_HIP_H */
