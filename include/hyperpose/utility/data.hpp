// hyperpose::feature_map_t / internal_t — reference include/hyperpose/utility/data.hpp:17-67.
// A feature_map_t owns a HOST copy (API compatibility with the reference, src/tensorrt.cpp:423-428).  The
// MI355X fast path keeps feature maps in HBM (dnn::tensorrt::inference_device + parser::paf::process_device).
#pragma once
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <ostream>
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hp_hip.h"
#include "human.hpp"

namespace hyperpose {

/// Addition: tiled inference (include/hp_hip.h, "regions and tiles").  A frame much larger than the network's input is cut into cols x rows
/// tiles that share at least `overlap` pixels (plus, with_full, the whole frame as region 0), every region is inferred at the network's
/// size, and the humans are mapped back to the frame (to_frame) and merged (merge_humans, utility/human.hpp).  min_common / tol: two
/// detections from different regions are one person when at least min_common joints are present in both and their mean distance is
/// at most tol times the larger one's extent; the defaults are HP_TILING_DEFAULT_*.
struct tiling {
    int cols = 1, rows = 1;
    int overlap_x = 0, overlap_y = 0;
    bool with_full = false;
    int min_common = HP_TILING_DEFAULT_MIN_COMMON;
    double tol = HP_TILING_DEFAULT_TOL;
    int regions() const { return cols * rows + (with_full ? 1 : 0); }
    hp_tiling c_form() const { return hp_tiling{ cols, rows, overlap_x, overlap_y, with_full ? 1 : 0, min_common, tol }; }
};

/// Addition: HDR input (include/hp_hip.h, "HDR video in").  The description of a stream of PQ (HDR10) or HLG 10-bit frames - P010 / I010 yuv_frames -
/// that dnn::tensorrt::set_tonemap, the stream's set_tonemap and draw_humans take: which transfer function the code values follow, whether the
/// BT.2020 primaries are converted to BT.709, and the tone curve's two parameters (the defaults are HP_HDR_DEFAULT_*: BT.2408 reference white, a
/// 1000 cd/m2 grade).  The tone curve and the HLG system gamma are applied per channel, an approximation the header states.
struct hdr {
    int transfer = HP_TRC_PQ; // HP_TRC_PQ or HP_TRC_HLG
    bool to_bt709 = true;
    float peak_nits = HP_HDR_DEFAULT_PEAK, white_nits = HP_HDR_DEFAULT_WHITE;
    hp_hdr_desc c_form() const { return hp_hdr_desc{ transfer, to_bt709 ? 1 : 0, peak_nits, white_nits }; }
};

/// Addition: upright input (include/hp_hip.h, "upright input").  How a frame is STORED relative to the upright picture: `quarter_turns` clockwise
/// quarter turns bring it upright (0 .. 3 = 0, 90, 180, 270 degrees - a container's `rotate` tag), after `mirrored` (left-right, first) is undone.
/// What dnn::tensorrt::set_orientation, the stream's set_orientation, to_stored / to_upright and draw_humans take.
struct orientation {
    int quarter_turns = 0;
    bool mirrored = false;
    int code() const { return (quarter_turns & 3) + (mirrored ? 4 : 0); } // HP_ORIENT_*
    static orientation from_code(int code) { return orientation{ code & 3, (code & 4) != 0 }; }
    /// EXIF orientation 1 .. 8; std::invalid_argument otherwise
    static orientation from_exif(int exif)
    {
        const int c = hp_orientation_from_exif(exif);
        if (c < 0)
            throw std::invalid_argument(hp_last_error());
        return from_code(c);
    }
    bool upright() const { return code() == HP_ORIENT_NONE; }
};

/// hp_oriented_size: the upright size of a frame stored as `stored`
inline cv::Size oriented_size(cv::Size stored, const orientation& o)
{
    int w = 0, h = 0;
    if (hp_oriented_size(o.code(), stored.width, stored.height, &w, &h) != HP_OK)
        throw std::invalid_argument(hp_last_error());
    return cv::Size(w, h);
}

/// hp_tile_plan: the regions of a `size` frame, the whole frame first when t.with_full, then the tiles row-major.  `yuv_format`: the
/// HP_YUV_* layout whose chroma alignment the tiles keep (-1: none, a BGR frame).  Throws std::invalid_argument on a plan the rules refuse.
/// With an orientation, `size` is the UPRIGHT size (oriented_size) and the tiles keep the alignment of their STORED rectangles: behind a quarter
/// turn the pair is swapped.
inline std::vector<cv::Rect> plan_tiles(cv::Size size, const tiling& t, int yuv_format = -1, const orientation& o = orientation{})
{
    int ax = 1, ay = 1;
    if (yuv_format >= 0 && hp_yuv_roi_alignment(yuv_format, &ax, &ay) != HP_OK)
        throw std::invalid_argument(hp_last_error());
    if (o.quarter_turns & 1)
        std::swap(ax, ay);
    const hp_tiling c = t.c_form();
    hp_roi out[64];
    const int n = hp_tile_plan(&c, size.width, size.height, ax, ay, out, 64);
    if (n < 0)
        throw std::invalid_argument(hp_last_error());
    std::vector<cv::Rect> r;
    for (int i = 0; i < n; ++i)
        r.emplace_back(out[i].x, out[i].y, out[i].w, out[i].h);
    return r;
}

namespace detail {
    // The output tensors of ONE dnn::tensorrt::inference call while they still lie in the engine's device buffers.  The reference copies
    // every tensor of every image to the host before it returns (src/tensorrt.cpp:423-428) and the parser copies nothing back; here the
    // maps a call returns are views of this record: a parser mirror that is handed such a map reads the batch straight from HBM (and
    // parses ALL its frames in one launch the first time one of them is asked for), and the HOST copy the reference's feature_map_t
    // promises is made when somebody looks at it - view<T>() - or, at the latest, just before the engine overwrites the buffers (its
    // next inference call, or its destruction).  Semantics are the reference's; the 4.5 MB D2H + H2D round trip per LW-OpenPose batch
    // happens only for callers that really read the maps.
    struct device_batch {
        hp_engine* engine = nullptr;
        std::shared_ptr<std::atomic<uint64_t>> live; // the engine's call counter: == gen while the device buffers still hold this batch
        uint64_t gen = 0;
        int n = 0;
        struct out {
            std::string name;
            std::vector<int> shape; // {C, H, W}
            const float* dev = nullptr; // [n][C][H][W]
            size_t per = 0;         // floats per frame
        };
        std::vector<out> outs;
        std::vector<std::unique_ptr<char[]>> host; // per output, [n][per] floats, once materialised
        std::mutex m;
        bool device_valid() const { return live && live->load() == gen; }
        // the host copy of output i (made on first use, while the device buffers are valid; the engine calls it for every output before it
        // re-uses them)
        const char* host_of(int i)
        {
            std::lock_guard<std::mutex> lk(m);
            if (host.empty())
                host.resize(outs.size());
            if (!host[i]) {
                if (!device_valid())
                    throw std::logic_error("hyperpose: feature map outlived its engine's buffers without a host copy (engine bug)");
                std::unique_ptr<char[]> h{ new char[outs[i].per * n * sizeof(float)] };
                if (hp_engine_output_to_host(engine, i, n, reinterpret_cast<float*>(h.get())) != HP_OK)
                    throw std::runtime_error(hp_last_error());
                host[i] = std::move(h);
            }
            return host[i].get();
        }
        void materialize()
        {
            for (size_t i = 0; i < outs.size(); ++i)
                (void)host_of((int)i);
        }
    };
} // namespace detail

struct feature_map_t {
public:
    feature_map_t(std::string name, std::unique_ptr<char[]>&& tensor, std::vector<int> shape)
        : m_name(std::move(name)), m_data(std::move(tensor)), m_shape(std::move(shape)) {}
    /// (this library's engine: output `out` of frame `frame` of a batch that still lives on the device)
    feature_map_t(std::shared_ptr<detail::device_batch> batch, int out, int frame)
        : m_name(batch->outs[out].name), m_shape(batch->outs[out].shape), m_batch(std::move(batch)), m_out(out), m_frame(frame) {}
    friend std::ostream& operator<<(std::ostream& out, const feature_map_t& map)
    {
        out << map.m_name << ":[";
        for (auto& s : map.m_shape)
            out << s << ", ";
        return out << ']';
    }
    inline const std::string& name() const { return m_name; }
    inline const std::vector<int>& shape() const { return m_shape; }
    template <typename T>
    inline const T* view() const
    {
        if (m_batch)
            return reinterpret_cast<const T*>(m_batch->host_of(m_out) + (size_t)m_frame * m_batch->outs[m_out].per * sizeof(float));
        return reinterpret_cast<T*>(m_data.get());
    }
    // ---- additions: where the tensor lies on the device, if it still does (nullptr otherwise)
    inline const detail::device_batch* device_batch() const { return m_batch && m_batch->device_valid() ? m_batch.get() : nullptr; }
    inline const std::shared_ptr<detail::device_batch>& batch_handle() const { return m_batch; }
    inline int batch_output() const { return m_out; }
    inline int batch_frame() const { return m_frame; }

private:
    std::string m_name;
    std::unique_ptr<char[]> m_data;
    std::vector<int> m_shape;
    std::shared_ptr<detail::device_batch> m_batch;
    int m_out = 0, m_frame = 0;
};

using internal_t = std::vector<feature_map_t>;

/// Addition: one video frame as a decoder delivers it - YUV 4:2:0, 8 bits per sample, in HOST memory, planes addressed by their own
/// pointers and row strides in bytes (decoder surfaces with padded pitch work; no OpenCV needed).  `format` is HP_YUV_NV12 (`u` = the
/// plane of interleaved (U, V) pairs, `v` unused) or HP_YUV_I420 (`u`, `v` = two planes of height/2 rows of width/2 bytes).  width and
/// height must be even.  dnn::tensorrt::inference / calibrate take a vector of these next to their cv::Mat forms; the frame goes to the
/// device in its 1.5-byte form and is converted (cv::cvtColor COLOR_YUV2BGR_NV12 / _I420 arithmetic) inside the resize kernel.
struct yuv420_frame {
    int format = HP_YUV_NV12;
    const uint8_t* y = nullptr;
    const uint8_t* u = nullptr;
    const uint8_t* v = nullptr;
    int y_stride = 0, uv_stride = 0;
    int width = 0, height = 0;
    /// a contiguous, tightly packed frame of width*height*3/2 bytes (what cv2 / ffmpeg rawvideo hand out)
    static yuv420_frame packed(int format, const uint8_t* data, int width, int height)
    {
        yuv420_frame f;
        f.format = format, f.y = data, f.width = width, f.height = height, f.y_stride = width;
        f.u = data + (size_t)width * height;
        f.uv_stride = format == HP_YUV_NV12 ? width : width / 2;
        f.v = format == HP_YUV_NV12 ? nullptr : f.u + (size_t)(width / 2) * (height / 2);
        return f;
    }
    bool empty() const { return !y || !u || width <= 0 || height <= 0; }
};

/// Addition: one video frame of ANY layout the C ABI's hp_yuv_image names (include/hp_hip.h: NV12 I420 P010 I010 NV16 I422 YUY2 UYVY
/// I444), with its colour matrix (HP_YUV_BT601 / _BT709 / _BT2020) and range (HP_YUV_LIMITED / _FULL), planes addressed by their own
/// pointers and row strides in bytes, in host memory or - `on_device` - in device memory on the engine's device (a decoder surface: it
/// is read where it lies, nothing is copied; it must be complete when inference() is called).  dnn::tensorrt::inference / calibrate
/// take a vector of these; the conversion (hp_resize_yuv's arithmetic) happens inside the resize kernel.  A yuv420_frame converts
/// implicitly: BT.601 limited range, which is what its own overloads compute.
struct yuv_frame {
    int format = HP_YUV_NV12, matrix = HP_YUV_BT601, range = HP_YUV_LIMITED;
    int width = 0, height = 0;
    const void* plane[3] = { nullptr, nullptr, nullptr }; // Y (or the packed plane), U or UV, V
    int stride[3] = { 0, 0, 0 };                          // bytes
    bool on_device = false;

    yuv_frame() = default;
    yuv_frame(const yuv420_frame& f) // NOLINT: implicit on purpose
        : format(f.format), width(f.width), height(f.height)
    {
        plane[0] = f.y, plane[1] = f.u, plane[2] = f.format == HP_YUV_I420 ? f.v : nullptr;
        stride[0] = f.y_stride, stride[1] = f.uv_stride, stride[2] = f.format == HP_YUV_I420 ? f.uv_stride : 0;
    }
    /// number of planes (0 for an unknown format), unpadded bytes per row and number of rows of plane k: hp_yuv_plane_layout, the C ABI's
    /// one statement of the layouts (0 for a size the layout cannot hold)
    static int plane_count(int format) { return hp_yuv_plane_layout(format, 0, 2, 2, nullptr, nullptr); }
    static size_t row_bytes(int format, int k, int width, int height)
    {
        size_t row = 0;
        hp_yuv_plane_layout(format, k, width, height, &row, nullptr);
        return row;
    }
    static int rows(int format, int k, int width, int height)
    {
        int n = 0;
        hp_yuv_plane_layout(format, k, width, height, nullptr, &n);
        return n;
    }
    /// a contiguous, tightly packed frame of hp_yuv_packed_bytes(format, width, height) bytes: planes back to back, rows without padding
    static yuv_frame packed(int format, const void* data, int width, int height, int matrix = HP_YUV_BT601, int range = HP_YUV_LIMITED,
        bool on_device = false)
    {
        yuv_frame f;
        f.format = format, f.matrix = matrix, f.range = range, f.width = width, f.height = height, f.on_device = on_device;
        const uint8_t* at = (const uint8_t*)data;
        for (int k = 0; k < plane_count(format); ++k) {
            f.plane[k] = at, f.stride[k] = (int)row_bytes(format, k, width, height);
            at += row_bytes(format, k, width, height) * (size_t)rows(format, k, width, height);
        }
        return f;
    }
    hp_yuv_image image() const
    {
        hp_yuv_image im;
        im.format = format, im.matrix = matrix, im.range = range, im.width = width, im.height = height;
        for (int k = 0; k < 3; ++k)
            im.plane[k] = plane[k], im.stride[k] = stride[k];
        return im;
    }
    bool empty() const { return !plane[0] || width <= 0 || height <= 0; }
};

/// Addition: one packed 8-bit frame of any layout the C ABI's hp_rgb_image names (include/hp_hip.h, "packed RGB and grey frames": HP_RGB_BGR24,
/// _RGB24, _BGRA32, _RGBA32, _ARGB32, _ABGR32, _GRAY8) - what screen capture, compositors, canvases, PIL-style pictures and grey cameras deliver -
/// with its row stride in bytes, in host memory or - `on_device` - in device memory on the engine's device (read where it lies, nothing is copied;
/// complete when inference() is called; 4-byte layouts then need an address and a stride that are multiples of 4).  Memory order is as the name
/// reads, the fourth byte is ignored, grey gives B = G = R.  dnn::tensorrt::inference / calibrate take a vector of these; nothing is repacked on the
/// host: the layout is read inside the resize kernel.
struct rgb_frame {
    int format = HP_RGB_BGR24;
    int width = 0, height = 0;
    const void* data = nullptr;
    int stride = 0; // bytes
    bool on_device = false;

    rgb_frame() = default;
    /// a frame whose rows are `stride` bytes apart
    rgb_frame(int format, const void* data, int width, int height, int stride, bool on_device = false)
        : format(format), width(width), height(height), data(data), stride(stride), on_device(on_device)
    {
    }
    /// a contiguous, tightly packed frame of hp_rgb_packed_bytes(format, width, height) bytes
    static rgb_frame packed(int format, const void* data, int width, int height, bool on_device = false)
    {
        return rgb_frame(format, data, width, height, width * hp_rgb_pixel_bytes(format), on_device);
    }
    hp_rgb_image image() const
    {
        hp_rgb_image im;
        im.format = format, im.width = width, im.height = height, im.data = data, im.stride = stride;
        return im;
    }
    bool empty() const { return !data || width <= 0 || height <= 0; }
};

// ---- free functions of the reference's data.hpp (:58-67), evaluated by the same device code as the engine's own pre-processing
namespace detail {
    struct dev_ptr { // scoped hp_malloc
        void* p = nullptr;
        explicit dev_ptr(size_t n) { hp_malloc(&p, n); }
        ~dev_ptr() { hp_free(p); }
        dev_ptr(const dev_ptr&) = delete;
    };
    inline const uint8_t* mat_data(const cv::Mat& m)
    {
#ifdef HYPERPOSE_USE_OPENCV
        return m.data;
#else
        return m.data();
#endif
    }
} // namespace detail

/// nhwc_images_append_nchw_batch (include/hyperpose/utility/data.hpp:58-64, src/data.cpp:21-51): u8 HWC images -> f32 CHW appended to
/// `data`, every value multiplied by `factor`, channels {2,1,0} when flip_rb.  hp_preproc_u8hwc_to_f32nchw does the arithmetic.
inline void nhwc_images_append_nchw_batch(std::vector<float>& data, std::vector<cv::Mat> images, double factor = 1.0, bool flip_rb = false)
{
    for (const auto& im : images) {
        const size_t n = (size_t)im.rows * im.cols * 3;
        if (!n)
            continue;
        detail::dev_ptr din(n), dout(n * sizeof(float));
        const size_t at = data.size();
        data.resize(at + n);
        if (!din.p || !dout.p || hp_memcpy_h2d(din.p, detail::mat_data(im), n) != HP_OK
            || hp_preproc_u8hwc_to_f32nchw((const uint8_t*)din.p, 1, im.rows, im.cols, factor, flip_rb ? 1 : 0, (float*)dout.p, nullptr) != HP_OK
            || hp_device_synchronize() != HP_OK || hp_memcpy_d2h(data.data() + at, dout.p, n * sizeof(float)) != HP_OK)
            throw std::runtime_error(hp_last_error());
    }
}

/// non_scaling_resize (data.hpp:67, src/data.cpp:53-69): aspect-preserving resize into the top-left corner of a `size` image filled with
/// `bgcolor`; hp_letterbox_u8c3 does the arithmetic (bit-equal to cv::resize INTER_LINEAR on the resized region).
inline cv::Mat non_scaling_resize(const cv::Mat& input, const cv::Size& size, const std::array<int, 3>& bgcolor = { 0, 0, 0 })
{
    cv::Mat out(size.height, size.width, CV_8UC3);
    const size_t ni = (size_t)input.rows * input.cols * 3, no = (size_t)size.area() * 3;
    detail::dev_ptr din(ni), dout(no);
    if (!din.p || !dout.p || hp_memcpy_h2d(din.p, detail::mat_data(input), ni) != HP_OK
        || hp_letterbox_u8c3((const uint8_t*)din.p, input.cols, input.rows, input.cols * 3, (uint8_t*)dout.p, size.width, size.height, size.width * 3,
               bgcolor[0], bgcolor[1], bgcolor[2], nullptr) != HP_OK
        || hp_device_synchronize() != HP_OK || hp_memcpy_d2h(const_cast<uint8_t*>(detail::mat_data(out)), dout.p, no) != HP_OK)
        throw std::runtime_error(hp_last_error());
    return out;
}

} // namespace hyperpose
