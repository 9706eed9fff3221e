// hyperpose::dnn::tensorrt over libhp_hip.so — the class name, constructor signatures, member functions and error behaviour of the
// reference engine (include/hyperpose/operator/dnn/tensorrt.hpp:14-19, 33-141; src/tensorrt.cpp), so that reference call sites such as
// examples/operator_api_batched_images_paf.example.cpp:36-56 compile and run unchanged:
//     tensorrt(onnx{file}, {w, h}, batch)          tensorrt(uff{...}, {w, h}, batch)          tensorrt(tensorrt_serialized{file}, {w, h}, batch)
//     engine.inference(std::vector<cv::Mat>)       engine.inference(std::vector<float> nchw, n)       engine.save(path)
// Header-only on top of the C ABI (include/hp_hip.h); the network runs as hand-written gfx950 kernels.  `data_type` selects the
// arithmetic as it does in the reference (src/tensorrt.cpp:327,353): kFLOAT - the default, as there - is fp32 storage and fp32
// matrix-pipe arithmetic (HP_DTYPE_F32), kHALF the fused fp16 kernels with fp32 accumulation (HP_DTYPE_F16, the fast path), kINT8
// post-training quantization on the int8 matrix pipe (HP_DTYPE_I8): such an engine infers only after calibrate() (TensorRT's MinMax
// calibrator over the given frames) or after loading a serialized engine that was calibrated; kINT32 / kBOOL have no meaning for these
// networks and are refused like an engine-build failure.  Frames of any size are resized on
// the DEVICE exactly as the reference does on the host: cv::resize (INTER_LINEAR) or, with keep_ratio, non_scaling_resize
// (src/tensorrt.cpp:446-451, src/data.cpp:53-69) through hp_resize_u8c3 / hp_letterbox_u8c3.  Addition: inference / calibrate also take
// std::vector<yuv420_frame> (NV12 / I420 video frames, utility/data.hpp), converted inside the resize kernel (hp_resize_yuv420), and
// std::vector<yuv_frame> (every layout, matrix and range of hp_yuv_image, host or device-resident; hp_resize_yuv) and std::vector<rgb_frame> (packed
// RGB, BGRA-family and grey frames with a stride, host or device-resident; hp_resize_rgb).
#pragma once
#include <array>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../../hp_hip.h"
#include "../../utility/data.hpp"
#include "../../utility/model.hpp"

namespace hyperpose {

/// Data type related to TensorRT data type (include/hyperpose/operator/dnn/tensorrt.hpp:14-30).
struct data_type {
    static constexpr int kFLOAT = 0;
    static constexpr int kHALF = 1;
    static constexpr int kINT8 = 2;
    static constexpr int kINT32 = 3;
    static constexpr int kBOOL = 4;
    int val = kFLOAT;
    inline data_type(int v)
        : val(v)
    {
    }
    /// HP_DTYPE_* of the C ABI, or -1 for the types no engine is built in
    inline int hp_dtype() const { return val == kFLOAT ? HP_DTYPE_F32 : val == kHALF ? HP_DTYPE_F16 : val == kINT8 ? HP_DTYPE_I8 : -1; }
};

namespace detail {
    // 8-bit BGR pixels of a cv::Mat for both the bundled cv_min.hpp and real OpenCV (cv::Mat::data is a member there and the matrix
    // may be non-continuous or of another type)
    inline const uint8_t* mat_bytes(const cv::Mat& m, std::vector<uint8_t>& scratch)
    {
#ifdef HYPERPOSE_USE_OPENCV
        if (m.type() != CV_8UC3)
            throw std::logic_error("hyperpose: frames must be 8-bit 3-channel (CV_8UC3)");
        if (m.isContinuous())
            return m.data;
        scratch.resize((size_t)m.rows * m.cols * 3);
        for (int r = 0; r < m.rows; ++r)
            std::memcpy(scratch.data() + (size_t)r * m.cols * 3, m.ptr(r), (size_t)m.cols * 3);
        return scratch.data();
#else
        (void)scratch;
        return m.data();
#endif
    }
} // namespace detail

namespace dnn {

    class tensorrt {
    public:
        /// UFF is TensorRT's own graph format and cannot be read here: like every unrecoverable engine error of the reference
        /// (src/tensorrt.cpp:141-158) this logs and exits.
        explicit tensorrt(const uff& uff_model, cv::Size input_size, int max_batch_size = 8, bool keep_ratio = false,
            data_type dtype = data_type::kFLOAT, double factor = 1. / 255, bool flip_rgb = true)
            : m_inp_size(input_size), m_max_batch_size(max_batch_size), m_keep_ratio(keep_ratio), m_factor(factor), m_flip_rgb(flip_rgb)
        {
            (void)dtype;
            fatal(("UFF models (" + uff_model.model_path + ") are a TensorRT format; export the model to ONNX (dnn::onnx) instead").c_str());
        }

        explicit tensorrt(const onnx& onnx_model, cv::Size input_size, int max_batch_size = 8, bool keep_ratio = false,
            data_type dtype = data_type::kFLOAT, double factor = 1. / 255, bool flip_rgb = true)
            : m_inp_size(input_size), m_max_batch_size(max_batch_size), m_keep_ratio(keep_ratio), m_factor(factor), m_flip_rgb(flip_rgb)
        {
            if (dtype.hp_dtype() < 0)
                fatal("hyperpose::dnn::tensorrt: only data_type::kFLOAT, data_type::kHALF and data_type::kINT8 engines can be built");
            if (hp_model_from_onnx_file(&m_model, onnx_model.model_path.c_str(), input_size.width, input_size.height) != HP_OK)
                fatal(hp_last_error());
            if (hp_engine_create_from_model_dtype(&m_engine, m_model, max_batch_size, factor, flip_rgb ? 1 : 0, nullptr, 0, dtype.hp_dtype()) != HP_OK)
                fatal(hp_last_error());
            after_create();
        }

        explicit tensorrt(const tensorrt_serialized& serialized_model, cv::Size input_size, int max_batch_size = 8, bool keep_ratio = false,
            double factor = 1. / 255, bool flip_rgb = true)
            : m_inp_size(input_size), m_max_batch_size(max_batch_size), m_keep_ratio(keep_ratio), m_factor(factor), m_flip_rgb(flip_rgb)
        {
            // (factor / flip_rgb are stored in the file by `save`, as TensorRT bakes them into the plan it serializes)
            if (hp_engine_load(&m_engine, serialized_model.model_path.c_str(), max_batch_size) != HP_OK)
                fatal(hp_last_error());
            int w = 0, h = 0;
            hp_engine_input_size(m_engine, &w, &h);
            if (w != input_size.width || h != input_size.height)
                fatal("serialized engine was built for another input size");
            after_create();
        }

        /// Addition: a built-in topology (no model file needed).
        explicit tensorrt(const builtin_model& model, cv::Size input_size, int max_batch_size = 8, bool keep_ratio = false,
            data_type dtype = data_type::kFLOAT, double factor = 1. / 255, bool flip_rgb = true)
            : m_inp_size(input_size), m_max_batch_size(max_batch_size), m_keep_ratio(keep_ratio), m_factor(factor), m_flip_rgb(flip_rgb)
        {
            if (dtype.hp_dtype() < 0)
                fatal("hyperpose::dnn::tensorrt: only data_type::kFLOAT, data_type::kHALF and data_type::kINT8 engines can be built");
            if (hp_model_build(&m_model, model.arch.c_str(), input_size.width, input_size.height) != HP_OK)
                fatal(hp_last_error());
            std::vector<float> w = model.weights;
            if (w.empty()) {
                w.resize(hp_model_num_weights(m_model));
                hp_model_init_weights(m_model, model.seed, w.data(), w.size());
            }
            if (hp_engine_create_from_model_dtype(&m_engine, m_model, max_batch_size, factor, flip_rgb ? 1 : 0, w.data(), w.size(), dtype.hp_dtype()) != HP_OK)
                fatal(hp_last_error());
            after_create();
        }

        /// The builtin_model constructor (an addition of this library) took (model, size, batch, keep_ratio, factor, flip_rgb) before it learned
        /// `dtype`; data_type(int) is implicit - as in the reference - so that old positional call would still compile, with factor truncated
        /// into a data_type.  A floating-point argument in the dtype position is a compile error instead.
        template <class F, class = typename std::enable_if<std::is_floating_point<F>::value>::type>
        tensorrt(const builtin_model&, cv::Size, int, bool, F, bool = true) = delete;

        tensorrt(const tensorrt&) = delete;
        tensorrt& operator=(const tensorrt&) = delete;
        ~tensorrt()
        {
            retire_last_batch(); // maps of the last call that are still alive get their host copy before the buffers go
            if (m_host_net)
                hp_free_host(m_host_net);
            if (m_dev_raw)
                hp_free(m_dev_raw);
            if (m_dev_net)
                hp_free(m_dev_net);
            hp_tonemap_destroy(m_tonemap);
            hp_engine_destroy(m_engine);
            hp_model_destroy(m_model);
        }

        inline int max_batch_size() noexcept { return m_max_batch_size; }

        /// Addition: HDR input (utility/data.hpp, hdr; hp_tonemap_create).  While set, the 10-bit yuv_frames (HP_YUV_P010 / HP_YUV_I010) of
        /// inference(std::vector<yuv_frame>), calibrate(std::vector<yuv_frame>) and inference(yuv_frame, regions) are PQ / HLG frames and are
        /// tone-mapped to SDR sRGB while they are resized (hp_resize_yuv_hdr, hp_letterbox_yuv_hdr, hp_resize_rois_yuv_hdr); 8-bit frames take
        /// the SDR calls as before.  A description the C ABI refuses is a std::logic_error and leaves the previous one in place.
        void set_tonemap(const hdr& h)
        {
            const hp_hdr_desc d = h.c_form();
            hp_tonemap* next = nullptr;
            if (hp_tonemap_create(&next, &d) != HP_OK)
                throw std::logic_error(hp_last_error());
            hp_tonemap_destroy(m_tonemap);
            m_tonemap = next;
        }
        void clear_tonemap()
        {
            hp_tonemap_destroy(m_tonemap);
            m_tonemap = nullptr;
        }
        /// Addition: upright input (utility/data.hpp, orientation; hp_resize_oriented_*).  While a non-upright orientation is set, the frames of
        /// inference(std::vector<cv::Mat>), inference(std::vector<yuv_frame>), both inference(frame, regions) and their calibrate() twins are
        /// STORED frames and are read upright inside the resize: the maps equal those of the same call on the frames oriented first
        /// (hp_orient_u8c3_host), bit for bit; regions are in UPRIGHT coordinates (plan them on oriented_size()).  The yuv420_frame overloads
        /// throw std::logic_error while an orientation is set: pass yuv_frames.
        void set_orientation(const orientation& o) { m_orientation = o.code(); }
        /// Addition: flip ensemble (include/hp_hip.h, "flip ensemble"; hp_engine_set_flip_ensemble_coco).  While on, every inference() call on frames
        /// or regions runs each network-sized picture and its left-right flip and returns the merged maps: left and right channels swapped back, the
        /// x component of the part-affinity fields negated, the two sets averaged, on the device.  The batch then holds max_batch_size() / 2 frames or
        /// regions (the over-size-batch std::logic_error beyond) and the float-buffer overload throws std::logic_error.  COCO PAF networks only: an
        /// engine with other outputs is a std::logic_error with the C ABI's message (other skeletons: hp_engine_set_flip_ensemble on handle()).
        void set_flip_ensemble(bool on)
        {
            if (hp_engine_set_flip_ensemble_coco(m_engine, on ? 1 : 0) != HP_OK)
                throw std::logic_error(hp_last_error());
        }
        bool flip_ensemble() const { return hp_engine_flip_ensemble(m_engine) == 1; }
        /// Addition: scale ensemble (include/hp_hip.h, "scale ensemble"; hp_engine_set_scale_ensemble_coco).  While on, every inference() call on
        /// frames or regions also runs each network-sized picture shrunk by every one of `scales` (1 .. 3 values in (0, 1]) and returns the maps
        /// of the K = scales.size() + 1 passes resampled to the map grid and averaged, on the device.  The batch then holds max_batch_size() / K
        /// frames or regions (/ 2K with the flip ensemble) and the float-buffer overload throws std::logic_error.  COCO PAF networks only (a
        /// std::logic_error with the C ABI's message otherwise).  An empty list turns it off.
        void set_scale_ensemble(const std::vector<float>& scales)
        {
            if (hp_engine_set_scale_ensemble_coco(m_engine, scales.data(), (int)scales.size()) != HP_OK)
                throw std::logic_error(hp_last_error());
        }
        int scale_ensemble() const { return hp_engine_scale_ensemble(m_engine); } // K, 1 while off
        inline cv::Size input_size() noexcept { return m_inp_size; }

        /// src/tensorrt.cpp:436-461: every image is brought to the network's size (cv::resize, or non_scaling_resize when keep_ratio)
        /// and the batch is inferred; throws std::logic_error on an over-size batch (:439-443).
        std::vector<internal_t> inference(std::vector<cv::Mat> inputs)
        {
            if (!begin_batch(inputs.size()))
                return {};
            const size_t net_frame = net_frame_bytes();
            if (!m_host_net && hp_malloc_host((void**)&m_host_net, net_frame * m_max_batch_size) != HP_OK)
                fatal(hp_last_error());
            std::vector<uint8_t> scratch;
            bool all_net_sized = m_orientation == HP_ORIENT_NONE;
            for (const cv::Mat& f : inputs) {
                if (f.empty())
                    fatal("hyperpose::dnn::tensorrt::inference: empty image");
                all_net_sized = all_net_sized && f.cols == m_inp_size.width && f.rows == m_inp_size.height;
            }
            if (all_net_sized) {
                // resize to the same size is a copy (src/tensorrt.cpp:446-451): the frames are gathered in ONE pinned buffer and go up in one
                // asynchronous copy per half-batch in front of the network's launches (the reference converts every frame to an f32 NCHW
                // staging vector on the host and copies 4 x the bytes, src/tensorrt.cpp:380-383)
                for (size_t i = 0; i < inputs.size(); ++i)
                    std::memcpy(m_host_net + i * net_frame, detail::mat_bytes(inputs[i], scratch), net_frame);
                if (hp_engine_infer_u8(m_engine, m_host_net, (int)inputs.size(), 0, nullptr) != HP_OK)
                    fatal(hp_last_error());
                return collect(inputs.size());
            }
            for (size_t i = 0; i < inputs.size(); ++i)
                frame_to_device(inputs[i], m_dev_net + i * net_frame, scratch);
            return run_batch(inputs.size());
        }

        /// Addition: the same call for video frames in the decoder's own form (utility/data.hpp, yuv420_frame: NV12 or I420 in host memory).
        /// Every frame is uploaded in its 1.5-byte form and brought to the network's size by the fused conversion + resize kernel
        /// (hp_resize_yuv420, or hp_letterbox_yuv420 when keep_ratio): the maps equal those of the cv::Mat overload on the frames
        /// converted with cv::cvtColor(COLOR_YUV2BGR_NV12 / _I420), bit for bit.  Same over-size-batch exception, same calibration rule.
        std::vector<internal_t> inference(const std::vector<yuv420_frame>& inputs)
        {
            if (!begin_batch(inputs.size()))
                return {};
            std::vector<uint8_t> scratch;
            for (size_t i = 0; i < inputs.size(); ++i)
                yuv_frame_to_device(inputs[i], m_dev_net + i * net_frame_bytes(), scratch);
            return run_batch(inputs.size());
        }

        /// Addition: the same call for frames of any layout, colour matrix and range (utility/data.hpp, yuv_frame), in host memory or -
        /// yuv_frame::on_device - as device-resident decoder surfaces that are read where they lie.  A host frame is uploaded in its own
        /// packed form (hp_yuv_packed_bytes) and brought to the network's size by hp_resize_yuv (hp_letterbox_yuv when keep_ratio); the
        /// maps equal those of the cv::Mat overload on the converted frames, bit for bit.  Same over-size-batch exception, same
        /// calibration rule.  A std::vector<yuv420_frame> keeps its own overload above.
        std::vector<internal_t> inference(const std::vector<yuv_frame>& inputs)
        {
            if (!begin_batch(inputs.size()))
                return {};
            std::vector<uint8_t> scratch;
            for (size_t i = 0; i < inputs.size(); ++i)
                yuv_image_to_device(inputs[i], m_dev_net + i * net_frame_bytes(), scratch);
            return run_batch(inputs.size());
        }

        /// Addition: the same call for packed RGB, BGRA-family and grey frames (utility/data.hpp, rgb_frame), in host memory or - rgb_frame::on_device -
        /// device-resident.  A host frame is uploaded once in its own form (hp_rgb_packed_bytes: nothing is repacked to BGR on the host) and brought
        /// to the network's size by hp_resize_rgb; the maps equal those of the cv::Mat overload on the frames converted with hp_rgb_to_bgr_host, bit
        /// for bit.  set_orientation and both ensembles act as for every other frame type; a tone-map does not apply (8-bit SDR frames).  Same
        /// over-size-batch exception, same calibration rule; a description the C ABI refuses is a std::logic_error.
        std::vector<internal_t> inference(const std::vector<rgb_frame>& inputs)
        {
            if (!begin_batch(inputs.size()))
                return {};
            std::vector<uint8_t> scratch;
            for (size_t i = 0; i < inputs.size(); ++i)
                rgb_image_to_device(inputs[i], m_dev_net + i * net_frame_bytes(), scratch);
            return run_batch(inputs.size());
        }

        /// Addition: many regions of ONE frame in one call (tiled inference: hyperpose::plan_tiles, to_frame, merge_humans).  One packet per
        /// region, each equal, bit for bit, to inference() of that region cut out into a cv::Mat of its own: the frame goes up once and
        /// all regions are brought to the network's size by one hp_resize_rois_u8c3 call.  regions.size() <= max_batch_size
        /// (std::logic_error beyond); a region that is empty or not inside the frame is a std::logic_error too.
        std::vector<internal_t> inference(const cv::Mat& frame, const std::vector<cv::Rect>& regions)
        {
            if (!begin_batch(regions.size()))
                return {};
            if (frame.empty())
                fatal("hyperpose::dnn::tensorrt::inference: empty image");
            std::vector<uint8_t> scratch;
            const uint8_t* src = detail::mat_bytes(frame, scratch);
            const size_t bytes = (size_t)frame.cols * frame.rows * 3;
            reserve_raw(bytes);
            if (hp_memcpy_h2d(m_dev_raw, src, bytes) != HP_OK)
                fatal(hp_last_error());
            const std::vector<hp_roi> rois = to_rois(regions);
            if (hp_resize_rois_oriented_u8c3(m_dev_raw, frame.cols, frame.rows, frame.cols * 3, m_orientation, rois.data(), (int)rois.size(),
                    m_keep_ratio ? 1 : 0, 0, 0, 0, m_dev_net, m_inp_size.width, m_inp_size.height, m_inp_size.width * 3, net_frame_bytes(),
                    hp_engine_stream(m_engine))
                != HP_OK) // (orientation 0 forwards to hp_resize_rois_u8c3)
                throw std::logic_error(hp_last_error());
            return run_batch(rois.size());
        }

        /// The same for a yuv_frame (host planes are uploaded once, a device-resident surface is read where it lies; hp_resize_rois_yuv):
        /// the regions keep the layout's alignment (hyperpose::plan_tiles(size, tiling, frame.format) plans them so).
        std::vector<internal_t> inference(const yuv_frame& frame, const std::vector<cv::Rect>& regions)
        {
            if (!begin_batch(regions.size()))
                return {};
            std::vector<uint8_t> scratch;
            const hp_yuv_image im = yuv_image_on_device(frame, scratch);
            const std::vector<hp_roi> rois = to_rois(regions);
            // (orientation 0 forwards to hp_resize_rois_yuv, or with a tone-map to hp_resize_rois_yuv_hdr)
            if (hp_resize_rois_oriented_yuv(&im, tonemap_for(frame), m_orientation, rois.data(), (int)rois.size(), m_keep_ratio ? 1 : 0, 0, 0, 0, m_dev_net,
                    m_inp_size.width, m_inp_size.height, m_inp_size.width * 3, net_frame_bytes(), hp_engine_stream(m_engine))
                != HP_OK)
                throw std::logic_error(hp_last_error());
            return run_batch(rois.size());
        }

        /// The same for an rgb_frame (hp_resize_rois_rgb): regions of any alignment, in upright coordinates under set_orientation.
        std::vector<internal_t> inference(const rgb_frame& frame, const std::vector<cv::Rect>& regions)
        {
            if (!begin_batch(regions.size()))
                return {};
            std::vector<uint8_t> scratch;
            const hp_rgb_image im = rgb_image_on_device(frame, scratch);
            const std::vector<hp_roi> rois = to_rois(regions);
            if (hp_resize_rois_rgb(&im, m_orientation, rois.data(), (int)rois.size(), m_keep_ratio ? 1 : 0, 0, 0, 0, m_dev_net, m_inp_size.width,
                    m_inp_size.height, m_inp_size.width * 3, net_frame_bytes(), hp_engine_stream(m_engine))
                != HP_OK)
                throw std::logic_error(hp_last_error());
            return run_batch(rois.size());
        }

        /// data_type::kINT8: TensorRT's MinMax calibration (an IInt8MinMaxCalibrator fed with these frames).  Frames of any size are brought to
        /// the network's size exactly as inference() does; any number of frames (the engine runs them in max_batch_size chunks).  Replaces
        /// every per-layer activation scale; calibration is never implicit.
        void calibrate(const std::vector<cv::Mat>& frames)
        {
            calibrate_with(frames, [this](const cv::Mat& f, uint8_t* dst, std::vector<uint8_t>& scratch) {
                if (f.empty())
                    fatal("hyperpose::dnn::tensorrt::calibrate: empty image");
                frame_to_device(f, dst, scratch);
            });
        }
        /// Addition: calibration from YUV 4:2:0 frames, brought to the network's size exactly as inference(std::vector<yuv420_frame>) does
        void calibrate(const std::vector<yuv420_frame>& frames)
        {
            calibrate_with(frames, [this](const yuv420_frame& f, uint8_t* dst, std::vector<uint8_t>& scratch) { yuv_frame_to_device(f, dst, scratch); });
        }
        /// Addition: calibration from frames of any layout, brought to the network's size exactly as inference(std::vector<yuv_frame>) does
        void calibrate(const std::vector<yuv_frame>& frames)
        {
            calibrate_with(frames, [this](const yuv_frame& f, uint8_t* dst, std::vector<uint8_t>& scratch) { yuv_image_to_device(f, dst, scratch); });
        }
        /// Addition: calibration from packed RGB / grey frames, brought to the network's size exactly as inference(std::vector<rgb_frame>) does
        void calibrate(const std::vector<rgb_frame>& frames)
        {
            calibrate_with(frames, [this](const rgb_frame& f, uint8_t* dst, std::vector<uint8_t>& scratch) { rgb_image_to_device(f, dst, scratch); });
        }
        /// false for a data_type::kINT8 engine that was neither calibrated nor loaded calibrated
        bool calibrated() const
        {
            if (hp_engine_dtype(m_engine) != HP_DTYPE_I8)
                return true;
            hp_engine_desc d{};
            if (hp_engine_describe(m_engine, &d) != HP_OK || !d.int8_scales)
                return false;
            for (int i = 0; i < d.n_layers; ++i)
                if (d.int8_scales[i] < 0.f)
                    return false;
            return true;
        }

        /// src/tensorrt.cpp:364-434: plain NCHW float buffers, no scaling / channel swap.
        std::vector<internal_t> inference(const std::vector<float>& float_buffer, size_t batch_size)
        {
            if (batch_size > (size_t)m_max_batch_size)
                throw std::logic_error("Input batch size overflow: Yours@" + std::to_string(batch_size) + " Max@" + std::to_string(m_max_batch_size));
            if (float_buffer.size() < batch_size * 3 * (size_t)m_inp_size.area())
                throw std::logic_error("Input float buffer is smaller than batch_size x 3 x H x W");
            if (flip_ensemble())
                throw std::logic_error("hyperpose::dnn::tensorrt: float buffers are not available while the flip ensemble is on, pass frames");
            if (scale_ensemble() > 1)
                throw std::logic_error("hyperpose::dnn::tensorrt: float buffers are not available while the scale ensemble is on, pass frames");
            require_calibrated();
            retire_last_batch();
            if (hp_engine_infer_f32(m_engine, float_buffer.data(), (int)batch_size, 0, nullptr) != HP_OK)
                fatal(hp_last_error());
            return collect(batch_size);
        }

        /// tensorrt::save (tensorrt.hpp:121-123, src/tensorrt.cpp:463-471)
        void save(const std::string path)
        {
            if (hp_engine_save(m_engine, path.c_str()) != HP_OK)
                fatal(hp_last_error());
        }

        // ---- additions for device-resident use (the stream operator and the parsers' process_device forms)
        void inference_device(const uint8_t* dev_hwc_bgr, int n, void* stream = nullptr)
        {
            require_calibrated();
            retire_last_batch();
            if (hp_engine_infer_u8(m_engine, dev_hwc_bgr, n, 1, stream) != HP_OK)
                fatal(hp_last_error());
        }
        hp_engine* handle() { return m_engine; }
        bool keep_ratio() const { return m_keep_ratio; }
        /// Addition (utility/map_view.hpp): the fractions (x, y) of the network's input - and so of its output maps - that an UPRIGHT frame of
        /// `frame` pixels fills: the letterbox's inner size over the input size under keep_ratio, (1, 1) otherwise (hp_mapview_cover)
        std::array<double, 2> map_cover(cv::Size frame) const
        {
            std::array<double, 2> cover { 1., 1. };
            if (hp_mapview_cover(frame.width, frame.height, m_inp_size.width, m_inp_size.height, m_keep_ratio ? 1 : 0, cover.data()) != HP_OK)
                throw std::invalid_argument(hp_last_error());
            return cover;
        }

        /// frames or regions one inference() call takes: max_batch_size(), half of it while the flip ensemble is on, 1 / K of that under the scale ensemble
        size_t batch_room() const { return (size_t)m_max_batch_size / (flip_ensemble() ? 2 : 1) / scale_ensemble(); }
        std::string overflow_note() const
        {
            const int passes = scale_ensemble() * (flip_ensemble() ? 2 : 1);
            if (scale_ensemble() > 1) // (the flip ensemble's note below keeps its wording while the scale ensemble is off)
                return " (max_batch_size " + std::to_string(m_max_batch_size) + " / " + std::to_string(passes) + ": the scale ensemble"
                    + (flip_ensemble() ? " and the flip ensemble run" : " runs") + " every picture " + std::to_string(passes) + " times)";
            return flip_ensemble() ? " (max_batch_size " + std::to_string(m_max_batch_size) + " halved: the flip ensemble runs every picture with its flip)" : "";
        }

        void require_calibrated() const
        {
            if (!calibrated())
                throw std::logic_error("hyperpose::dnn::tensorrt: a data_type::kINT8 engine must be calibrated first: call calibrate() with "
                                       "representative frames (or load a serialized engine that was calibrated)");
        }

    private:
        size_t net_frame_bytes() const { return (size_t)m_inp_size.width * m_inp_size.height * 3; }
        // what every frame-taking inference() does first: the calibration rule, the over-size-batch exception, the batch buffer, and the
        // previous call's maps get their host copy (the engine is idle here: the previous call was synchronised before it returned).
        // False for an empty batch, which returns no packets.
        bool begin_batch(size_t n)
        {
            require_calibrated();
            if (n > batch_room())
                throw std::logic_error("Input batch size overflow: Yours@" + std::to_string(n) + " Max@" + std::to_string(batch_room()) + overflow_note());
            if (n == 0)
                return false;
            if (!m_dev_net && hp_malloc((void**)&m_dev_net, net_frame_bytes() * m_max_batch_size) != HP_OK)
                fatal(hp_last_error());
            retire_last_batch();
            return true;
        }
        // ... and last: the n network-sized slots in m_dev_net are inferred
        std::vector<internal_t> run_batch(size_t n)
        {
            if (hp_engine_infer_u8(m_engine, m_dev_net, (int)n, 1, nullptr) != HP_OK)
                fatal(hp_last_error());
            return collect(n);
        }
        // the body of every calibrate(): `to_device(frame, dst, scratch)` brings one frame to the network's size at device address dst
        template <class Frame, class ToDevice> void calibrate_with(const std::vector<Frame>& frames, ToDevice to_device)
        {
            if (hp_engine_dtype(m_engine) != HP_DTYPE_I8)
                throw std::logic_error("hyperpose::dnn::tensorrt::calibrate: only data_type::kINT8 engines are calibrated");
            if (frames.empty())
                throw std::logic_error("hyperpose::dnn::tensorrt::calibrate: no frames");
            retire_last_batch();
            uint8_t* all = nullptr; // every frame at the network's size, on the device: the calibration is one call over all of them
            if (hp_malloc((void**)&all, net_frame_bytes() * frames.size()) != HP_OK)
                fatal(hp_last_error());
            std::vector<uint8_t> scratch;
            for (size_t i = 0; i < frames.size(); ++i)
                to_device(frames[i], all + i * net_frame_bytes(), scratch);
            const int rc = hp_device_synchronize() == HP_OK ? hp_engine_calibrate_u8(m_engine, all, (int)frames.size(), 1) : HP_ERR_HIP;
            hp_free(all);
            if (rc != HP_OK)
                fatal(hp_last_error());
        }
        // one frame brought to the network's size at device address dst (src/tensorrt.cpp:446-451): cv::resize (INTER_LINEAR) or, with
        // keep_ratio, non_scaling_resize on the device, read upright under set_orientation; a network-sized upright frame is a copy
        void frame_to_device(const cv::Mat& f, uint8_t* dst, std::vector<uint8_t>& scratch)
        {
            const uint8_t* src = detail::mat_bytes(f, scratch);
            const size_t bytes = (size_t)f.cols * f.rows * 3;
            if (f.cols == m_inp_size.width && f.rows == m_inp_size.height && m_orientation == HP_ORIENT_NONE) { // resize to the same size is a copy
                if (hp_memcpy_h2d(dst, src, bytes) != HP_OK)
                    fatal(hp_last_error());
                return;
            }
            reserve_raw(bytes);
            if (hp_memcpy_h2d(m_dev_raw, src, bytes) != HP_OK)
                fatal(hp_last_error());
            // (orientation 0 forwards to hp_letterbox_u8c3 / hp_resize_u8c3)
            const int rc = hp_resize_oriented_u8c3(m_dev_raw, f.cols, f.rows, f.cols * 3, m_orientation, m_keep_ratio ? 1 : 0, 0, 0, 0, dst, m_inp_size.width,
                m_inp_size.height, m_inp_size.width * 3, hp_engine_stream(m_engine));
            if (rc != HP_OK || hp_engine_synchronize(m_engine) != HP_OK) // m_dev_raw is re-used by the next frame
                fatal(hp_last_error());
        }
        // the same for a YUV 4:2:0 frame: its planes are packed without row padding into ONE upload of width*height*3/2 bytes, then the fused
        // conversion + resize (or letterbox) writes dst; a network-sized frame gets the conversion alone
        void yuv_frame_to_device(const yuv420_frame& f, uint8_t* dst, std::vector<uint8_t>& scratch)
        {
            if (f.empty() || (f.format == HP_YUV_I420 && !f.v))
                fatal("hyperpose::dnn::tensorrt: empty YUV frame");
            if (f.format != HP_YUV_NV12 && f.format != HP_YUV_I420)
                throw std::logic_error("hyperpose: yuv420_frame::format must be HP_YUV_NV12 or HP_YUV_I420");
            if (m_orientation != HP_ORIENT_NONE)
                throw std::logic_error("hyperpose: yuv420_frames are not available while an orientation is set, pass yuv_frames");
            if (f.width % 2 || f.height % 2)
                throw std::logic_error("hyperpose: YUV 4:2:0 frames need even width and height");
            const bool nv12 = f.format == HP_YUV_NV12;
            const size_t w = (size_t)f.width, h = (size_t)f.height, luma = w * h, bytes = luma * 3 / 2, crow = nv12 ? w : w / 2;
            if ((size_t)f.y_stride < w || (size_t)f.uv_stride < crow)
                throw std::logic_error("hyperpose: yuv420_frame stride smaller than a row");
            scratch.resize(bytes);
            for (size_t r = 0; r < h; ++r)
                std::memcpy(scratch.data() + r * w, f.y + r * (size_t)f.y_stride, w);
            for (size_t r = 0; r < h / 2; ++r) {
                std::memcpy(scratch.data() + luma + r * crow, f.u + r * (size_t)f.uv_stride, crow);
                if (!nv12)
                    std::memcpy(scratch.data() + luma + luma / 4 + r * crow, f.v + r * (size_t)f.uv_stride, crow);
            }
            reserve_raw(bytes);
            if (hp_memcpy_h2d(m_dev_raw, scratch.data(), bytes) != HP_OK)
                fatal(hp_last_error());
            const uint8_t *du = m_dev_raw + luma, *dv = nv12 ? nullptr : du + luma / 4;
            const int rc = m_keep_ratio
                ? hp_letterbox_yuv420(f.format, m_dev_raw, f.width, du, dv, (int)crow, f.width, f.height, dst, m_inp_size.width, m_inp_size.height,
                      m_inp_size.width * 3, 0, 0, 0, hp_engine_stream(m_engine))
                : hp_resize_yuv420(f.format, m_dev_raw, f.width, du, dv, (int)crow, f.width, f.height, dst, m_inp_size.width, m_inp_size.height,
                      m_inp_size.width * 3, hp_engine_stream(m_engine));
            if (rc != HP_OK || hp_engine_synchronize(m_engine) != HP_OK) // m_dev_raw is re-used by the next frame
                fatal(hp_last_error());
        }
        // the same for a yuv_frame of any layout: a host frame's planes are packed without row padding into ONE upload of
        // hp_yuv_packed_bytes, a device frame is read where it lies; then hp_resize_oriented_yuv writes dst: with orientation 0 that is
        // hp_resize_yuv / hp_letterbox_yuv, for a 10-bit frame under set_tonemap their *_hdr twins
        void yuv_image_to_device(const yuv_frame& f, uint8_t* dst, std::vector<uint8_t>& scratch)
        {
            const hp_yuv_image im = yuv_image_on_device(f, scratch);
            const int w = m_inp_size.width, h = m_inp_size.height;
            const int rc = hp_resize_oriented_yuv(&im, tonemap_for(f), m_orientation, m_keep_ratio ? 1 : 0, 0, 0, 0, dst, w, h, w * 3, hp_engine_stream(m_engine));
            if (rc != HP_OK || hp_engine_synchronize(m_engine) != HP_OK) // m_dev_raw is re-used by the next frame
                fatal(hp_last_error());
        }
        // the checks of a yuv_frame and its description as a kernel reads it: the caller's surface, or the packed copy in m_dev_raw
        hp_yuv_image yuv_image_on_device(const yuv_frame& f, std::vector<uint8_t>& scratch)
        {
            const int planes = yuv_frame::plane_count(f.format);
            if (planes == 0)
                throw std::logic_error("hyperpose: yuv_frame::format must be one of HP_YUV_NV12 .. HP_YUV_I444");
            if (f.empty())
                fatal("hyperpose::dnn::tensorrt: empty YUV frame");
            const size_t bytes = hp_yuv_packed_bytes(f.format, f.width, f.height);
            if (bytes == 0)
                throw std::logic_error("hyperpose: a yuv_frame of this format cannot be " + std::to_string(f.width) + " x " + std::to_string(f.height)
                    + " (4:2:0 needs even width and height, 4:2:2 an even width)");
            for (int k = 0; k < planes; ++k) {
                if (!f.plane[k])
                    fatal("hyperpose::dnn::tensorrt: empty YUV frame");
                if (f.stride[k] <= 0 || (size_t)f.stride[k] < yuv_frame::row_bytes(f.format, k, f.width, f.height))
                    throw std::logic_error("hyperpose: yuv_frame stride smaller than a row");
            }
            hp_yuv_image im = f.image();
            if (!f.on_device) {
                scratch.resize(bytes);
                reserve_raw(bytes);
                size_t at = 0;
                for (int k = 0; k < planes; ++k) {
                    const size_t row = yuv_frame::row_bytes(f.format, k, f.width, f.height);
                    im.plane[k] = m_dev_raw + at, im.stride[k] = (int32_t)row;
                    for (int r = 0; r < yuv_frame::rows(f.format, k, f.width, f.height); ++r, at += row)
                        std::memcpy(scratch.data() + at, (const uint8_t*)f.plane[k] + (size_t)r * f.stride[k], row);
                }
                if (hp_memcpy_h2d(m_dev_raw, scratch.data(), bytes) != HP_OK)
                    fatal(hp_last_error());
            }
            return im;
        }
        // the same for an rgb_frame: a host frame's rows are packed without padding into ONE upload of hp_rgb_packed_bytes, in its own layout; a
        // device frame is read where it lies; then hp_resize_rgb writes dst
        void rgb_image_to_device(const rgb_frame& f, uint8_t* dst, std::vector<uint8_t>& scratch)
        {
            const hp_rgb_image im = rgb_image_on_device(f, scratch);
            const int w = m_inp_size.width, h = m_inp_size.height;
            if (hp_resize_rgb(&im, m_orientation, m_keep_ratio ? 1 : 0, 0, 0, 0, dst, w, h, w * 3, hp_engine_stream(m_engine)) != HP_OK)
                throw std::logic_error(hp_last_error());
            if (hp_engine_synchronize(m_engine) != HP_OK) // m_dev_raw is re-used by the next frame
                fatal(hp_last_error());
        }
        // the checks of an rgb_frame and its description as a kernel reads it: the caller's surface, or the packed copy in m_dev_raw
        hp_rgb_image rgb_image_on_device(const rgb_frame& f, std::vector<uint8_t>& scratch)
        {
            hp_rgb_image im = f.image();
            const size_t pixel = (size_t)hp_rgb_pixel_bytes(f.format);
            if (pixel == 0)
                throw std::logic_error("hyperpose: rgb_frame::format must be one of HP_RGB_BGR24 .. HP_RGB_GRAY8");
            if (f.empty())
                throw std::logic_error("hyperpose: empty rgb_frame");
            const size_t row = (size_t)f.width * pixel, bytes = row * (size_t)f.height;
            if (f.stride <= 0 || (size_t)f.stride < row)
                throw std::logic_error("hyperpose: rgb_frame stride smaller than a row");
            if (!f.on_device) {
                const uint8_t* src = (const uint8_t*)f.data;
                if ((size_t)f.stride != row) {
                    scratch.resize(bytes);
                    for (int r = 0; r < f.height; ++r)
                        std::memcpy(scratch.data() + (size_t)r * row, src + (size_t)r * f.stride, row);
                    src = scratch.data();
                }
                reserve_raw(bytes);
                if (hp_memcpy_h2d(m_dev_raw, src, bytes) != HP_OK)
                    fatal(hp_last_error());
                im.data = m_dev_raw, im.stride = (int32_t)row;
            }
            return im;
        }
        // the tone-map of a frame: set_tonemap's for the 10-bit layouts, none (the SDR calls) otherwise
        const hp_tonemap* tonemap_for(const yuv_frame& f) const
        {
            return m_tonemap && (f.format == HP_YUV_P010 || f.format == HP_YUV_I010) ? m_tonemap : nullptr;
        }
        void reserve_raw(size_t bytes)
        {
            if (bytes <= m_raw_bytes)
                return;
            if (m_dev_raw)
                hp_free(m_dev_raw);
            m_dev_raw = nullptr, m_raw_bytes = 0;
            if (hp_malloc((void**)&m_dev_raw, bytes) != HP_OK)
                fatal(hp_last_error());
            m_raw_bytes = bytes;
        }
        static std::vector<hp_roi> to_rois(const std::vector<cv::Rect>& regions)
        {
            std::vector<hp_roi> r;
            for (const cv::Rect& q : regions)
                r.push_back(hp_roi{ q.x, q.y, q.width, q.height });
            return r;
        }
        [[noreturn]] static void fatal(const char* msg)
        {
            std::cerr << "[HyperPose::ERROR  ] " << msg << "\n";
            std::exit(-1);
        }
        // one batch in flight per call, like the reference's synchronous inference: kFLOAT engines run it as two half-batches side by side
        // (hp_engine_set_concurrency; bit-identical outputs, measured 2490 -> 1962 us per batch of 8 LW-OpenPose frames)
        void after_create()
        {
            m_calls = std::make_shared<std::atomic<uint64_t>>(0);
            if (!std::getenv("HP_MIRROR_ONE_STREAM"))
                hp_engine_set_concurrency(m_engine, 2);
        }
        // the maps of the previous call lose their device buffers now: those still alive copy themselves to the host first
        void retire_last_batch()
        {
            if (auto last = m_last.lock())
                last->materialize();
            m_last.reset();
            if (m_calls)
                ++*m_calls;
        }
        /// src/tensorrt.cpp:400-433: one internal_t per image, maps sorted by tensor name (:405).  The maps are views of the engine's device
        /// buffers with a host copy made on demand (utility/data.hpp, detail::device_batch).
        std::vector<internal_t> collect(size_t n)
        {
            if (hp_engine_synchronize(m_engine) != HP_OK)
                fatal(hp_last_error());
            auto rec = std::make_shared<detail::device_batch>();
            rec->engine = m_engine, rec->live = m_calls, rec->gen = m_calls->load(), rec->n = (int)n;
            const int no = hp_engine_num_outputs(m_engine);
            for (int i = 0; i < no; ++i) { // already sorted by tensor name (src/tensorrt.cpp:405)
                const char* name = nullptr;
                int shape[3];
                const float* dev = nullptr;
                hp_engine_output(m_engine, i, &name, shape, &dev);
                detail::device_batch::out o;
                o.name = name, o.shape = { shape[0], shape[1], shape[2] }, o.dev = dev, o.per = (size_t)shape[0] * shape[1] * shape[2];
                rec->outs.push_back(std::move(o));
            }
            std::vector<internal_t> ret(n);
            for (size_t j = 0; j < n; ++j)
                for (int i = 0; i < no; ++i)
                    ret[j].emplace_back(rec, i, (int)j);
            m_last = rec;
            if (std::getenv("HP_MIRROR_EAGER_HOST_COPY")) // (tests: the reference's behaviour, every map on the host before the call returns)
                rec->materialize();
            return ret;
        }
        const cv::Size m_inp_size; // w, h
        const int m_max_batch_size;
        const bool m_keep_ratio;
        const double m_factor;
        const bool m_flip_rgb;
        hp_model* m_model = nullptr;
        hp_engine* m_engine = nullptr;
        uint8_t* m_dev_raw = nullptr; // one camera-sized frame
        size_t m_raw_bytes = 0;
        uint8_t* m_dev_net = nullptr; // the batch at network size
        uint8_t* m_host_net = nullptr; // ... and its pinned staging copy on the host
        int m_orientation = HP_ORIENT_NONE; // set_orientation: the HP_ORIENT_* code of the stored frames
        hp_tonemap* m_tonemap = nullptr; // set_tonemap: the tables of the HDR description in device memory
        std::shared_ptr<std::atomic<uint64_t>> m_calls; // bumped whenever the engine's output buffers are about to be overwritten
        std::weak_ptr<detail::device_batch> m_last;
    };

} // namespace dnn
} // namespace hyperpose
