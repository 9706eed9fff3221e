// hyperpose::draw_maps — addition: what the network itself produced, shown on the frame.  The confidence maps (map_view::max: the largest channel)
// or the part-affinity fields (map_view::field: the longest vector) of one frame are colour-mapped, up-sampled with the parser's half-pixel
// bilinear rule and blended into a video frame where it lies, in the frame's own layout, matrix, range and bit depth (hp_mapview_*,
// include/hp_hip.h; the rules: DESIGN.md 1.1 "Map view").  The reference draws this view in Python (draw_results); its C++ surface has none.
// A yuv_frame with `on_device` set, or a device_bgr picture, is painted by two kernel launches on `stream` (asynchronous, stream-ordered) that read
// the engine's output where it lies while the feature map's device view is still valid - that is until the engine's next inference call - and a
// device copy of the map's host copy afterwards (that path waits for the stream); a yuv_frame in host memory is painted by the library's host twin
// from the host copy, which gives the same bytes.  `cover` is dnn::tensorrt::map_cover(frame size): which fraction of the maps the frame fills.
// Order on one frame: redact_humans, then draw_maps, then draw_humans on top.  The stream operator recycles its engine outputs before the caller
// holds the humans, so this view serves the operator API only; graphics white for PQ / HLG frames is out of scope (10-bit frames get the SDR
// formulas at depth 10).  Errors of the C ABI (opacity outside (0, 1], a gain <= 0, channels beyond the tensor's) throw std::logic_error.
#pragma once
#include <array>
#include <stdexcept>
#include <string>

#include "data.hpp"
#include "overlay.hpp"

namespace hyperpose {

struct map_view {
    enum { max = HP_MAPVIEW_MAX, field = HP_MAPVIEW_FIELD };
    enum { jet = HP_MAPVIEW_JET, heat = HP_MAPVIEW_HEAT, grey = HP_MAPVIEW_GREY };
    enum { constant = HP_MAPVIEW_ALPHA_CONSTANT, scaled = HP_MAPVIEW_ALPHA_SCALED };
    int mode = max;
    int palette = jet;
    int alpha = constant;
    float opacity = 0.5f;
    float gain = 1;
    int first_channel = 0;
    int channels = -1; /* all: every channel (max) or every pair (field) from first_channel on */
    int channel_step = 1; /* in units of the mode: channels (max) or (x, y) pairs (field: pair k starts at first_channel + 2 * k * channel_step) */
};

using map_cover = std::array<double, 2>; // (x, y) of hp_mapview_cover

namespace detail {
    inline void mapview_check(int rc)
    {
        if (rc < HP_OK)
            throw std::logic_error(std::string("hyperpose::draw_maps: ") + hp_last_error());
    }
    // the calling thread's hp_mapview handle (thread_handle, overlay.hpp)
    inline hp_mapview* mapview_handle(size_t cells)
    {
        return thread_handle<hp_mapview, hp_mapview_create, hp_mapview_destroy>(cells, 1 << 16, "hyperpose::draw_maps");
    }
    struct mapview_call {
        hp_mapview_desc d {};
        int32_t palette[256][4];
        std::unique_ptr<dev_ptr> staged; // a device copy of the host copy, when the engine's buffers have moved on
    };
    // `device`: the frame is in device memory, so the maps must be too
    inline void mapview_prepare(mapview_call& c, const feature_map_t& map, const map_cover& cover, const map_view& v, int orientation, bool device)
    {
        const auto& shape = map.shape();
        if (shape.size() != 3)
            throw std::logic_error("hyperpose::draw_maps: the feature map is not [C, H, W]");
        hp_mapview_desc& d = c.d;
        d.C = shape[0], d.mh = shape[1], d.mw = shape[2];
        const bool pairs = v.mode == map_view::field;
        d.c0 = v.first_channel, d.c_step = v.channel_step * (pairs ? 2 : 1);
        d.cn = v.channels >= 0 ? v.channels : d.c_step > 0 ? (d.C - d.c0 - (pairs ? 2 : 1)) / d.c_step + 1 : 0;
        d.mode = v.mode, d.gain = v.gain, d.cover_x = cover[0], d.cover_y = cover[1], d.orientation = orientation, d.has_roi = 0;
        if (const auto* batch = device ? map.device_batch() : nullptr)
            d.maps = batch->outs[(size_t)map.batch_output()].dev, d.frame = map.batch_frame();
        else {
            d.maps = map.view<float>(), d.frame = 0;
            if (device) {
                const size_t bytes = (size_t)d.C * d.mh * d.mw * sizeof(float);
                c.staged.reset(new dev_ptr(bytes));
                if (!c.staged->p || hp_memcpy_h2d(c.staged->p, d.maps, bytes) != HP_OK)
                    throw std::runtime_error(std::string("hyperpose::draw_maps: ") + hp_last_error());
                d.maps = static_cast<const float*>(c.staged->p);
            }
        }
        mapview_check(hp_mapview_palette(v.palette, v.alpha, c.palette));
    }
    // a staged copy is freed when the call returns: the stream must have read it by then
    inline void mapview_finish(const mapview_call& c)
    {
        if (c.staged)
            mapview_check(hp_device_synchronize());
    }
} // namespace detail

/// `frame.plane[]` is WRITTEN (the struct declares it const because the engine only reads it)
inline void draw_maps(yuv_frame& frame, const feature_map_t& map, const map_cover& cover, const orientation& o, const map_view& v = {}, void* stream = nullptr)
{
    detail::mapview_call c;
    detail::mapview_prepare(c, map, cover, v, o.code(), frame.on_device);
    const hp_yuv_image im = frame.image();
    if (frame.on_device) {
        detail::mapview_check(hp_mapview_draw_yuv(detail::mapview_handle((size_t)c.d.mh * c.d.mw), &im, &c.d, c.palette, v.opacity, stream));
        detail::mapview_finish(c);
    } else
        detail::mapview_check(hp_mapview_draw_yuv_host(&im, &c.d, c.palette, v.opacity));
}

inline void draw_maps(const device_bgr& picture, const feature_map_t& map, const map_cover& cover, const orientation& o, const map_view& v = {},
    void* stream = nullptr)
{
    detail::mapview_call c;
    detail::mapview_prepare(c, map, cover, v, o.code(), true);
    detail::mapview_check(hp_mapview_draw_u8c3(detail::mapview_handle((size_t)c.d.mh * c.d.mw), picture.ptr, picture.width, picture.height,
        picture.stride ? picture.stride : picture.width * 3, &c.d, c.palette, v.opacity, stream));
    detail::mapview_finish(c);
}

/// frames that are stored upright
inline void draw_maps(yuv_frame& frame, const feature_map_t& map, const map_cover& cover, const map_view& v = {}, void* stream = nullptr)
{
    draw_maps(frame, map, cover, orientation{}, v, stream);
}
inline void draw_maps(const device_bgr& picture, const feature_map_t& map, const map_cover& cover, const map_view& v = {}, void* stream = nullptr)
{
    draw_maps(picture, map, cover, orientation{}, v, stream);
}

} // namespace hyperpose
