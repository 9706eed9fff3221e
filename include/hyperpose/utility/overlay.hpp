// hyperpose::draw_humans — addition: the skeletons of a frame's humans painted into a video frame where it lies, in the frame's own layout,
// colour space and bit depth (hp_overlay_*, include/hp_hip.h).  The device-side counterpart of draw_human (human.hpp, untouched): a
// yuv_frame with `on_device` set, or a device_bgr picture, is painted by one kernel launch on `stream` (asynchronous, stream-ordered); a
// yuv_frame in host memory is painted by the library's host twin, which gives the same bytes.  The picture is defined by exact integer rules
//  - capsules of width T for limbs, discs of radius T for parts, T by draw_human's rule unless `thickness` > 0, the last
// primitive wins, `opacity` in (0, 1] blends - and is not cv::line / cv::circle's raster.  Humans are in the FRAME's normalised coordinates
// (after resume_ratio).  Errors of the C ABI (bad layout, opacity outside (0, 1], frames over 8192 x 8192) throw std::logic_error.
#pragma once
#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "data.hpp"
#include "human.hpp"

namespace hyperpose {

/// an 8-bit BGR HWC picture in device memory, rows `stride` bytes apart (0 = packed rows)
struct device_bgr {
    uint8_t* ptr = nullptr;
    int width = 0, height = 0, stride = 0;
};

namespace detail {
    inline std::vector<hp_human> to_c_humans(const std::vector<human_t>& humans)
    {
        std::vector<hp_human> out(humans.size());
        for (size_t i = 0; i < humans.size(); ++i) {
            for (int k = 0; k < COCO_N_PARTS; ++k) {
                const auto& p = humans[i].parts[k];
                out[i].parts[k] = hp_body_part{ p.has_value ? 1 : 0, p.x, p.y, p.score };
            }
            out[i].score = humans[i].score;
        }
        return out;
    }
    // the calling thread's handle of one kind (hp_overlay, hp_redact), made for at least `floor` items and grown when a frame brings more than
    // it was made for (one handle = one thread, hp_hip.h).  It is released when the thread ends; for the main thread that is before objects
    // of static storage duration are destroyed ([basic.start.term]), hence before the HIP runtime's own teardown, and the destroy functions
    // ignore what a late call returns
    template <class H, int (*Create)(H**, int), void (*Destroy)(H*)> H* thread_handle(size_t n, size_t floor, const char* who)
    {
        struct holder {
            H* h = nullptr;
            size_t cap = 0;
            ~holder() { Destroy(h); }
        };
        thread_local holder t;
        if (!t.h || t.cap < n) {
            Destroy(t.h);
            t.h = nullptr, t.cap = std::max(floor, n);
            if (Create(&t.h, (int)t.cap) != HP_OK)
                throw std::runtime_error(std::string(who) + ": " + hp_last_error());
        }
        return t.h;
    }
    inline hp_overlay* overlay_handle(size_t n_humans)
    {
        return thread_handle<hp_overlay, hp_overlay_create, hp_overlay_destroy>(n_humans, 64, "hyperpose::draw_humans");
    }
    inline void overlay_check(int rc)
    {
        if (rc != HP_OK)
            throw std::logic_error(std::string("hyperpose::draw_humans: ") + hp_last_error());
    }
} // namespace detail

/// `frame.plane[]` is WRITTEN (the struct declares it const because the engine only reads it)
inline void draw_humans(yuv_frame& frame, const std::vector<human_t>& humans, float opacity = 1, int thickness = 0, void* stream = nullptr)
{
    const auto list = detail::to_c_humans(humans);
    const hp_yuv_image im = frame.image();
    if (frame.on_device)
        detail::overlay_check(hp_overlay_draw_yuv(detail::overlay_handle(list.size()), &im, list.data(), (int)list.size(), opacity, thickness, stream));
    else
        detail::overlay_check(hp_overlay_draw_yuv_host(&im, list.data(), (int)list.size(), opacity, thickness));
}

/// The same on an HDR frame (utility/data.hpp, hdr): a P010 / I010 frame is painted with graphics white at `h.white_nits` in the frame's transfer
/// function (hp_yuv_colours_hdr) instead of full-scale code values; an 8-bit frame is painted as above.
inline void draw_humans(yuv_frame& frame, const std::vector<human_t>& humans, const hdr& h, float opacity = 1, int thickness = 0, void* stream = nullptr)
{
    const auto list = detail::to_c_humans(humans);
    const hp_yuv_image im = frame.image();
    const hp_hdr_desc d = h.c_form();
    if (frame.on_device) {
        hp_overlay* o = detail::overlay_handle(list.size());
        detail::overlay_check(hp_overlay_set_transfer(o, &d));
        const int rc = hp_overlay_draw_yuv(o, &im, list.data(), (int)list.size(), opacity, thickness, stream);
        hp_overlay_set_transfer(o, nullptr); // the thread's handle serves the SDR overloads too
        detail::overlay_check(rc);
    } else
        detail::overlay_check(hp_overlay_draw_yuv_host_hdr(&im, &d, list.data(), (int)list.size(), opacity, thickness));
}

inline void draw_humans(const device_bgr& picture, const std::vector<human_t>& humans, float opacity = 1, int thickness = 0, void* stream = nullptr)
{
    const auto list = detail::to_c_humans(humans);
    detail::overlay_check(hp_overlay_draw_u8c3(detail::overlay_handle(list.size()), picture.ptr, picture.width, picture.height,
        picture.stride ? picture.stride : picture.width * 3, list.data(), (int)list.size(), opacity, thickness, stream));
}

/// Addition: upright input (utility/data.hpp, orientation).  `humans` are in the UPRIGHT frame's normalised coordinates - what an engine or a stream
/// with set_orientation(o) returns - and the picture is the frame as it is STORED: the records go through to_stored, then the overload above.
inline void draw_humans(yuv_frame& frame, std::vector<human_t> humans, const orientation& o, float opacity = 1, int thickness = 0, void* stream = nullptr)
{
    to_stored(humans, o);
    draw_humans(frame, humans, opacity, thickness, stream);
}
inline void draw_humans(yuv_frame& frame, std::vector<human_t> humans, const orientation& o, const hdr& h, float opacity = 1, int thickness = 0,
    void* stream = nullptr)
{
    to_stored(humans, o);
    draw_humans(frame, humans, h, opacity, thickness, stream);
}
inline void draw_humans(const device_bgr& picture, std::vector<human_t> humans, const orientation& o, float opacity = 1, int thickness = 0,
    void* stream = nullptr)
{
    to_stored(humans, o);
    draw_humans(picture, humans, opacity, thickness, stream);
}

} // namespace hyperpose
