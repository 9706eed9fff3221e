// hyperpose::redact_humans — addition: the heads or the whole persons of a frame's humans pixelated or blacked out in a video frame where it
// lies, in the frame's own layout and on its own code values (hp_redact_*, include/hp_hip.h), before the frame is encoded, stored or shown.
// The write-back counterpart of draw_humans (overlay.hpp): a yuv_frame with `on_device` set, or a device_bgr picture, is redacted by one kernel
// launch on `stream` (asynchronous, stream-ordered); a yuv_frame in host memory by the library's host twin, which gives the same bytes.  The
// picture is defined by exact integer rules (DESIGN.md 1.1 "Redaction"): a disc per head, or a rectangle per person and the head disc, grown by
// `margin`; every `cell` x `cell` cell of the frame a region reaches is rewritten whole, with its per-channel mean or with black.  Humans are in
// the FRAME's normalised coordinates (after resume_ratio).  Errors of the C ABI (bad layout, an odd cell or one outside 2 .. 128, a margin
// outside (0, 8], frames over 8192 x 8192) throw std::logic_error.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "data.hpp"
#include "human.hpp"
#include "overlay.hpp"

namespace hyperpose {

struct redaction {
    enum { head = HP_REDACT_HEAD, body = HP_REDACT_BODY };
    enum { pixelate = HP_REDACT_PIXELATE, black = HP_REDACT_BLACK };
    int what = head;
    int effect = pixelate;
    int cell = 16;
    float margin = 1;
};

namespace detail {
    inline void redact_check(int rc)
    {
        if (rc < HP_OK)
            throw std::logic_error(std::string("hyperpose::redact_humans: ") + hp_last_error());
    }
    // the calling thread's hp_redact handle (thread_handle, overlay.hpp)
    inline hp_redact* redact_handle(size_t n_regions)
    {
        return thread_handle<hp_redact, hp_redact_create, hp_redact_destroy>(n_regions, 128, "hyperpose::redact_humans");
    }
    inline std::vector<hp_redact_region> redact_regions(const std::vector<human_t>& humans, int w, int h, const redaction& r)
    {
        const auto list = to_c_humans(humans);
        std::vector<hp_redact_region> regions(2 * list.size() + 1);
        const int n = hp_redact_regions(list.data(), (int)list.size(), w, h, r.what, r.margin, regions.data(), (int)regions.size());
        redact_check(n);
        regions.resize((size_t)n);
        return regions;
    }
} // namespace detail

/// `frame.plane[]` is WRITTEN (the struct declares it const because the engine only reads it)
inline void redact_humans(yuv_frame& frame, const std::vector<human_t>& humans, const redaction& r = {}, void* stream = nullptr)
{
    const auto regions = detail::redact_regions(humans, frame.width, frame.height, r);
    const hp_yuv_image im = frame.image();
    if (frame.on_device)
        detail::redact_check(hp_redact_yuv(detail::redact_handle(regions.size()), &im, regions.data(), (int)regions.size(), r.effect, r.cell, stream));
    else
        detail::redact_check(hp_redact_yuv_host(&im, regions.data(), (int)regions.size(), r.effect, r.cell));
}

inline void redact_humans(const device_bgr& picture, const std::vector<human_t>& humans, const redaction& r = {}, void* stream = nullptr)
{
    const auto regions = detail::redact_regions(humans, picture.width, picture.height, r);
    detail::redact_check(hp_redact_u8c3(detail::redact_handle(regions.size()), picture.ptr, picture.width, picture.height,
        picture.stride ? picture.stride : picture.width * 3, regions.data(), (int)regions.size(), r.effect, r.cell, stream));
}

/// Upright input (utility/data.hpp, orientation): `humans` are in the UPRIGHT frame's normalised coordinates and the picture is the frame as it is
/// STORED: the records go through to_stored, then the overload above.
inline void redact_humans(yuv_frame& frame, std::vector<human_t> humans, const orientation& o, const redaction& r = {}, void* stream = nullptr)
{
    to_stored(humans, o);
    redact_humans(frame, humans, r, stream);
}
inline void redact_humans(const device_bgr& picture, std::vector<human_t> humans, const orientation& o, const redaction& r = {}, void* stream = nullptr)
{
    to_stored(humans, o);
    redact_humans(picture, humans, r, stream);
}

} // namespace hyperpose
