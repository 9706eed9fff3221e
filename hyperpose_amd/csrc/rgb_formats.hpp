// rgb_formats.hpp — the ONE host-side description of the packed 8-bit layouts hp_rgb_image names (include/hp_hip.h, "packed RGB and grey frames"):
// how many bytes a pixel has and at which byte of it B, G and R lie.  The rule, restated from the header: memory order is as the name reads (BGRA32 is
// bytes B, G, R, A), the fourth byte is ignored, GRAY8 gives B = G = R = the sample.  Shared by the front end (resize_rgb.hip: argument checks and the
// kernels' addressing), the pipeline (pipeline.cpp: packing a host frame for upload) and the host twin hp_rgb_to_bgr_host.  Pure: it needs nothing but
// hp_hip.h and the standard headers and compiles with a plain C++ compiler (tests/cpp/rgb_formats.cpp uses it so); `validate` is only declared here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/hp_hip.h"

namespace hp_rgb {

struct layout {
    const char* name;
    int pixel_bytes; // 1, 3 or 4
    int b, g, r;     // byte offsets of the three channels inside a pixel
};

inline const layout* layout_of(int format)
{
    static const layout table[] = {
        { "HP_RGB_BGR24", 3, 0, 1, 2 }, { "HP_RGB_RGB24", 3, 2, 1, 0 }, { "HP_RGB_BGRA32", 4, 0, 1, 2 }, { "HP_RGB_RGBA32", 4, 2, 1, 0 },
        { "HP_RGB_ARGB32", 4, 3, 2, 1 }, { "HP_RGB_ABGR32", 4, 1, 2, 3 }, { "HP_RGB_GRAY8", 1, 0, 0, 0 },
    };
    return format >= 0 && format < (int)(sizeof(table) / sizeof(table[0])) ? &table[format] : nullptr;
}

// bytes of one tightly packed frame; 0 for an invalid format or size
inline size_t packed_bytes(int format, int w, int h)
{
    const layout* l = layout_of(format);
    return l && w > 0 && h > 0 ? (size_t)w * h * l->pixel_bytes : 0;
}

// Every rule of a description; 0, or -1 with the refusal in msg (it names the layout and the offending quantity).  `kernel_access`: a kernel reads the
// plane where it lies and fetches a 4-byte pixel as ONE aligned 32-bit word, so the 4-byte layouts need an address and a stride that are multiples of
// 4; false for host frames, which are re-packed byte by byte before a kernel sees them.
inline int check(const hp_rgb_image* im, const char* who, bool kernel_access, char* msg, size_t cap)
{
    if (!im)
        return snprintf(msg, cap, "%s: null image", who), -1;
    const layout* l = layout_of(im->format);
    if (!l)
        return snprintf(msg, cap, "%s: unknown format %d (HP_RGB_BGR24 .. HP_RGB_GRAY8)", who, im->format), -1;
    if (im->width <= 0 || im->height <= 0)
        return snprintf(msg, cap, "%s: %s: empty frame (%d x %d)", who, l->name, im->width, im->height), -1;
    if (!im->data)
        return snprintf(msg, cap, "%s: %s: data is null", who, l->name), -1;
    if ((int64_t)im->stride < (int64_t)im->width * l->pixel_bytes)
        return snprintf(msg, cap, "%s: %s: stride %d is smaller than a row (%lld bytes)", who, l->name, im->stride, (long long)im->width * l->pixel_bytes), -1;
    if (kernel_access && l->pixel_bytes == 4 && (im->stride % 4 != 0 || (uintptr_t)im->data % 4 != 0))
        return snprintf(msg, cap, "%s: %s: 4-byte pixels need an address and a stride that are multiples of 4 (address %% 4 = %d, stride %d)", who, l->name,
                   (int)((uintptr_t)im->data % 4), im->stride),
               -1;
    return 0;
}

// the whole frame as 8-bit BGR, rows bgr_stride bytes apart (>= width * 3; padding bytes are not written); the description must have passed check()
inline void to_bgr(const hp_rgb_image& im, uint8_t* bgr, int bgr_stride)
{
    const layout& l = *layout_of(im.format);
    for (int y = 0; y < im.height; ++y) {
        const uint8_t* s = (const uint8_t*)im.data + (size_t)y * im.stride;
        uint8_t* d = bgr + (size_t)y * bgr_stride;
        for (int x = 0; x < im.width; ++x, s += l.pixel_bytes, d += 3)
            d[0] = s[l.b], d[1] = s[l.g], d[2] = s[l.r];
    }
}

// check() reported through the library's error text: HP_OK or HP_ERR_INVALID (message set); `who` starts the message
int validate(const hp_rgb_image* im, const char* who, bool kernel_access = true);

} // namespace hp_rgb
