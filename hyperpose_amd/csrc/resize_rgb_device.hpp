// resize_rgb_device.hpp — the `Taps` types (resize_device.hpp) of the packed 8-bit layouts hp_rgb_image names (rgb_formats.hpp): where the B, G, R of a
// source pixel come from.  Two of them:
//   rgb_taps     every layout: the pixel step and the byte offsets of B, G and R inside a pixel are kernel arguments, three byte loads per tap (GRAY8:
//                step 1 and three times offset 0)
//   rgb32_taps   the four 4-byte layouts: ONE aligned 32-bit load per tap, the channels taken out by shifts that are kernel arguments (8 * the byte
//                offset: the words are little-endian)
// What is read.  resize_pixel() asks only for pixels (x, y) with 0 <= x < width and 0 <= y < height of the frame or region it was given (it clamps the
// taps at the edges, reads the second column only where it exists, and the area mode runs only where the source is exactly twice the inner size);
// oriented_taps<> maps such a pixel to another pixel of the stored frame.  rgb_taps reads bytes x * step + {b, g, r} of row y with every offset < step,
// rgb32_taps bytes 4 x .. 4 x + 3: both inside the first width * pixel_bytes bytes of the row, whatever the stride is.  The 24-bit layouts have no
// wider load: a 32-bit load at the last pixel of a row would read one byte beyond it.  rgb32_taps needs what hp_rgb::check(kernel_access) demands:
// an address and a stride that are multiples of 4.
#pragma once
#include "resize_oriented_device.hpp"
#include "rgb_formats.hpp"

namespace hp_resize {

struct rgb_taps {
    const uint8_t* src;
    int stride, step;
    int ob, og, orr;
    __device__ __forceinline__ void load(int x, int y, int (&c)[3]) const
    {
        const uint8_t* s = src + (size_t)y * stride + x * step;
        c[0] = s[ob], c[1] = s[og], c[2] = s[orr];
    }
    __device__ __forceinline__ rgb_taps at(int rx, int ry) const { return rgb_taps{ src + (size_t)ry * stride + rx * step, stride, step, ob, og, orr }; }
};

struct rgb32_taps {
    const uint8_t* src;
    int stride;
    int sb, sg, sr; // bit shifts of B, G, R inside the little-endian word
    __device__ __forceinline__ void load(int x, int y, int (&c)[3]) const
    {
        const uint32_t w = *(const uint32_t*)(src + (size_t)y * stride + x * 4);
        c[0] = (w >> sb) & 255, c[1] = (w >> sg) & 255, c[2] = (w >> sr) & 255;
    }
    __device__ __forceinline__ rgb32_taps at(int rx, int ry) const { return rgb32_taps{ src + (size_t)ry * stride + rx * 4, stride, sb, sg, sr }; }
};

inline rgb_taps byte_taps_of(const hp_rgb_image& im, const hp_rgb::layout& l)
{
    return rgb_taps{ (const uint8_t*)im.data, im.stride, l.pixel_bytes, l.b, l.g, l.r };
}
inline rgb32_taps word_taps_of(const hp_rgb_image& im, const hp_rgb::layout& l)
{
    return rgb32_taps{ (const uint8_t*)im.data, im.stride, 8 * l.b, 8 * l.g, 8 * l.r };
}

} // namespace hp_resize
