// yuv_formats.hpp — the ONE host-side description of the video layouts hp_yuv_image names (include/hp_hip.h): how many planes a format
// has, how wide a sample is, how its chroma is sub-sampled and how many bytes a row of each plane holds.  Shared by the front-end
// (resize_yuv_formats.hip: argument checks and the kernel's addressing), the pipeline (pipeline.cpp: packing a frame's planes for upload), the
// units that write into frames (overlay.hip, redact.hpp) and the HDR host twin (tonemap.cpp).  Pure: it needs nothing but hp_hip.h and the
// standard headers and compiles with a plain C++ compiler (tests/cpp/redact_rules.cpp uses it so); `validate` is only declared here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hp_hip.h"

namespace hp_yuv {

struct layout {
    const char* name;
    int planes;       // 1 packed, 2 semi-planar, 3 planar
    int sample_bytes; // 1, or 2 for the 10-bit formats (16-bit little-endian words)
    int sx, sy;       // luma pixel (x, y) uses chroma sample (x >> sx, y >> sy)
    int shift;        // 16-bit formats: value = (word >> shift) & 1023
};

inline const layout* layout_of(int format)
{
    static const layout table[] = {
        { "HP_YUV_NV12", 2, 1, 1, 1, 0 }, { "HP_YUV_I420", 3, 1, 1, 1, 0 }, { "HP_YUV_P010", 2, 2, 1, 1, 6 }, { "HP_YUV_I010", 3, 2, 1, 1, 0 },
        { "HP_YUV_NV16", 2, 1, 1, 0, 0 }, { "HP_YUV_I422", 3, 1, 1, 0, 0 }, { "HP_YUV_YUY2", 1, 1, 1, 0, 0 }, { "HP_YUV_UYVY", 1, 1, 1, 0, 0 },
        { "HP_YUV_I444", 3, 1, 0, 0, 0 },
    };
    return format >= 0 && format < (int)(sizeof(table) / sizeof(table[0])) ? &table[format] : nullptr;
}

inline bool size_ok(const layout& l, int w, int h) { return w > 0 && h > 0 && (w & ((1 << l.sx) - 1)) == 0 && (h & ((1 << l.sy) - 1)) == 0; }

// bytes of one row of plane k without padding, and the number of rows of that plane (the size must have passed size_ok)
inline size_t row_bytes(const layout& l, int k, int w)
{
    if (l.planes == 1)
        return (size_t)w * 2;
    if (k == 0)
        return (size_t)w * l.sample_bytes;
    const size_t cw = (size_t)(w >> l.sx) * l.sample_bytes;
    return l.planes == 2 ? cw * 2 : cw;
}
inline int rows(const layout& l, int k, int h) { return k == 0 ? h : h >> l.sy; }

// Where the samples of an image lie, in bytes: the address of the first Y, U and V sample (semi-planar and packed layouts: inside the same
// plane), the row strides, and the steps between horizontally neighbouring samples.  Luma pixel (x, y) is at y + y * y_stride + x * y_step,
// its chroma at u | v + (y >> sy) * c_stride + (x >> sx) * c_step (the V plane of a planar frame: + (y >> sy) * v_extra, its own pitch).
// The one statement of "YUY2 is Y0 U Y1 V, UYVY is U Y0 V Y1, semi-planar pairs are (U, V)": the resize kernels read through it
// (resize_yuv_formats.hip), the overlay kernels write through it (overlay.hip) and the redaction derives its channel patterns from it (redact.hpp).
struct sample_map {
    const uint8_t *y, *u, *v;
    int y_stride, c_stride, v_extra;
    int y_step, c_step;
};
inline sample_map map_samples(const hp_yuv_image& im, const layout& l)
{
    const uint8_t *p0 = (const uint8_t*)im.plane[0], *p1 = (const uint8_t*)im.plane[1], *p2 = (const uint8_t*)im.plane[2];
    sample_map m;
    m.y_stride = im.stride[0];
    if (l.planes == 1) {
        const bool yuy2 = im.format == HP_YUV_YUY2;
        m.y = p0 + (yuy2 ? 0 : 1), m.u = p0 + (yuy2 ? 1 : 0), m.v = p0 + (yuy2 ? 3 : 2);
        m.c_stride = im.stride[0], m.y_step = 2, m.c_step = 4, m.v_extra = 0;
    } else if (l.planes == 2) {
        m.y = p0, m.u = p1, m.v = p1 + l.sample_bytes;
        m.c_stride = im.stride[1], m.y_step = l.sample_bytes, m.c_step = 2 * l.sample_bytes, m.v_extra = 0;
    } else {
        m.y = p0, m.u = p1, m.v = p2;
        m.c_stride = im.stride[1], m.y_step = l.sample_bytes, m.c_step = l.sample_bytes, m.v_extra = im.stride[2] - im.stride[1];
    }
    return m;
}

// One sample of a frame in HOST memory, read and written bytewise: a host plane is not held to the kernels' alignment rule.  16-bit samples are
// little-endian words holding value << shift (the value is (word >> shift) & 1023; the bits outside it are stored as zero).
inline int host_get(const uint8_t* q, int sample_bytes, int shift) { return sample_bytes == 2 ? ((q[0] | (q[1] << 8)) >> shift) & 1023 : q[0]; }
inline void host_put(uint8_t* q, int sample_bytes, int shift, int v)
{
    if (sample_bytes == 2) {
        const int word = v << shift;
        q[0] = (uint8_t)(word & 255), q[1] = (uint8_t)(word >> 8);
    } else
        q[0] = (uint8_t)v;
}

// format, matrix, range, size, planes and strides of one image; `who` starts the message.  HP_OK or HP_ERR_INVALID (message set).
// `kernel_access`: a kernel reads (resize) or writes (overlay) the planes where they lie, so 16-bit words need even addresses and strides;
// false for host frames, which are re-packed byte by byte before a kernel sees them or are painted bytewise by the overlay's host twin
int validate(const hp_yuv_image* im, const char* who, bool kernel_access = true);

} // namespace hp_yuv
