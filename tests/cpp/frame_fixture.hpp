// What tests/cpp/overlay_api.cpp and tests/cpp/redact_api.cpp share: seeded noise for a frame's planes and three humans with missing parts and
// parts beyond the frame.
#pragma once
#include <hyperpose/hyperpose.hpp>

#include <vector>

static std::vector<uint8_t> noise(size_t n, unsigned seed, bool p010)
{
    std::vector<uint8_t> v(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i)
        s = s * 1664525u + 1013904223u, v[i] = (uint8_t)(s >> 24);
    if (p010)
        for (size_t i = 0; i + 1 < n; i += 2)
            v[i] &= 0xC0; // a P010 word holds its sample in the high ten bits
    return v;
}

// every human's parts lie within spread_x / 2, spread_y / 2 of its centre
static std::vector<hyperpose::human_t> some_humans(float spread_x, float spread_y)
{
    std::vector<hyperpose::human_t> out(3);
    unsigned s = 77;
    auto next = [&] { return (s = s * 1664525u + 1013904223u, (float)(s >> 8) / (float)(1 << 24)); };
    for (size_t i = 0; i < out.size(); ++i) {
        out[i].score = 1;
        const float cx = 0.2f + 0.3f * i, cy = 0.3f + 0.2f * i;
        for (int k = 0; k < hyperpose::COCO_N_PARTS; ++k)
            if (k % 5 != (int)i) // some parts missing
                out[i].parts[k] = hyperpose::body_part_t{ true, cx + spread_x * (next() - 0.5f), cy + spread_y * (next() - 0.5f), 1.f };
    }
    out[2].parts[3].x = 1.2f, out[2].parts[4].y = -0.1f; // beyond the frame
    return out;
}
