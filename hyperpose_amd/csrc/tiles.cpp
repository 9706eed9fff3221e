// tiles.cpp — the host side of tiled inference (include/hp_hip.h, "regions and tiles"): the planner that cuts a frame into overlapping,
// layout-aligned regions (hp_tile_plan), the way back from a region's normalised coordinates to the frame's (hp_humans_to_frame) and the
// merge that fuses the partial skeletons of a person who straddles a tile border (hp_humans_merge).  No device code and no reference
// counterpart (the reference squeezes every frame into one network input).  Integers and IEEE doubles only, evaluated in the order the
// header states, so that tests/tiles_ref.py can restate every rule in numpy and compare bytes; the unit is built with -ffp-contract=off.
// The lists are a few KB per frame: this runs on the thread that collects, next to the parsers' host tails.
#include "hp_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
int64_t align_down(int64_t v, int64_t a) { return v / a * a; }

// one axis of the plan: the tile size and the origin of tile i
void plan_axis(int W, int c, int overlap, int a, int& tw, int* x)
{
    const int64_t o = align_up(overlap, a);
    tw = (int)std::min<int64_t>(W, align_up((W + (int64_t)(c - 1) * o + c - 1) / c, a));
    for (int i = 0; i < c; ++i)
        x[i] = c == 1 ? 0 : i == c - 1 ? W - tw : (int)align_down((int64_t)i * (W - tw) / (c - 1), a);
}

struct extent {
    int m = 0; // present parts
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    double size() const { return m ? std::max(x1 - x0, y1 - y0) : 0.; }
};

extent extent_of(const hp_human& h, int fw, int fh)
{
    extent e;
    for (const auto& p : h.parts) {
        if (!p.has_value)
            continue;
        const double px = (double)p.x * fw, py = (double)p.y * fh;
        if (e.m++ == 0)
            e.x0 = e.x1 = px, e.y0 = e.y1 = py;
        else
            e.x0 = std::min(e.x0, px), e.x1 = std::max(e.x1, px), e.y0 = std::min(e.y0, py), e.y1 = std::max(e.y1, py);
    }
    return e;
}

} // namespace

namespace hp {

// hp_humans_merge without the capacity rule: the kept humans, in kept order (the pipeline's collect uses this form)
int merge_humans(const hp_human* in, const int32_t* region_of, int n, int fw, int fh, int min_common, double tol, std::vector<hp_human>& kept)
{
    kept.clear();
    HP_REQUIRE(n >= 0 && (n == 0 || (in && region_of)), HP_ERR_INVALID, "hp_humans_merge: null argument");
    HP_REQUIRE(fw > 0 && fh > 0, HP_ERR_INVALID, "hp_humans_merge: empty frame (%d x %d)", fw, fh);
    HP_REQUIRE(min_common >= 1 && tol >= 0., HP_ERR_INVALID, "hp_humans_merge: min_common %d (>= 1), tol %g (>= 0)", min_common, tol);
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) {
        HP_REQUIRE(region_of[i] >= 0 && region_of[i] < 64, HP_ERR_INVALID, "hp_humans_merge: human %d comes from region %d (0 .. 63)", i, region_of[i]);
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (in[a].score != in[b].score)
            return in[a].score > in[b].score;
        return region_of[a] < region_of[b]; // equal regions: stable = by index
    });
    std::vector<uint64_t> regions;
    for (const int i : order) {
        const hp_human& c = in[i];
        const uint64_t bit = (uint64_t)1 << region_of[i];
        const double sc = extent_of(c, fw, fh).size();
        size_t into = kept.size();
        for (size_t k = 0; k < kept.size(); ++k) {
            if (regions[k] & bit)
                continue;
            int m = 0;
            double sum = 0.;
            for (int j = 0; j < HP_COCO_N_PARTS; ++j) {
                const hp_body_part &pk = kept[k].parts[j], &pc = c.parts[j];
                if (!pk.has_value || !pc.has_value)
                    continue;
                const double dx = (double)pk.x * fw - (double)pc.x * fw, dy = (double)pk.y * fh - (double)pc.y * fh;
                sum += std::sqrt(dx * dx + dy * dy);
                ++m;
            }
            if (m < min_common)
                continue;
            const double sk = extent_of(kept[k], fw, fh).size();
            if (sum <= (tol * m) * std::max(sk, sc)) {
                into = k;
                break;
            }
        }
        if (into == kept.size()) {
            kept.push_back(c);
            regions.push_back(bit);
            continue;
        }
        for (int j = 0; j < HP_COCO_N_PARTS; ++j) {
            hp_body_part& pk = kept[into].parts[j];
            const hp_body_part& pc = c.parts[j];
            if (pc.has_value && (!pk.has_value || pc.score > pk.score))
                pk = pc;
        }
        regions[into] |= bit;
    }
    return HP_OK;
}

} // namespace hp

extern "C" {

int hp_tile_plan(const hp_tiling* t, int frame_w, int frame_h, int ax, int ay, hp_roi* out, int cap)
{
    HP_REQUIRE(t && out, HP_ERR_INVALID, "hp_tile_plan: null argument");
    HP_REQUIRE(frame_w > 0 && frame_h > 0 && ax >= 1 && ay >= 1, HP_ERR_INVALID, "hp_tile_plan: frame %d x %d, alignment %d, %d", frame_w, frame_h, ax, ay);
    HP_REQUIRE(frame_w % ax == 0 && frame_h % ay == 0, HP_ERR_INVALID, "hp_tile_plan: a %d x %d frame is no multiple of the alignment (%d, %d)", frame_w,
        frame_h, ax, ay);
    HP_REQUIRE(t->cols >= 1 && t->rows >= 1 && t->overlap_x >= 0 && t->overlap_y >= 0 && (t->with_full == 0 || t->with_full == 1), HP_ERR_INVALID,
        "hp_tile_plan: %d x %d tiles, overlap %d, %d, with_full %d", t->cols, t->rows, t->overlap_x, t->overlap_y, t->with_full);
    const int64_t count = (int64_t)t->cols * t->rows + t->with_full;
    HP_REQUIRE(t->cols <= 64 && t->rows <= 64 && count <= 64, HP_ERR_INVALID, "hp_tile_plan: %d x %d tiles%s are more than 64 regions", t->cols, t->rows,
        t->with_full ? " and the whole frame" : "");
    HP_REQUIRE(cap >= count, HP_ERR_CAPACITY, "hp_tile_plan: %d regions, room for %d", (int)count, cap);
    int tw = 0, th = 0, xs[64], ys[64];
    plan_axis(frame_w, t->cols, t->overlap_x, ax, tw, xs);
    plan_axis(frame_h, t->rows, t->overlap_y, ay, th, ys);
    int n = 0;
    if (t->with_full)
        out[n++] = hp_roi{ 0, 0, frame_w, frame_h };
    for (int r = 0; r < t->rows; ++r)
        for (int c = 0; c < t->cols; ++c)
            out[n++] = hp_roi{ xs[c], ys[r], tw, th };
    return n;
}

void hp_humans_to_frame(hp_human* humans, int n, const hp_roi* roi, int frame_w, int frame_h)
{
    if (!humans || !roi)
        return;
    for (int i = 0; i < n; ++i)
        for (auto& p : humans[i].parts)
            if (p.has_value) {
                p.x = (float)((roi->x + (double)p.x * roi->w) / frame_w);
                p.y = (float)((roi->y + (double)p.y * roi->h) / frame_h);
            }
}

int hp_humans_merge(const hp_human* in, const int32_t* region_of, int n, int frame_w, int frame_h, int min_common, double tol, hp_human* out, int cap)
{
    std::vector<hp_human> kept;
    HP_TRY(hp::merge_humans(in, region_of, n, frame_w, frame_h, min_common, tol, kept));
    HP_REQUIRE(cap >= 0 && (out || kept.empty() || cap == 0), HP_ERR_INVALID, "hp_humans_merge: null output");
    const int m = std::min<int>((int)kept.size(), cap);
    if (m > 0)
        memcpy(out, kept.data(), sizeof(hp_human) * m);
    HP_REQUIRE((int)kept.size() <= cap, HP_ERR_CAPACITY, "hp_humans_merge: %d humans kept, room for %d", (int)kept.size(), cap);
    return (int)kept.size();
}

} // extern "C"
