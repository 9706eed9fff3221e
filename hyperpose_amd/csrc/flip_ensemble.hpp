// flip_ensemble.hpp - the flip ensemble of PAF networks (include/hp_hip.h "flip ensemble"): the network runs on a frame and on its
// left-right flip, the flipped maps are flipped back - left and right channels swapped, the x component of the part-affinity fields negated - and
// the two sets of maps are averaged before parsing.  The ONE definition of the merge, for n frames whose 2n maps [C][H][W] lie back to back,
// frames first, their flips behind them:
//
//     a = maps[f][c][y][x]      b = maps[n + f][perm[c]][y][W - 1 - x]
//     maps[f][c][y][x] = sign[c] > 0 ? 0.5f * (a + b) : 0.5f * (a - b)          (fp32, no fused operation; one addition, one multiplication)
//
// in place: every element reads its own location and a map that is never written.  Because a + b = b + a and 0.5f * (a - b) = -(0.5f * (b - a))
// hold bit for bit, the ensemble E is exactly equivariant whenever perm is an involution with sign[perm[c]] == sign[c]:
//     E(flip(x))[perm[c]](W - 1 - p) * sign[c] == E(x)[c](p)
// - in every bit but one: where a == b exactly, a negated channel holds 0.5f * (a - b) = +0 on one side and -(+0) = -0 on the other (no f with
// f(a, b) == -f(b, a) in every bit exists at a == b).  The two zeros compare equal and no parser tells them apart.
//
// The COCO tables are derived (hp_flip_tables_coco) from the two tables the PAF parser reads, restated here as overlay.hpp restates COCO_PAIRS:
// the limbs as pairs of parts (c_pairs, paf_parser.hip) and the two PAF channels of every limb (c_pairs_net), of which the first is the one the
// limb integral pairs with the x direction.
#pragma once
#include "hp_hip.h"

namespace hp_flip {

constexpr int MAX_C = 256; // the merge's tables travel by value in the kernel's arguments

constexpr int COCO_PAIRS[HP_COCO_N_PAIRS][2] = { { 1, 2 }, { 1, 5 }, { 2, 3 }, { 3, 4 }, { 5, 6 }, { 6, 7 }, { 1, 8 }, { 8, 9 }, { 9, 10 }, { 1, 11 },
    { 11, 12 }, { 12, 13 }, { 1, 0 }, { 0, 14 }, { 14, 16 }, { 0, 15 }, { 15, 17 }, { 2, 16 }, { 5, 17 } };
constexpr int COCO_PAIRS_NET[HP_COCO_N_PAIRS][2] = { { 12, 13 }, { 20, 21 }, { 14, 15 }, { 16, 17 }, { 22, 23 }, { 24, 25 }, { 0, 1 }, { 2, 3 },
    { 4, 5 }, { 6, 7 }, { 8, 9 }, { 10, 11 }, { 28, 29 }, { 30, 31 }, { 34, 35 }, { 32, 33 }, { 36, 37 }, { 18, 19 }, { 26, 27 } };
// a person's left and right: nose (0) and neck (1) are their own mirror image
constexpr int COCO_PART_FLIP[HP_COCO_N_PARTS] = { 0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16 };

} // namespace hp_flip
