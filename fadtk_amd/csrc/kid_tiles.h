// Work units of the subset protocol of the polynomial-kernel distance (fad_kid_subsets, kad.hip) -- plain C++, shared by the device
// code, the host's launch plan and the CPU test of the coverage (tests/native_cpu/kid_tiles_cover.cpp).  DESIGN.md 4.15.
//
// Subset q is s gathered rows of x and s gathered rows of y, each in an image of its own of s_pad = 128 * T rows (T = blocks(s)).
// Its pair space is three independent blocks of 128 x 128 tiles, and one tile is one work unit that writes one float64:
//   XX  the upper triangle of x's T x T grid, tri_tiles(T) units, a diagonal tile counting only column > row (kad_tiles.h);
//   YY  the same of y;
//   XY  the T x T square of x's rows against y's, every pair, the diagonal i == j included.
// A subset has units_per_subset(T) = T (T + 1) + T^2 units, numbered XX first, then YY, then XY; subset q of a group takes the units
// [q * U, (q + 1) * U).  A pass over a group of subsets is cut into launches of consecutive units by kad::launches and mapped to
// workgroups and XCDs by kad::slot_tile, exactly as kad_tiles.h maps tiles, so one XCD's stretch holds whole subsets' worth of
// consecutive units and re-reads a subset's 2 * s_pad rows from its own L2.
// The images of all subsets may not fit: plan() cuts the subsets into groups whose two images stay under a byte budget; the groups go
// through the workspace one after another.  A unit's value depends on its tile alone, so the grouping never shows in a result.
#pragma once

#include "kad_tiles.h"

#include <vector>

namespace fad {
namespace kid {

using kad::kTile;

enum Block { XX = 0, YY = 1, XY = 2 };

struct Unit { int64_t q; int block; int64_t I, J; };

KAD_HD inline int64_t units_per_subset(int64_t T) { return T * (T + 1) + T * T; }

// unit u of a group -> (subset q of the group, block, tile I, J); T = blocks(subset_size)
KAD_HD inline Unit unit_of(int64_t u, int64_t T) {
    const int64_t U = units_per_subset(T), tt = kad::tri_tiles(T), q = u / U;
    int64_t w = u % U;
    if (w < 2 * tt) {
        const int block = w < tt ? XX : YY;
        const kad::Tile t = kad::tri_tile(block == XX ? w : w - tt, T);
        return Unit{q, block, t.I, t.J};
    }
    w -= 2 * tt;
    return Unit{q, XY, w / T, w % T};
}

// the unit of (q, block, I, J): the inverse of unit_of (I <= J in XX and YY)
KAD_HD inline int64_t unit_index(int64_t q, int block, int64_t I, int64_t J, int64_t T) {
    const int64_t tt = kad::tri_tiles(T), base = q * units_per_subset(T);
    if (block == XY) return base + 2 * tt + I * T + J;
    return base + (block == YY ? tt : 0) + kad::tri_row_start(I, T) + (J - I);
}

// the pair at local (r, c) of a unit's tile, counted or not: rows of the subset only; XX / YY: j > i; XY: every pair
KAD_HD inline bool pair_counted(int block, int64_t I, int64_t J, int r, int c, int64_t s) {
    return kad::pair_counted(block != XY, I, J, r, c, s, s);
}

// bytes of a group's two images and their row markers
KAD_HD inline int64_t subset_bytes(int64_t subset_size, int64_t row_bytes) {
    return 2 * kad::blocks(subset_size) * kTile * (row_bytes + (int64_t)sizeof(float));
}

// host only: the groups [q0, q0 + count) of subsets whose images stay under `budget` bytes (one subset per group where even one
// subset is over it)
struct Group { int64_t q0, count; };
inline std::vector<Group> plan(int64_t n_subsets, int64_t subset_size, int64_t row_bytes, int64_t budget) {
    int64_t per = budget / subset_bytes(subset_size, row_bytes);
    if (per < 1) per = 1;
    std::vector<Group> out;
    for (int64_t q0 = 0; q0 < n_subsets; q0 += per) out.push_back(Group{q0, per < n_subsets - q0 ? per : n_subsets - q0});
    return out;
}

// The byte budget fad_kid_subsets gives plan(): 128 MiB.  The usual protocol (100 subsets of 1000 rows) takes 50 MiB of images at
// D = 128 and 200 MiB at D = 512 in fp16, so one or two groups; a group of one subset at the largest rows (s_pad 2^31 is far off) is
// never refused.  Small enough that a test crosses it with a few hundred rows (float32, D = 1280, s = 129: 51 subsets a group).
constexpr int64_t kImageBudget = (int64_t)128 << 20;

}  // namespace kid
}  // namespace fad
