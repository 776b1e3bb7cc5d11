// Work units of the KAD uncertainty pass (fad_kad_uncertainty, kad.hip) -- plain C++, shared by the device code, the host's launch
// plan and the CPU test of the coverage (tests/native_cpu/kad_unc_tiles_cover.cpp).  DESIGN.md 4.9.
//
// The baseline X (n rows) and the S evaluation sets are packed into one image Z, each starting on a 128-row tile boundary: X takes the
// row blocks [0, TX), set s the blocks [blk[s], blk[s + 1]) (blk[0] = TX, blk[S] = TZ).  Every row sum the estimate needs is a column
// sum of Z x Z over one row segment:
//   column block J of X:     rows of X (K_XX, self excluded) and rows of every set s (K_YsX)   -> S + 1 segments
//   column block J of set s: rows of X (K_XYs) and rows of set s (K_YsYs, self excluded)       -> 2 segments
// so the pass walks K_XX once, every K_YsYs once and every cross product in both orientations, and a diagonal tile (I == J) lies in
// K_XX or a K_YsYs, where the pair of a row with itself is dropped by index.  A segment's row blocks are cut into units of at most
// `rr` blocks (one workgroup walks a unit, accumulating its 128 columns, then writes one float64 slot per column), so no unit's row
// run crosses a set.  Units are listed segment by segment: J = 0, 1, ... and inside a column block of X the segments X, set 0,
// set 1, ...; of a set's block X, then the set.  seg_start[k] .. seg_start[k + 1] are the units of segment k (unc_segment).
// A pass is cut into launches of whole units whose tiles stay under kad::tiles_per_launch_for(.., kUncEpilogue) (kad_tiles.h).
#pragma once

#include "kad_song_tiles.h"

#include <vector>

namespace fad {
namespace kad {

constexpr int kUncMaxSets = 64;
constexpr int64_t kUncUnits = 16384;    // the pass aims at about this many units: a few tens per workgroup slot of a full launch
// The column-sum epilogue with the self mask: per pair the exponential of the sums, a select, and a float32 add into the lane's
// column (DESIGN.md 4.7 measured kad_cols_kernel's epilogue at 0.94x of the sum pass's pair rate), weighed a little above kSumEpilogue.
constexpr int64_t kUncEpilogue = 160;

// first row block of every set (S + 1 entries; blk[S] = TZ, the blocks of Z); X holds [0, blocks(n))
inline std::vector<int64_t> unc_blocks(int64_t n, const int64_t* ms, int S) {
    std::vector<int64_t> blk((size_t)S + 1);
    blk[0] = blocks(n);
    for (int s = 0; s < S; ++s) blk[(size_t)s + 1] = blk[(size_t)s] + blocks(ms[s]);
    return blk;
}

// segments of the pass: TX (S + 1) + 2 (TZ - TX)
KAD_HD inline int64_t unc_segments(int64_t TX, int64_t TZ, int S) { return TX * (S + 1) + 2 * (TZ - TX); }

// segment of column block J and row group g (0: X, s + 1: set s); J >= TX lies in set `own`, whose only groups are 0 and own + 1
KAD_HD inline int64_t unc_segment(int64_t J, int g, int64_t TX, int S) {
    return J < TX ? J * (S + 1) + g : TX * (S + 1) + 2 * (J - TX) + (g != 0);
}

// tiles of the pass: K_XX, both orientations of every cross product, every K_YsYs
inline int64_t unc_tiles(const std::vector<int64_t>& blk) {
    const int S = (int)blk.size() - 1;
    const int64_t TX = blk[0], TZ = blk[(size_t)S];
    int64_t t = TX * TX + 2 * TX * (TZ - TX);
    for (int s = 0; s < S; ++s) t += (blk[(size_t)s + 1] - blk[(size_t)s]) * (blk[(size_t)s + 1] - blk[(size_t)s]);
    return t;
}

// row blocks per unit: about kUncUnits units over the pass's tiles, and short enough that one launch holds at least kUncLaunchUnits
// of them (more than the device's workgroup slots; as kPrdcLaunchUnits)
constexpr int64_t kUncLaunchUnits = 2048;
KAD_HD inline int64_t unc_rows_per_unit(int64_t tiles, int64_t per_launch) {
    int64_t rr = (tiles + kUncUnits - 1) / kUncUnits;
    const int64_t cap = per_launch / kUncLaunchUnits;
    if (rr > cap) rr = cap;
    return rr < 1 ? 1 : rr;
}

// the units of the pass in segment order and seg_start (unc_segments + 1 entries)
inline void unc_units(const std::vector<int64_t>& blk, int64_t rr, std::vector<Unit>* units, std::vector<int64_t>* seg_start) {
    const int S = (int)blk.size() - 1;
    const int64_t TX = blk[0];
    units->clear();
    seg_start->clear();
    auto segment = [&](int64_t J, int64_t r0, int64_t r1) {
        seg_start->push_back((int64_t)units->size());
        for (int64_t I0 = r0; I0 < r1; I0 += rr) units->push_back(Unit{J, I0, I0 + rr < r1 ? I0 + rr : r1});
    };
    for (int64_t J = 0; J < TX; ++J) {
        segment(J, 0, TX);
        for (int s = 0; s < S; ++s) segment(J, blk[(size_t)s], blk[(size_t)s + 1]);
    }
    for (int s = 0; s < S; ++s)
        for (int64_t J = blk[(size_t)s]; J < blk[(size_t)s + 1]; ++J) {
            segment(J, 0, TX);
            segment(J, blk[(size_t)s], blk[(size_t)s + 1]);
        }
    seg_start->push_back((int64_t)units->size());
}

// units per launch of the pass: whole units of at most rr tiles under the launch's tile budget (host only: kad::launch_budget)
inline int64_t unc_units_per_launch(int64_t rr, int64_t depth, bool f32) {
    const int64_t t = tiles_per_launch_for(depth, f32, kUncEpilogue) / rr;
    return t < 1 ? 1 : t;
}

}  // namespace kad
}  // namespace fad
