// Work units of the per-song KAD passes (fad_kad_individual, kad.hip) -- plain C++, shared by the device code, the host's launch
// plan and the CPU test of the coverage (tests/native_cpu/kad_song_tiles_cover.cpp).  DESIGN.md 4.7.
//
// Y is the concatenation of the songs, M rows; song s is rows [offsets[s], offsets[s + 1]).  Both passes produce per-COLUMN sums
// (one column = one song row), so a work unit is a column block J and a run of row blocks [I0, I1) that one workgroup walks,
// accumulating its columns in registers, and then writes one float64 slot per column:
//   cross  (X x Y): the rectangle of TI x TJ tiles; unit u = R * TJ + J takes the row blocks [R * rr, min(TI, (R + 1) * rr)) of
//          column block J, so consecutive units (and one XCD's stretch of them) stream the same X rows.  Slot row R.
//   band   (Y x Y, pairs i < j inside one song): column block J needs the row blocks from the block of the first row of the song that
//          holds row J * 128 up to J itself; that band is cut into pieces of at most kBandPiece blocks, one unit (and one slot row
//          of 128 columns) each, so a long song's band spreads over many workgroups.  Units are listed column block by column
//          block, and band_start[J] .. band_start[J + 1] are those of J.
// A pass is cut into launches of whole units whose tiles stay under kad::tiles_per_launch (kad_tiles.h); inside a launch the
// units map to workgroups and XCDs exactly as kad_tiles.h maps tiles.
#pragma once

#include "kad_tiles.h"

#include <vector>

namespace fad {
namespace kad {

constexpr int64_t kCrossUnits = 8192;   // the cross pass aims at this many units (a few per workgroup slot of a full launch)
constexpr int64_t kBandPiece = 32;      // row blocks per band unit at most

struct Unit { int64_t J, I0, I1; };

// row blocks per cross unit: enough units to fill the device, and never more tiles than one launch may take
KAD_HD inline int64_t cross_rows_per_unit(int64_t TI, int64_t TJ, int64_t per_launch) {
    int64_t nr = (kCrossUnits + TJ - 1) / TJ;
    if (nr > TI) nr = TI;
    if (nr < 1) nr = 1;
    int64_t rr = (TI + nr - 1) / nr;
    return rr > per_launch ? per_launch : rr;
}
KAD_HD inline int64_t cross_ranges(int64_t TI, int64_t rr) { return (TI + rr - 1) / rr; }
KAD_HD inline Unit cross_unit(int64_t u, int64_t TI, int64_t TJ, int64_t rr) {
    const int64_t R = u / TJ, I0 = R * rr;
    return Unit{u % TJ, I0, I0 + rr < TI ? I0 + rr : TI};
}

// Units per launch of a pass whose units take at most `unit_tiles` tiles each (host only: kad::launch_budget).
inline int64_t units_per_launch(int64_t unit_tiles, int64_t depth, bool f32) {
    const int64_t t = tiles_per_launch(depth, f32) / (unit_tiles > 0 ? unit_tiles : 1);
    return t < 1 ? 1 : t;
}

// PRDC's radius (X x X, Y x Y) and cross (X x Y) passes use the cross map over their rectangles, with units short
// enough that one launch holds at least kPrdcLaunchUnits of them (at n = 10^6 the plain cross map would give a launch fewer units than
// the device has workgroup slots).  `per_launch` is kad::tiles_per_launch_for with the pass's epilogue weight.
constexpr int64_t kPrdcLaunchUnits = 2048;
KAD_HD inline int64_t prdc_rows_per_unit(int64_t TI, int64_t TJ, int64_t per_launch) {
    const int64_t cap = per_launch / kPrdcLaunchUnits;
    return cross_rows_per_unit(TI, TJ, cap < 1 ? 1 : cap);
}
KAD_HD inline int64_t prdc_units_per_launch(int64_t rr, int64_t per_launch) {
    const int64_t t = per_launch / rr;
    return t < 1 ? 1 : t;
}

// The pair (i, j) at local (r, c) of band tile (I, J), I <= J: counted when j > i and j lies before the end of i's song.
// `end_i` is offsets[song(i) + 1] for a row of Y, and 0 for a padding row (i >= M): songs are contiguous, so i < j < end_i is
// exactly "same song".  The kernel holds end_i - J * 128 per row and compares it to c.
KAD_HD inline bool band_pair_counted(int64_t I, int64_t J, int r, int c, int64_t end_i) {
    const int64_t j = J * kTile + c;
    return j < end_i && (I < J || c > r);
}

// the song that holds row `row` (offsets non-decreasing, offsets[0] = 0 <= row < offsets[n_songs]): the last s with offsets[s] <= row
KAD_HD inline int64_t song_of_row(const int64_t* offsets, int64_t n_songs, int64_t row) {
    int64_t lo = 0, hi = n_songs;                 // offsets[lo] <= row < offsets[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

// The band's units in order of J, and start[J] (TJ + 1 entries) -- M = offsets[n_songs] > 0.
inline void band_units(const int64_t* offsets, int64_t n_songs, std::vector<Unit>* units, std::vector<int64_t>* start) {
    const int64_t M = offsets[n_songs], TJ = blocks(M);
    units->clear();
    start->assign((size_t)TJ + 1, 0);
    for (int64_t J = 0; J < TJ; ++J) {
        (*start)[(size_t)J] = (int64_t)units->size();
        const int64_t lo = offsets[song_of_row(offsets, n_songs, J * kTile)] / kTile;
        for (int64_t I0 = lo; I0 <= J; I0 += kBandPiece) units->push_back(Unit{J, I0, I0 + kBandPiece < J + 1 ? I0 + kBandPiece : J + 1});
    }
    (*start)[(size_t)TJ] = (int64_t)units->size();
}

}  // namespace kad
}  // namespace fad
