// Plan of the KAD permutation sweep (fad_kad_permutation_sweep, kad.hip) and its aggregation (fad_kad_aggregate) -- plain C++, shared
// by the host's launch plan, the CPU test of the coverage (tests/native_cpu/kad_perm_sweep_cover.cpp) and the stand-alone check of the
// aggregation (tests/native_cpu/kad_aggregate_check.cpp).  DESIGN.md 4.13.
//
// The pass of kad_perm_tiles.h walks Z's triangle once per group of labelling words.  The pair GEMM of a tile does not depend on sigma,
// so a walk of the sweep carries `nb` bandwidths times `nw` words: kad_perm_sweep_kernel<NB> keeps the same kPermWords float64 partials
// per lane, as NB rows of kPermWords / NB words.  n_bw bandwidths are cut into runs of NB (the last one shorter); a run of g bandwidths
// takes the smallest kernel that holds it (perm_sweep_kernel_nb: 1 is kad_perm_kernel itself, 3 runs in the kernel of 4 with its fourth
// row idle), and the W words of the call are cut for that kernel into as few balanced groups as there must be.  NB is the one of 1, 2, 4
// that gives the fewest walks, the smaller at a tie: about W n_bw / kPermWords of them whichever it is, and exactly one walk per
// bandwidth in kad_perm_kernel itself when the labellings fill kPermWords words (P = 992 .. 1023).  A launch takes a run of consecutive
// tiles of one walk, at most tiles_per_launch_for(depth, f32, perm_epilogue(kernel_nb * nw)) of them.
#pragma once

#include "kad_perm_tiles.h"

#include <algorithm>
#include <vector>

namespace fad {
namespace kad {

constexpr int kPermSweepMax = 16;              // bandwidths per call (FAD_KAD_PERM_MAX_BANDWIDTHS)
constexpr int kPermSweepNB = 4;                // the widest kernel instantiated (2 and 4)

// the kernel (its NB) that runs g <= kPermSweepNB bandwidths in one walk, and the words a walk of it holds per bandwidth
KAD_HD inline int perm_sweep_kernel_nb(int g) { return g <= 1 ? 1 : g <= 2 ? 2 : 4; }
KAD_HD inline int64_t perm_sweep_words(int kernel_nb) { return kPermWords / kernel_nb; }

// walks of the whole call when the bandwidths are cut into runs of NB
inline int64_t perm_sweep_walk_count(int n_bw, int64_t W, int NB) {
    int64_t walks = 0;
    for (int b0 = 0; b0 < n_bw; b0 += NB) {
        const int64_t cap = perm_sweep_words(perm_sweep_kernel_nb(n_bw - b0 < NB ? n_bw - b0 : NB));
        walks += (W + cap - 1) / cap;
    }
    return walks;
}

// NB of the call: the fewest walks, the smaller NB at a tie
inline int perm_sweep_nb(int n_bw, int64_t W) {
    int best = 1;
    for (int NB = 2; NB <= kPermSweepNB; NB *= 2)
        if (perm_sweep_walk_count(n_bw, W, NB) < perm_sweep_walk_count(n_bw, W, best)) best = NB;
    return best;
}

// one triangle walk: bandwidths [b0, b0 + nb) in the kernel of `kernel_nb`, words [w0, w0 + nw) -- word group `wg` of the run's `wgs`
struct PermSweepWalk { int b0, nb, kernel_nb; int64_t w0, nw, wg, wgs; };

inline std::vector<PermSweepWalk> perm_sweep_walks(int n_bw, int64_t labellings) {
    std::vector<PermSweepWalk> out;
    const int64_t W = perm_words(labellings);
    const int NB = perm_sweep_nb(n_bw, W);
    for (int b0 = 0; b0 < n_bw; b0 += NB) {
        const int nb = n_bw - b0 < NB ? n_bw - b0 : NB, k = perm_sweep_kernel_nb(nb);
        const int64_t cap = perm_sweep_words(k), wgs = (W + cap - 1) / cap;
        for (int64_t g = 0; g < wgs; ++g) {
            const int64_t w0 = perm_group_start(g, wgs, W);
            out.push_back(PermSweepWalk{b0, nb, k, w0, perm_group_start(g + 1, wgs, W) - w0, g, wgs});
        }
    }
    return out;
}

struct PermSweepLaunch { int64_t walk, u0, cnt, grid; };

// host only: every launch of the sweep over TZ row blocks, walk by walk; walk_slots[i] = the slots of walk i (its widest launch's grid)
inline std::vector<PermSweepLaunch> perm_sweep_launches(int64_t TZ, const std::vector<PermSweepWalk>& walks, int64_t depth, bool f32,
                                                        int64_t cap, std::vector<int64_t>* walk_slots = nullptr) {
    std::vector<PermSweepLaunch> out;
    const int64_t tiles = tri_tiles(TZ);
    if (walk_slots) walk_slots->assign(walks.size(), 0);
    for (size_t i = 0; i < walks.size(); ++i) {
        const int64_t per = tiles_per_launch_for(depth, f32, perm_epilogue(walks[i].kernel_nb * walks[i].nw));
        int64_t slots = 0;
        for (const Launch& l : launches(tiles, per, cap)) {
            out.push_back(PermSweepLaunch{(int64_t)i, l.u0, l.cnt, l.grid});
            slots = l.grid > slots ? l.grid : slots;
        }
        if (walk_slots) (*walk_slots)[i] = slots;
    }
    return out;
}

// The min-p aggregate over bandwidths (fad_kad_aggregate): t is [n_bw][n_lab], labelling 0 the observed one.
//   p_b(j) = #{i : t_b(i) >= t_b(j)} / n_lab,  p_values[b] = p_b(0),  m(j) = min_b p_b(j),  p_aggregated = #{j : m(j) <= m(0)} / n_lab.
// Pure counting on integers: the counts are compared, not the quotients.  A NaN entry compares false both ways.
inline void perm_aggregate(const double* t, int n_bw, int64_t n_lab, double* p_values, double* p_aggregated) {
    std::vector<int64_t> least((size_t)n_lab, n_lab + 1);
    std::vector<double> sorted((size_t)n_lab);
    for (int b = 0; b < n_bw; ++b) {
        const double* tb = t + (int64_t)b * n_lab;
        for (int64_t i = 0; i < n_lab; ++i) sorted[(size_t)i] = tb[i];
        // ascending, NaNs last: #{i : t(i) >= x} = the finite entries from the first one >= x on
        int64_t finite = 0;
        for (int64_t i = 0; i < n_lab; ++i)
            if (sorted[(size_t)i] == sorted[(size_t)i]) sorted[(size_t)finite++] = sorted[(size_t)i];
        std::sort(sorted.begin(), sorted.begin() + finite);
        for (int64_t j = 0; j < n_lab; ++j) {
            int64_t lo = 0, hi = finite;                                              // first index with sorted >= tb[j]
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (sorted[(size_t)mid] >= tb[j]) hi = mid; else lo = mid + 1;
            }
            const int64_t ge = tb[j] == tb[j] ? finite - lo : 0;
            if (j == 0 && p_values) p_values[b] = (double)ge / (double)n_lab;
            if (ge < least[(size_t)j]) least[(size_t)j] = ge;
        }
    }
    int64_t le = 0;
    for (int64_t j = 0; j < n_lab; ++j) le += least[(size_t)j] <= least[0];
    if (p_aggregated) *p_aggregated = (double)le / (double)n_lab;
}

}  // namespace kad
}  // namespace fad
