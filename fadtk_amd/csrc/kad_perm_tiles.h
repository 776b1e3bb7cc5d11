// Work units of the KAD permutation test (fad_kad_permutation_test, kad.hip) -- plain C++, shared by the device code, the host's launch
// plan and the CPU test of the coverage (tests/native_cpu/kad_perm_tiles_cover.cpp).  DESIGN.md 4.10.
//
// Z = [X; Y] is packed contiguously (N = n + m rows, TZ = blocks(N) row blocks).  The pass walks the upper triangle of Z's 128 x 128
// tiles (kad_tiles.h's tri_tile numbering) once per permutation group.  A group is up to kPermWords words of 32 labellings each: one
// workgroup holds a float64 partial per (labelling, lane half, wave) of its group in registers, so a group is as many labellings as fit
// without spills; the P + 1 labellings of a call (the observed one first) are cut into as few groups as there must be, of balanced
// width.  A unit is one (group, triangle tile); a launch takes a run of consecutive tiles of one group, at most
// tiles_per_launch_for(depth, f32, perm_epilogue(words)) of them, and its persistent workgroups keep their partials across all the
// tiles they walk (kad_tiles.h slot_tile).  At the launch's end workgroup w adds them into slot w of its group (32 * words float64
// values): the launches of a group run in order on one stream, so every slot is summed in the same order on every run.
#pragma once

#include "kad_tiles.h"

#include <vector>

namespace fad {
namespace kad {

constexpr int kPermWords = 32;                 // words (of 32 labellings) per group: 1024 labellings, 64 VGPRs of float64 partials
constexpr int64_t kPermMax = 65536;            // random labellings per call
// The permutation epilogue per tile and wave: the exponentials and f16 conversion of the kernel tile (about the sum pass's epilogue),
// then per word 8 v_mfma_f32_32x32x16_f16 (32 depth units, as the k loop counts a 16-bit MFMA) and about 100 VALU issues for the label
// fragments and masked sums.  Sized from the slowest launch measured.
constexpr int64_t kPermEpilogueBase = 192, kPermEpiloguePerWord = 128;
KAD_HD inline int64_t perm_epilogue(int64_t words) { return kPermEpilogueBase + kPermEpiloguePerWord * words; }

KAD_HD inline int64_t perm_words(int64_t labellings) { return (labellings + 31) / 32; }
KAD_HD inline int64_t perm_groups(int64_t words) { return (words + kPermWords - 1) / kPermWords; }
// group g of `ng` over `words` words: [perm_group_start(g), perm_group_start(g + 1)), balanced widths of at most kPermWords
KAD_HD inline int64_t perm_group_start(int64_t g, int64_t ng, int64_t words) { return g * words / ng; }

struct PermLaunch { int64_t group, w0, nw, u0, cnt, grid; };

// host only: every launch of the pass over TZ row blocks for `labellings` labellings (grid capped at `cap`), group by group;
// group_slots[g] = the slots of group g (its widest launch's grid)
inline std::vector<PermLaunch> perm_launches(int64_t TZ, int64_t labellings, int64_t depth, bool f32, int64_t cap,
                                             std::vector<int64_t>* group_slots = nullptr) {
    std::vector<PermLaunch> out;
    const int64_t W = perm_words(labellings), ng = perm_groups(W), tiles = tri_tiles(TZ);
    if (group_slots) group_slots->assign((size_t)ng, 0);
    for (int64_t g = 0; g < ng; ++g) {
        const int64_t w0 = perm_group_start(g, ng, W), nw = perm_group_start(g + 1, ng, W) - w0;
        int64_t slots = 0;
        for (const Launch& l : launches(tiles, tiles_per_launch_for(depth, f32, perm_epilogue(nw)), cap)) {
            out.push_back(PermLaunch{g, w0, nw, l.u0, l.cnt, l.grid});
            slots = l.grid > slots ? l.grid : slots;
        }
        if (group_slots) (*group_slots)[(size_t)g] = slots;
    }
    return out;
}

}  // namespace kad
}  // namespace fad
