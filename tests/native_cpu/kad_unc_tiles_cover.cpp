// CPU check of fadtk_amd/csrc/kad_unc_tiles.h, the work units of the KAD uncertainty pass (fad_kad_uncertainty, kad.hip): over the
// launches the host cuts the pass into and the persistent walk of each launch's workgroups, every tile the estimate needs -- K_XX, both
// orientations of every X x Y_s product, every K_YsYs -- is taken exactly once and no other tile is; every unit lies inside its
// segment (so no unit's row run crosses a set) and its segment is the one unc_segment names for it; and no launch takes more tiles than
// kad::tiles_per_launch_for(.., kUncEpilogue) allows.  Sizes up to n = 10^6 and S = 64, ragged sets of 2 .. 300 rows.
#include "../../fadtk_amd/csrc/kad_unc_tiles.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace fad::kad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the row group of row block I: 0 for X, s + 1 for set s
static int group_of(const std::vector<int64_t>& blk, int64_t I) {
    if (I < blk[0]) return 0;
    int s = 0;
    while (I >= blk[(size_t)s + 1]) ++s;
    return s + 1;
}

static void check(int64_t n, const std::vector<int64_t>& ms, int64_t depth, bool f32, int64_t cap, const char* label) {
    const int S = (int)ms.size();
    const std::vector<int64_t> blk = unc_blocks(n, ms.data(), S);
    const int64_t TX = blk[0], TZ = blk[(size_t)S], per = tiles_per_launch_for(depth, f32, kUncEpilogue);
    const int64_t rr = unc_rows_per_unit(unc_tiles(blk), per);
    CHECK(rr >= 1 && rr <= per, "%s: rr %lld", label, (long long)rr);
    std::vector<Unit> units;
    std::vector<int64_t> seg;
    unc_units(blk, rr, &units, &seg);
    const int64_t U = (int64_t)units.size();
    CHECK((int64_t)seg.size() == unc_segments(TX, TZ, S) + 1 && seg[0] == 0 && seg.back() == U, "%s: %zu segment starts", label, seg.size());

    // every unit: inside one row group, in the segment unc_segment gives its (J, group), at most rr blocks
    std::vector<int64_t> seg_of((size_t)U, -1);
    for (size_t k = 0; k + 1 < seg.size(); ++k) {
        CHECK(seg[k] < seg[k + 1], "%s: empty segment %zu", label, k);
        for (int64_t u = seg[k]; u < seg[k + 1]; ++u) seg_of[(size_t)u] = (int64_t)k;
    }
    int64_t tiles = 0;
    for (int64_t u = 0; u < U; ++u) {
        const Unit& t = units[(size_t)u];
        const int g = group_of(blk, t.I0);
        CHECK(t.I0 < t.I1 && t.I1 - t.I0 <= rr && t.J >= 0 && t.J < TZ, "%s: unit %lld", label, (long long)u);
        CHECK(group_of(blk, t.I1 - 1) == g, "%s: unit %lld rows [%lld, %lld) cross a set", label, (long long)u, (long long)t.I0, (long long)t.I1);
        const int own = group_of(blk, t.J);
        CHECK(own == 0 || g == 0 || g == own, "%s: unit %lld pairs set %d rows with set %d columns", label, (long long)u, g - 1, own - 1);
        CHECK(seg_of[(size_t)u] == unc_segment(t.J, g, TX, S), "%s: unit %lld in segment %lld, not %lld", label, (long long)u,
              (long long)seg_of[(size_t)u], (long long)unc_segment(t.J, g, TX, S));
        tiles += t.I1 - t.I0;
    }
    CHECK(tiles == unc_tiles(blk), "%s: %lld tiles in the units, %lld in the pass", label, (long long)tiles, (long long)unc_tiles(blk));

    // the launches: every unit once, under the tile cap; every needed tile once (a tile count per (I, J) where the grid is small,
    // a count per column block and row group where it is not)
    const bool full = TZ <= 4096;
    std::vector<unsigned char> seen(full ? (size_t)(TZ * TZ) : 0, 0);
    std::vector<int64_t> per_seg(seg.size() - 1, 0);
    std::vector<unsigned char> unit_seen((size_t)U, 0);
    for (const Launch& l : launches(U, unc_units_per_launch(rr, depth, f32), cap)) {
        const int64_t G = l.grid;
        CHECK(G % kXcds == 0 && G >= kXcds && G <= launch_slots(l.cnt), "%s: grid %lld for %lld units", label, (long long)G, (long long)l.cnt);
        int64_t launch_tiles = 0;
        for (int64_t w = 0; w < G; ++w)
            for (int64_t L = w; L < launch_slots(l.cnt); L += G) {
                bool live;
                const int64_t v = slot_tile(L, l.cnt, &live);
                if (!live) continue;
                const int64_t u = l.u0 + v;
                CHECK(v >= 0 && v < l.cnt && u < U, "%s: slot %lld -> %lld", label, (long long)L, (long long)v);
                unit_seen[(size_t)u]++;
                const Unit& t = units[(size_t)u];
                launch_tiles += t.I1 - t.I0;
                per_seg[(size_t)seg_of[(size_t)u]] += t.I1 - t.I0;
                if (full)
                    for (int64_t I = t.I0; I < t.I1; ++I) seen[(size_t)(I * TZ + t.J)]++;
            }
        CHECK(launch_tiles <= per, "%s: a launch of %lld tiles, cap %lld", label, (long long)launch_tiles, (long long)per);
    }
    for (int64_t u = 0; u < U; ++u) CHECK(unit_seen[(size_t)u] == 1, "%s: unit %lld taken %d times", label, (long long)u, unit_seen[(size_t)u]);
    for (int64_t J = 0; J < TZ; ++J) {
        const int own = group_of(blk, J);
        for (int g = 0; g <= S; ++g) {
            const bool needed = own == 0 || g == 0 || g == own;
            if (!needed) continue;
            const int64_t rows = g == 0 ? TX : blk[(size_t)g] - blk[(size_t)g - 1];
            CHECK(per_seg[(size_t)unc_segment(J, g, TX, S)] == rows, "%s: column block %lld, group %d: %lld of %lld tiles", label,
                  (long long)J, g, (long long)per_seg[(size_t)unc_segment(J, g, TX, S)], (long long)rows);
        }
    }
    if (full)
        for (int64_t I = 0; I < TZ; ++I)
            for (int64_t J = 0; J < TZ; ++J) {
                const int gi = group_of(blk, I), gj = group_of(blk, J);
                const int want = (gi == 0 || gj == 0 || gi == gj) ? 1 : 0;
                CHECK(seen[(size_t)(I * TZ + J)] == want, "%s: tile (%lld, %lld) taken %d times, want %d", label, (long long)I, (long long)J,
                      seen[(size_t)(I * TZ + J)], want);
            }
    printf("%s: n %lld S %d TZ %lld rr %lld units %lld\n", label, (long long)n, S, (long long)TZ, (long long)rr, (long long)U);
}

int main() {
    std::mt19937_64 rng(7);
    auto ragged = [&](int S, int lo, int hi) {
        std::vector<int64_t> ms((size_t)S);
        for (auto& m : ms) m = lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
        return ms;
    };
    const int64_t caps[2] = {512, 64};
    check(2, {2}, 128, false, caps[0], "tiny");
    check(255, {257}, 128, false, caps[0], "S=1 ragged");
    check(300, {2, 3, 129, 300}, 512, true, caps[1], "S=4 small f32");
    check(1000, ragged(3, 2, 300), 1024, false, caps[0], "S=3 ragged");
    check(5000, ragged(64, 2, 300), 128, false, caps[0], "S=64 ragged");
    check(100000, {100000}, 512, false, caps[0], "config-3 S=1");
    check(100000, {100000, 100000, 100000, 100000}, 128, false, caps[0], "config-3 S=4");
    check(1000000, {1000000}, 128, false, caps[0], "n=1e6 S=1");
    check(1000000, ragged(64, 2, 300), 128, false, caps[0], "n=1e6 S=64 ragged");
    check(1000000, ragged(64, 2, 300), 1024, true, caps[1], "n=1e6 S=64 ragged f32");
    // under a small launch budget (kad::set_launch_budget, what FAD_KAD_LAUNCH_BUDGET sets in kad.hip): the shapes of the GPU test of the cut
    for (int64_t budget : {(int64_t)1, (int64_t)1 << 18}) {
        fad::kad::set_launch_budget(budget);
        if (budget == 1) CHECK(fad::kad::unc_units_per_launch(1, 128, false) == 64 && fad::kad::unc_rows_per_unit(1000000, fad::kad::tiles_per_launch_for(128, false, fad::kad::kUncEpilogue)) == 1,
                               "the floor at budget 1");
        check(1290, {1410, 700}, 128, false, caps[0], "cut test, two sets");
        check(1290, {1410, 700}, 24, true, caps[0], "cut test, two sets f32");
        check(2700, {}, 128, false, caps[0], "cut test, pooled rows");
    }
    fad::kad::set_launch_budget(0);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK\n");
    return 0;
}
