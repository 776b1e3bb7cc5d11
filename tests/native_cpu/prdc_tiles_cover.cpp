// CPU check of the unit map of fad_prdc's passes (kad.hip): kad_song_tiles.h's cross map with rows per unit from
// kad::prdc_rows_per_unit.  Over the launches a pass is cut into (kad::launches with kad::prdc_units_per_launch) and the persistent
// walk of each launch's workgroups, every tile of the rows x columns rectangle is taken exactly once, every unit's slot row R lies
// below NR, no launch takes more tiles than kad::tiles_per_launch_for allows with the pass's epilogue weight, and a launch holds at
// least kPrdcLaunchUnits units unless it is the whole pass.  Radius passes (n x n, top-k weight) and cross passes (n x m, flag weight)
// at sizes up to 10^6 rows.
#include "../../fadtk_amd/csrc/kad_song_tiles.h"

#include <cstdio>
#include <vector>

using namespace fad::kad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_pass(int64_t n, int64_t m, int64_t depth, bool f32, int64_t epilogue, int64_t cap) {
    const int64_t TI = blocks(n), TJ = blocks(m), per = tiles_per_launch_for(depth, f32, epilogue);
    const int64_t rr = prdc_rows_per_unit(TI, TJ, per), NR = cross_ranges(TI, rr), upl = prdc_units_per_launch(rr, per);
    CHECK(rr >= 1 && NR * rr >= TI && (NR - 1) * rr < TI && upl * rr <= per, "n %lld m %lld: rr %lld NR %lld per %lld", (long long)n,
          (long long)m, (long long)rr, (long long)NR, (long long)per);
    std::vector<unsigned char> seen((size_t)(TI * TJ), 0);
    const std::vector<Launch> ls = launches(NR * TJ, upl, cap);
    for (const Launch& l : ls) {
        const int64_t G = l.grid;
        CHECK(G % kXcds == 0 && G >= kXcds && G <= launch_slots(l.cnt) && G <= cap, "grid %lld for %lld units", (long long)G, (long long)l.cnt);
        // (a launch budget under kPrdcLaunchUnits tiles -- only a test's FAD_KAD_LAUNCH_BUDGET gives one -- cannot hold that many units)
        CHECK(ls.size() == 1 || l.cnt >= kPrdcLaunchUnits || &l == &ls.back() || per < kPrdcLaunchUnits, "n %lld m %lld: a launch of %lld units", (long long)n,
              (long long)m, (long long)l.cnt);
        int64_t tiles = 0;
        for (int64_t w = 0; w < G; ++w)
            for (int64_t L = w; L < launch_slots(l.cnt); L += G) {
                bool live;
                const int64_t v = slot_tile(L, l.cnt, &live);
                if (!live) continue;
                const int64_t u = l.u0 + v;
                const Unit t = cross_unit(u, TI, TJ, rr);
                CHECK(u / TJ < NR && t.J >= 0 && t.J < TJ && t.I0 >= 0 && t.I0 < t.I1 && t.I1 <= TI, "unit %lld -> J %lld rows [%lld, %lld)",
                      (long long)u, (long long)t.J, (long long)t.I0, (long long)t.I1);
                for (int64_t I = t.I0; I < t.I1; ++I) seen[(size_t)(I * TJ + t.J)]++;
                tiles += t.I1 - t.I0;
            }
        CHECK(tiles <= per, "n %lld m %lld: a launch of %lld tiles, cap %lld", (long long)n, (long long)m, (long long)tiles, (long long)per);
    }
    for (size_t q = 0; q < seen.size(); ++q)
        CHECK(seen[q] == 1, "n %lld m %lld: tile (%lld, %lld) taken %d times", (long long)n, (long long)m, (long long)(q / TJ),
              (long long)(q % TJ), seen[q]);
}

int main() {
    const int64_t sizes[][2] = {{2, 2}, {6, 17}, {129, 300}, {1000, 1000}, {3000, 5000}, {100000, 100000}, {100000, 20000},
                                {1000000, 129}, {129, 1000000}};
    for (auto& s : sizes) {
        check_pass(s[0], s[0], 128, false, kTopkEpilogue, 512);
        check_pass(s[1], s[1], 2048, true, kTopkEpilogue, 512);
        check_pass(s[0], s[1], 512, false, kFlagEpilogue, 512);
        check_pass(s[0], s[1], 2048, true, kFlagEpilogue, 8);
    }
    check_pass(1000000, 1000000, 128, false, kTopkEpilogue, 512);         // n = m = 10^6 at D = 128, float16
    check_pass(1000000, 1000000, 128, false, kFlagEpilogue, 512);
    // under a small launch budget (kad::set_launch_budget, what FAD_KAD_LAUNCH_BUDGET sets in kad.hip): the shapes of the GPU test of the cut
    for (int64_t budget : {(int64_t)1, (int64_t)1 << 18, (int64_t)1 << 21}) {
        set_launch_budget(budget);
        for (int64_t ep : {kTopkEpilogue, kFlagEpilogue, kNearestEpilogue}) {
            check_pass(1290, 1410, 128, false, ep, 512);
            check_pass(2700, 2700, 24, true, ep, 512);
            check_pass(5800, 1300, 128, false, ep, 512);
            check_pass(7100, 7100, 24, true, ep, 512);
        }
    }
    set_launch_budget(0);
    printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
