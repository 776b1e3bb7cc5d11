// CPU check of fadtk_amd/csrc/kid_tiles.h, the work units of fad_kid_subsets (kad.hip): over the launches the host cuts a group's pass
// into and the persistent walk of each launch's workgroups, every (subset, block, tile) unit is taken exactly once; unit_of and
// unit_index are inverse; pair_counted counts every pair i != j of a subset's XX / YY block once as (i < j) and every pair of XY once,
// and no pair that touches a padding row; no launch takes more units than kad::tiles_per_launch allows; and kid::plan's groups cover
// the subsets exactly once, in order, under the budget (one subset per group where one alone is over it).
#include "../../fadtk_amd/csrc/kid_tiles.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_units(int64_t s, int64_t n_subsets, int64_t depth, bool f32, int64_t cap) {
    const int64_t T = kad::blocks(s), U = kid::units_per_subset(T), total = n_subsets * U, per = kad::tiles_per_launch(depth, f32);
    CHECK(U == 2 * kad::tri_tiles(T) + T * T, "s %lld: %lld units", (long long)s, (long long)U);
    std::vector<unsigned char> seen((size_t)total, 0);
    for (const kad::Launch& l : kad::launches(total, per, cap)) {
        CHECK(l.cnt <= per, "a launch of %lld units, cap %lld", (long long)l.cnt, (long long)per);
        CHECK(l.grid % kad::kXcds == 0 && l.grid >= kad::kXcds && l.grid <= kad::launch_slots(l.cnt), "grid %lld for %lld units",
              (long long)l.grid, (long long)l.cnt);
        for (int64_t w = 0; w < l.grid; ++w)
            for (int64_t L = w; L < kad::launch_slots(l.cnt); L += l.grid) {
                bool live;
                const int64_t v = kad::slot_tile(L, l.cnt, &live);
                if (!live) continue;
                CHECK(v >= 0 && v < l.cnt, "slot %lld -> %lld of %lld", (long long)L, (long long)v, (long long)l.cnt);
                const int64_t u = l.u0 + v;
                const kid::Unit t = kid::unit_of(u, T);
                CHECK(t.q >= 0 && t.q < n_subsets && t.block >= kid::XX && t.block <= kid::XY && t.I >= 0 && t.I < T && t.J >= 0 && t.J < T &&
                      (t.block == kid::XY || t.I <= t.J), "unit %lld -> q %lld block %d tile (%lld, %lld)", (long long)u, (long long)t.q, t.block,
                      (long long)t.I, (long long)t.J);
                CHECK(kid::unit_index(t.q, t.block, t.I, t.J, T) == u, "unit %lld does not map back", (long long)u);
                seen[(size_t)u]++;
            }
    }
    for (int64_t u = 0; u < total; ++u) CHECK(seen[(size_t)u] == 1, "s %lld, %lld subsets: unit %lld taken %d times", (long long)s, (long long)n_subsets, (long long)u, seen[(size_t)u]);

    // every (block, tile) of one subset exactly once among its U units, and the pairs they count
    std::vector<unsigned char> tile_seen((size_t)(3 * T * T), 0);
    int64_t counted[3] = {0, 0, 0};
    for (int64_t w = 0; w < U; ++w) {
        const kid::Unit t = kid::unit_of((n_subsets - 1) * U + w, T);
        CHECK(t.q == n_subsets - 1, "unit %lld of the last subset -> q %lld", (long long)w, (long long)t.q);
        tile_seen[(size_t)((t.block * T + t.I) * T + t.J)]++;
        for (int r = 0; r < kad::kTile; ++r)
            for (int c = 0; c < kad::kTile; ++c) {
                if (!kid::pair_counted(t.block, t.I, t.J, r, c, s)) continue;
                const int64_t i = t.I * kad::kTile + r, j = t.J * kad::kTile + c;
                CHECK(i < s && j < s && (t.block == kid::XY || i < j), "block %d: pair (%lld, %lld) counted, s %lld", t.block, (long long)i, (long long)j, (long long)s);
                counted[t.block]++;
            }
    }
    for (int b = 0; b < 3; ++b)
        for (int64_t I = 0; I < T; ++I)
            for (int64_t J = 0; J < T; ++J)
                CHECK(tile_seen[(size_t)((b * T + I) * T + J)] == ((b == kid::XY || I <= J) ? 1 : 0), "block %d tile (%lld, %lld) taken %d times", b,
                      (long long)I, (long long)J, tile_seen[(size_t)((b * T + I) * T + J)]);
    CHECK(counted[kid::XX] == s * (s - 1) / 2 && counted[kid::YY] == s * (s - 1) / 2 && counted[kid::XY] == s * s,
          "s %lld: %lld / %lld / %lld pairs counted", (long long)s, (long long)counted[0], (long long)counted[1], (long long)counted[2]);
}

static void check_plan(int64_t n_subsets, int64_t s, int64_t row_bytes, int64_t budget) {
    const std::vector<kid::Group> groups = kid::plan(n_subsets, s, row_bytes, budget);
    const int64_t one = kid::subset_bytes(s, row_bytes);
    CHECK(one >= 2 * s * row_bytes, "subset_bytes(%lld, %lld) = %lld", (long long)s, (long long)row_bytes, (long long)one);
    int64_t next = 0;
    for (const kid::Group& g : groups) {
        CHECK(g.q0 == next && g.count >= 1, "group at %lld of %lld, expected %lld", (long long)g.q0, (long long)g.count, (long long)next);
        CHECK(g.count == 1 || g.count * one <= budget, "a group of %lld subsets takes %lld bytes, budget %lld", (long long)g.count,
              (long long)(g.count * one), (long long)budget);
        next += g.count;
    }
    CHECK(next == n_subsets, "the groups cover %lld of %lld subsets", (long long)next, (long long)n_subsets);
    if (budget < 2 * one) CHECK((int64_t)groups.size() == n_subsets, "budget %lld under two subsets: %zu groups for %lld subsets", (long long)budget, groups.size(), (long long)n_subsets);
    if (budget >= n_subsets * one) CHECK(groups.size() == 1, "everything fits: %zu groups", groups.size());
}

int main() {
    const int64_t sizes[] = {2, 128, 129, 300, 1000}, counts[] = {1, 3, 17, 100};
    for (int64_t s : sizes)
        for (int64_t q : counts) {
            check_units(s, q, 512, false, 512);
            check_units(s, q, 2048, true, 8);          // float32 at the deepest rows: the shortest launches, the smallest grid
        }
    check_units(1000, 1000, 2048, true, 512);          // 1000 x 1000: many launches
    check_units(3000, 2, 128, false, 512);

    for (int64_t s : sizes)
        for (int64_t q : counts)
            for (int64_t budget : {(int64_t)1, (int64_t)1 << 20, (int64_t)5 << 20, (int64_t)64 << 20, kid::kImageBudget, (int64_t)1 << 40}) {
                check_plan(q, s, 256, budget);
                check_plan(q, s, 5120, budget);
            }
    // the shape of the GPU test of the groups: float32, D = 1280, s = 129 crosses the entry point's budget with a few dozen subsets
    CHECK(kid::plan(60, 129, 5120, kid::kImageBudget).size() == 2, "60 subsets of 129 float32 rows at D = 1280: %zu groups",
          kid::plan(60, 129, 5120, kid::kImageBudget).size());

    // under a small launch budget (kad::set_launch_budget, what FAD_KAD_LAUNCH_BUDGET sets in kad.hip): the shapes of the GPU test of the cut
    for (int64_t budget : {(int64_t)1, (int64_t)1 << 18}) {
        kad::set_launch_budget(budget);
        check_units(129, 17, 128, false, 512);
        check_units(129, 17, 24, true, 512);
        check_units(300, 100, 16, false, 512);
    }
    kad::set_launch_budget(0);
    printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
