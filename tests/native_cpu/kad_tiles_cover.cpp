// CPU check of fadtk_amd/csrc/kad_tiles.h, the tile map of the KAD kernels (kad.hip): over the launches a pass is cut into and the
// persistent walk of each launch's workgroups, every tile of the triangle / rectangle is taken exactly once, an XCD takes one
// contiguous stretch of a launch's tiles, and the in-tile masks count every unordered pair i < j of a set once (no i == j) and
// every (i, j) of a rectangle once.
#include "../../fadtk_amd/csrc/kad_tiles.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fad::kad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// every (I, J) a pass's launches (the host's launch cut) hand out, in the order the workgroups of each launch would meet them
template <typename F>
static void walk(int64_t total, int64_t per_launch, int64_t cap, F&& take) {
    for (const Launch& l : launches(total, per_launch, cap)) {
        const int64_t u0 = l.u0, cnt = l.cnt, G = l.grid;
        CHECK(G % kXcds == 0 && G >= kXcds && G <= launch_slots(cnt), "grid %lld for %lld tiles", (long long)G, (long long)cnt);
        std::vector<int64_t> lo(kXcds, -1), hi(kXcds, -1);
        for (int64_t w = 0; w < G; ++w)
            for (int64_t L = w; L < launch_slots(cnt); L += G) {
                bool live;
                const int64_t v = slot_tile(L, cnt, &live);
                if (!live) continue;
                CHECK(v >= 0 && v < cnt, "slot %lld -> %lld of %lld", (long long)L, (long long)v, (long long)cnt);
                const int x = (int)(w % kXcds);
                CHECK(L % kXcds == x, "slot %lld of workgroup %lld left its XCD", (long long)L, (long long)w);
                lo[x] = lo[x] < 0 || v < lo[x] ? v : lo[x];
                hi[x] = v > hi[x] ? v : hi[x];
                take(u0 + v);
            }
        for (int x = 0; x + 1 < kXcds; ++x)
            if (lo[x + 1] >= 0) CHECK(hi[x] + 1 == lo[x + 1], "XCD %d ends at %lld, XCD %d starts at %lld", x, (long long)hi[x], x + 1, (long long)lo[x + 1]);
    }
}

static void check_tri_pairs(int64_t n, int64_t per_launch, int64_t cap) {
    const int64_t T = blocks(n);
    std::vector<unsigned char> seen((size_t)(n * n), 0);
    walk(tri_tiles(T), per_launch, cap, [&](int64_t u) {
        const Tile t = tri_tile(u, T);
        CHECK(t.I >= 0 && t.I < T && t.J >= t.I && t.J < T, "tile %lld -> (%lld, %lld) of %lld", (long long)u, (long long)t.I, (long long)t.J, (long long)T);
        for (int r = 0; r < kTile; ++r)
            for (int c = 0; c < kTile; ++c)
                if (pair_counted(true, t.I, t.J, r, c, n, n)) {
                    const int64_t i = t.I * kTile + r, j = t.J * kTile + c;
                    CHECK(i < j, "pair (%lld, %lld) counted in a triangle", (long long)i, (long long)j);
                    if (i < j) seen[(size_t)(i * n + j)]++;
                }
    });
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = i + 1; j < n; ++j) CHECK(seen[(size_t)(i * n + j)] == 1, "n %lld: pair (%lld, %lld) counted %d times", (long long)n, (long long)i, (long long)j, seen[(size_t)(i * n + j)]);
}

static void check_rect_pairs(int64_t n, int64_t m, int64_t per_launch, int64_t cap) {
    const int64_t TI = blocks(n), TJ = blocks(m);
    std::vector<unsigned char> seen((size_t)(n * m), 0);
    walk(TI * TJ, per_launch, cap, [&](int64_t u) {
        const Tile t = rect_tile(u, TJ);
        CHECK(t.I < TI && t.J < TJ, "rect tile %lld", (long long)u);
        for (int r = 0; r < kTile; ++r)
            for (int c = 0; c < kTile; ++c)
                if (pair_counted(false, t.I, t.J, r, c, n, m)) seen[(size_t)((t.I * kTile + r) * m + t.J * kTile + c)]++;
    });
    for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1, "n %lld m %lld: (%zu) counted %d times", (long long)n, (long long)m, k, seen[k]);
}

int main() {
    // tile level: every triangle / rectangle tile once, for every block count of n = 1 .. 3000 and several launch cuts
    const int64_t cuts[] = {1, 3, 7, 8, 13, 64, 1 << 20}, caps[] = {8, 16, 1024};
    for (int64_t T = 1; T <= blocks(3000); ++T)
        for (int64_t per : cuts)
            for (int64_t cap : caps) {
                std::vector<int> tri((size_t)(T * T), 0), rect((size_t)(T * (T + 3)), 0);
                walk(tri_tiles(T), per, cap, [&](int64_t u) { const Tile t = tri_tile(u, T); tri[(size_t)(t.I * T + t.J)]++; });
                for (int64_t I = 0; I < T; ++I)
                    for (int64_t J = 0; J < T; ++J) CHECK(tri[(size_t)(I * T + J)] == (J >= I ? 1 : 0), "T %lld tile (%lld, %lld)", (long long)T, (long long)I, (long long)J);
                walk(T * (T + 3), per, cap, [&](int64_t u) { const Tile t = rect_tile(u, T + 3); rect[(size_t)(t.I * (T + 3) + t.J)]++; });
                for (int v : rect) CHECK(v == 1, "T %lld rectangle", (long long)T);
            }
    // large grids: the double root of tri_tile stays exact
    for (int64_t T : {1000, 7813, 78125}) {
        const int64_t tot = tri_tiles(T);
        for (int64_t u : {(int64_t)0, tot / 3, tot / 2, tot - T - 1, tot - 2, tot - 1}) {
            const Tile t = tri_tile(u, T);
            CHECK(t.J >= t.I && t.J < T && tri_row_start(t.I, T) + (t.J - t.I) == u, "T %lld u %lld", (long long)T, (long long)u);
        }
    }
    // pair level: n = 1 .. 3000 (all up to 300, then the tile edges and a stride), every launch cut
    std::vector<int64_t> ns;
    for (int64_t n = 1; n <= 300; ++n) ns.push_back(n);
    for (int64_t n = 301; n <= 3000; n += 97) ns.push_back(n);
    for (int64_t n : {383, 384, 385, 1023, 1024, 1025, 2999, 3000}) ns.push_back(n);
    int64_t cases = 0;
    for (int64_t n : ns) {
        const int64_t per = n <= 300 ? cuts[n % 7] : (n % 2 ? 5 : 1 << 20);
        check_tri_pairs(n, per, caps[n % 3]);
        check_rect_pairs(n, 1 + (n * 7) % 301, per, caps[(n + 1) % 3]);
        ++cases;
    }
    // launch sizes: at least 64 tiles, fewer for deeper tiles and for the float32 MFMA
    CHECK(tiles_per_launch(64, false) > tiles_per_launch(512, false) && tiles_per_launch(512, false) > tiles_per_launch(512, true), "launch sizes");
    CHECK(tiles_per_launch(2048, true) >= 64, "launch floor");
    for (int64_t depth : {64, 128, 512, 2048}) {   // a histogram tile costs more than a sum tile, several times more while its epilogue dominates
        CHECK(tiles_per_launch(depth, false, true) < tiles_per_launch(depth, false), "histogram launches at depth %lld", (long long)depth);
        if (depth <= 128) CHECK(tiles_per_launch(depth, false, true) * 4 <= tiles_per_launch(depth, false), "histogram launches at depth %lld", (long long)depth);
    }
    // the launch budget (the seam FAD_KAD_LAUNCH_BUDGET sets in kad.hip) and the tally of what launches() planned
    CHECK(launch_budget() == ((int64_t)1 << 30), "default budget %lld", (long long)launch_budget());
    CHECK(tiles_per_launch_for(2048, true, kSumEpilogue) == 32640, "D = 2048 f32 sums: %lld tiles per launch", (long long)tiles_per_launch_for(2048, true, kSumEpilogue));
    CHECK(tiles_per_launch(128, false) == ((int64_t)1 << 30) / 256, "D = 128 16-bit sums: %lld", (long long)tiles_per_launch(128, false));
    {
        reset_plan_tally();
        const std::vector<Launch> l = launches(tri_tiles(257), tiles_per_launch(2048, true), 512);   // 33 153 tiles over 32 640
        CHECK(l.size() == 2 && l[0].u0 == 0 && l[0].cnt == 32640 && l[1].u0 == 32640 && l[1].cnt == 513, "T = 257 plans %zu launches", l.size());
        CHECK(l[0].grid == 512 && l[1].grid == 512, "grids %lld and %lld", (long long)l[0].grid, (long long)l[1].grid);
        const PlanTally t = plan_tally();
        CHECK(t.passes == 1 && t.launches == 2 && t.min_launches == 2 && t.max_launches == 2, "tally %lld %lld %lld %lld", (long long)t.passes,
              (long long)t.launches, (long long)t.min_launches, (long long)t.max_launches);
        CHECK(t.max_walk == (32640 + 511) / 512, "walk %lld", (long long)t.max_walk);
        launches(tri_tiles(256), tiles_per_launch(2048, true), 512);                                 // 32 896 tiles: still two
        launches(100, tiles_per_launch(2048, true), 512);                                            // one launch of 104 slots on 104 workgroups
        launches(0, 64, 512);                                                                        // nothing to plan: not a pass
        const PlanTally u = plan_tally();
        CHECK(u.passes == 3 && u.launches == 5 && u.min_launches == 1 && u.max_launches == 2 && u.max_walk == t.max_walk, "tally %lld %lld %lld %lld %lld",
              (long long)u.passes, (long long)u.launches, (long long)u.min_launches, (long long)u.max_launches, (long long)u.max_walk);
        reset_plan_tally();
        CHECK(plan_tally().passes == 0 && plan_tally().launches == 0 && plan_tally().min_launches == 0 && plan_tally().max_walk == 0, "reset");
    }
    for (int64_t budget : {(int64_t)1, (int64_t)1000, (int64_t)1 << 18, (int64_t)1 << 24}) {
        set_launch_budget(budget);
        CHECK(launch_budget() == budget, "budget %lld", (long long)budget);
        for (int64_t depth : {8, 24, 128, 512, 2048})
            for (int f32 = 0; f32 < 2; ++f32)
                for (int64_t ep : {kSumEpilogue, kHistEpilogue, kTopkEpilogue, kFlagEpilogue, kNearestEpilogue, 8 * kSumEpilogue}) {
                    const int64_t want = budget / ((f32 ? 16 * depth : depth) + ep), got = tiles_per_launch_for(depth, f32 != 0, ep);
                    CHECK(got == (want < 64 ? 64 : want), "budget %lld depth %lld f32 %d epilogue %lld: %lld", (long long)budget, (long long)depth, f32,
                          (long long)ep, (long long)got);
                    if (budget == 1) CHECK(got == 64, "the floor at budget 1: %lld", (long long)got);
                }
        CHECK(tiles_per_launch(128, false) == tiles_per_launch_for(128, false, kSumEpilogue) && tiles_per_launch(128, false, true) == tiles_per_launch_for(128, false, kHistEpilogue),
              "tiles_per_launch reads the budget");
    }
    set_launch_budget((int64_t)1 << 18);                      // 1024 tiles per launch at D = 128 in 16 bit: 46 blocks' triangle is 1024 + 57
    {
        reset_plan_tally();
        const std::vector<Launch> l = launches(tri_tiles(46), tiles_per_launch(128, false), 512);
        CHECK(l.size() == 2 && l[0].cnt == 1024 && l[1].cnt == 57 && l[1].grid == 64, "46 blocks at 2^18");
        CHECK(plan_tally().max_walk == 2, "walk %lld", (long long)plan_tally().max_walk);
    }
    set_launch_budget(1);                                     // the floor: every pair once when every launch holds 64 tiles
    check_tri_pairs(1290, tiles_per_launch(128, false), 512);
    check_rect_pairs(1290, 1410, tiles_per_launch(24, true), 512);
    for (int64_t bad : {(int64_t)0, (int64_t)-5}) {           // <= 0: the default
        set_launch_budget(bad);
        CHECK(launch_budget() == ((int64_t)1 << 30) && tiles_per_launch(2048, true) == 32640, "budget %lld falls back", (long long)bad);
    }
    printf("kad tiles: %lld pair cases, tiles per launch D=128 f16 %lld (histogram %lld), D=512 f16 %lld (histogram %lld), D=2048 f32 %lld\n",
           (long long)cases, (long long)tiles_per_launch(128, false), (long long)tiles_per_launch(128, false, true),
           (long long)tiles_per_launch(512, false), (long long)tiles_per_launch(512, false, true), (long long)tiles_per_launch(2048, true));
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK\n");
    return 0;
}
