// CPU check of fadtk_amd/csrc/kad_perm_tiles.h, the launches of the KAD permutation pass (fad_kad_permutation_test, kad.hip): over the
// launches the host cuts the pass into and the persistent walk of each launch's workgroups, every tile of Z's upper triangle is taken
// exactly once per permutation group; the groups cover every word of labellings once, each of at most kPermWords words and as few as
// there must be; every launch stays inside one group and under kad::tiles_per_launch_for(.., perm_epilogue(words)); a group's slots are
// as many as its widest launch's workgroups.  Sizes up to N = 2 * 10^6 rows and 65 537 labellings.
#include "../../fadtk_amd/csrc/kad_perm_tiles.h"

#include <cstdio>
#include <vector>

using namespace fad::kad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check(int64_t N, int64_t labellings, int64_t depth, bool f32, int64_t cap, const char* label) {
    const int64_t TZ = blocks(N), tiles = tri_tiles(TZ), W = perm_words(labellings), ng = perm_groups(W);
    std::vector<int64_t> gslots;
    const std::vector<PermLaunch> ls = perm_launches(TZ, labellings, depth, f32, cap, &gslots);
    CHECK(ng >= 1 && (ng - 1) * kPermWords < W && ng * kPermWords >= W, "%s: %lld groups for %lld words", label, (long long)ng, (long long)W);
    CHECK((int64_t)gslots.size() == ng, "%s: %zu group slot counts", label, gslots.size());
    std::vector<unsigned char> seen((size_t)tiles);
    int64_t words_seen = 0;
    size_t at = 0;
    for (int64_t g = 0; g < ng; ++g) {
        const int64_t w0 = perm_group_start(g, ng, W), nw = perm_group_start(g + 1, ng, W) - w0;
        CHECK(w0 == words_seen && nw >= 1 && nw <= kPermWords, "%s: group %lld words [%lld, +%lld)", label, (long long)g, (long long)w0,
              (long long)nw);
        words_seen += nw;
        std::fill(seen.begin(), seen.end(), 0);
        const int64_t per = tiles_per_launch_for(depth, f32, perm_epilogue(nw));
        int64_t slot = 0, next_u = 0;      // slot: the widest grid so far
        for (; at < ls.size() && ls[at].group == g; ++at) {
            const PermLaunch& l = ls[at];
            CHECK(l.w0 == w0 && l.nw == nw, "%s: launch of group %lld has words [%lld, +%lld)", label, (long long)g, (long long)l.w0,
                  (long long)l.nw);
            CHECK(l.cnt >= 1 && l.cnt <= per, "%s: a launch of %lld tiles, cap %lld", label, (long long)l.cnt, (long long)per);
            CHECK(l.u0 == next_u, "%s: launch starts at tile %lld, not %lld", label, (long long)l.u0, (long long)next_u);
            CHECK(l.grid % kXcds == 0 && l.grid >= kXcds && l.grid <= launch_slots(l.cnt) && l.grid <= cap, "%s: grid %lld", label,
                  (long long)l.grid);
            next_u += l.cnt;
            slot = l.grid > slot ? l.grid : slot;
            for (int64_t w = 0; w < l.grid; ++w)
                for (int64_t L = w; L < launch_slots(l.cnt); L += l.grid) {
                    bool live;
                    const int64_t v = slot_tile(L, l.cnt, &live);
                    if (!live) continue;
                    const int64_t u = l.u0 + v;
                    CHECK(v >= 0 && v < l.cnt && u < tiles, "%s: slot %lld -> tile %lld", label, (long long)L, (long long)u);
                    if (u >= 0 && u < tiles) seen[(size_t)u]++;
                    const Tile t = tri_tile(u, TZ);
                    CHECK(t.I >= 0 && t.I <= t.J && t.J < TZ, "%s: tile %lld -> (%lld, %lld)", label, (long long)u, (long long)t.I,
                          (long long)t.J);
                }
        }
        CHECK(next_u == tiles, "%s: group %lld walks %lld of %lld tiles", label, (long long)g, (long long)next_u, (long long)tiles);
        CHECK(gslots[(size_t)g] == slot, "%s: group %lld has %lld slots, its widest launch %lld", label, (long long)g, (long long)gslots[(size_t)g],
              (long long)slot);
        int64_t bad = 0;
        for (int64_t u = 0; u < tiles; ++u) bad += seen[(size_t)u] != 1;
        CHECK(bad == 0, "%s: group %lld: %lld tiles not taken exactly once", label, (long long)g, (long long)bad);
    }
    CHECK(at == ls.size(), "%s: %zu launches outside any group", label, ls.size() - at);
    CHECK(words_seen == W, "%s: groups cover %lld of %lld words", label, (long long)words_seen, (long long)W);
    // the triangle numbering itself: (I, J) row-major, each pair of row blocks I <= J once
    if (TZ <= 2048) {
        int64_t u = 0;
        for (int64_t I = 0; I < TZ; ++I)
            for (int64_t J = I; J < TZ; ++J, ++u) {
                const Tile t = tri_tile(u, TZ);
                CHECK(t.I == I && t.J == J, "%s: tile %lld is (%lld, %lld), not (%lld, %lld)", label, (long long)u, (long long)t.I,
                      (long long)t.J, (long long)I, (long long)J);
            }
    }
    printf("%s: N %lld TZ %lld labellings %lld groups %lld launches %zu\n", label, (long long)N, (long long)TZ, (long long)labellings,
           (long long)ng, ls.size());
}

int main() {
    check(4, 2, 128, false, 512, "n = m = 2, P = 1");
    check(702, 33, 1024, false, 512, "(2, 700), P = 32");
    check(256, 1001, 64, true, 64, "(127, 129) f32, P = 1000");
    check(1000, 1025, 128, false, 512, "P = 1024: two groups");
    check(5000, 65537, 2048, false, 512, "P = 65536");
    check(200000, 1001, 512, false, 512, "config-3, P = 1000");
    check(200000, 201, 128, false, 512, "config-3, P = 200");
    check(2000000, 1001, 128, false, 512, "N = 2e6, P = 1000");
    check(2000000, 2049, 2048, true, 64, "N = 2e6 f32, P = 2048");
    // under a small launch budget (kad::set_launch_budget, what FAD_KAD_LAUNCH_BUDGET sets in kad.hip): the shapes of the GPU test of the cut
    for (int64_t budget : {(int64_t)1, (int64_t)1 << 18}) {
        fad::kad::set_launch_budget(budget);
        check(2700, 34, 128, false, 512, "cut test, P = 33");
        check(2700, 34, 24, true, 512, "cut test f32, P = 33");
        check(2700, 1100, 80, false, 512, "cut test, two groups");
    }
    fad::kad::set_launch_budget(0);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK\n");
    return 0;
}
