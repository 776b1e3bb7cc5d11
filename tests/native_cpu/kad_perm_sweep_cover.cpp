// CPU check of fadtk_amd/csrc/kad_perm_sweep_tiles.h, the plan of the KAD permutation sweep (fad_kad_permutation_sweep, kad.hip): over
// the walks the host cuts a call into, the launches of each walk and the persistent walk of each launch's workgroups, every (bandwidth,
// labelling word, triangle tile) is taken exactly once; a walk holds kernel_nb * nw <= kPermWords partials per lane and nb <= kernel_nb
// bandwidths; every launch stays under tiles_per_launch_for(.., perm_epilogue(kernel_nb * nw)); a walk's slots are as many as its widest
// launch's workgroups; the walks are as few as any uniform cut into runs of 1, 2 or 4 bandwidths gives, the smaller run at a tie (one walk per bandwidth
// when the labellings fill kPermWords words); and a
// walk of one bandwidth is cut exactly as kad_perm_tiles.h cuts the single test (check_single: the same groups, slots and launches, which
// is what lets the single test run through the sweep's host driver).
#include "../../fadtk_amd/csrc/kad_perm_sweep_tiles.h"

#include <cstdio>
#include <vector>

using namespace fad::kad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check(int64_t N, int n_bw, int64_t labellings, int64_t depth, bool f32, int64_t cap, const char* label) {
    const int64_t TZ = blocks(N), tiles = tri_tiles(TZ), W = perm_words(labellings);
    const std::vector<PermSweepWalk> walks = perm_sweep_walks(n_bw, labellings);
    std::vector<int64_t> wslots;
    const std::vector<PermSweepLaunch> ls = perm_sweep_launches(TZ, walks, depth, f32, cap, &wslots);
    CHECK(wslots.size() == walks.size(), "%s: %zu slot counts for %zu walks", label, wslots.size(), walks.size());

    // as few walks as a uniform cut gives, ties to the smaller NB
    const int NB = perm_sweep_nb(n_bw, W);
    for (int other = 1; other <= kPermSweepNB; other *= 2) {
        const int64_t mine = perm_sweep_walk_count(n_bw, W, NB), theirs = perm_sweep_walk_count(n_bw, W, other);
        CHECK(mine < theirs || (mine == theirs && NB <= other), "%s: NB %d gives %lld walks, NB %d gives %lld", label, NB, (long long)mine, other,
              (long long)theirs);
    }
    CHECK((int64_t)walks.size() == perm_sweep_walk_count(n_bw, W, NB), "%s: %zu walks", label, walks.size());
    if (W == kPermWords)                                                                // a full group of words: the single test's kernel, once per bandwidth
        CHECK(NB == 1 && (int64_t)walks.size() == n_bw, "%s: %lld words do not run one walk per bandwidth", label, (long long)W);
    CHECK((int64_t)walks.size() * kPermWords >= (int64_t)n_bw * W, "%s: %zu walks cannot hold %d x %lld words", label, walks.size(), n_bw, (long long)W);

    std::vector<int> word_seen((size_t)(n_bw * W), 0);
    std::vector<unsigned char> seen((size_t)tiles);
    size_t at = 0;
    for (size_t i = 0; i < walks.size(); ++i) {
        const PermSweepWalk& w = walks[i];
        CHECK(w.nb >= 1 && w.nb <= w.kernel_nb && (w.kernel_nb == 1 || w.kernel_nb == 2 || w.kernel_nb == 4) && w.kernel_nb == perm_sweep_kernel_nb(w.nb),
              "%s: walk %zu runs %d bandwidths in the kernel of %d", label, i, w.nb, w.kernel_nb);
        CHECK(w.nw >= 1 && w.kernel_nb * w.nw <= kPermWords, "%s: walk %zu holds %d x %lld words", label, i, w.kernel_nb, (long long)w.nw);
        CHECK(w.b0 >= 0 && w.b0 + w.nb <= n_bw && w.w0 >= 0 && w.w0 + w.nw <= W && w.wg >= 0 && w.wg < w.wgs, "%s: walk %zu out of range", label, i);
        for (int b = w.b0; b < w.b0 + w.nb; ++b)
            for (int64_t x = w.w0; x < w.w0 + w.nw; ++x) word_seen[(size_t)(b * W + x)]++;
        std::fill(seen.begin(), seen.end(), 0);
        const int64_t per = tiles_per_launch_for(depth, f32, perm_epilogue(w.kernel_nb * w.nw));
        int64_t slot = 0, next_u = 0;
        for (; at < ls.size() && ls[at].walk == (int64_t)i; ++at) {
            const PermSweepLaunch& l = ls[at];
            CHECK(l.cnt >= 1 && l.cnt <= per, "%s: a launch of %lld tiles, cap %lld", label, (long long)l.cnt, (long long)per);
            CHECK(l.u0 == next_u, "%s: launch starts at tile %lld, not %lld", label, (long long)l.u0, (long long)next_u);
            CHECK(l.grid % kXcds == 0 && l.grid >= kXcds && l.grid <= launch_slots(l.cnt) && l.grid <= cap, "%s: grid %lld", label, (long long)l.grid);
            next_u += l.cnt;
            slot = l.grid > slot ? l.grid : slot;
            for (int64_t g = 0; g < l.grid; ++g)
                for (int64_t L = g; L < launch_slots(l.cnt); L += l.grid) {
                    bool live;
                    const int64_t v = slot_tile(L, l.cnt, &live);
                    if (!live) continue;
                    const int64_t u = l.u0 + v;
                    CHECK(v >= 0 && v < l.cnt && u < tiles, "%s: slot %lld -> tile %lld", label, (long long)L, (long long)u);
                    if (u >= 0 && u < tiles) seen[(size_t)u]++;
                }
        }
        CHECK(next_u == tiles, "%s: walk %zu covers %lld of %lld tiles", label, i, (long long)next_u, (long long)tiles);
        CHECK(wslots[i] == slot, "%s: walk %zu has %lld slots, its widest launch %lld", label, i, (long long)wslots[i], (long long)slot);
        int64_t bad = 0;
        for (int64_t u = 0; u < tiles; ++u) bad += seen[(size_t)u] != 1;
        CHECK(bad == 0, "%s: walk %zu: %lld tiles not taken exactly once", label, i, (long long)bad);
    }
    CHECK(at == ls.size(), "%s: %zu launches outside any walk", label, ls.size() - at);
    int64_t bad = 0;
    for (int v : word_seen) bad += v != 1;
    CHECK(bad == 0, "%s: %lld (bandwidth, word) pairs not covered exactly once", label, (long long)bad);

    // one bandwidth: the single test's own groups and launches
    if (n_bw == 1) {
        std::vector<int64_t> gslots;
        const std::vector<PermLaunch> single = perm_launches(TZ, labellings, depth, f32, cap, &gslots);
        CHECK(single.size() == ls.size() && gslots == wslots, "%s: one bandwidth is not cut as the single test", label);
        for (size_t i = 0; i < single.size() && i < ls.size(); ++i)
            CHECK(single[i].u0 == ls[i].u0 && single[i].cnt == ls[i].cnt && single[i].grid == ls[i].grid && single[i].w0 == walks[(size_t)ls[i].walk].w0 &&
                  single[i].nw == walks[(size_t)ls[i].walk].nw, "%s: launch %zu differs from the single test's", label, i);
    }
    printf("%s: N %lld B %d labellings %lld NB %d walks %zu launches %zu\n", label, (long long)N, n_bw, (long long)labellings, NB, walks.size(), ls.size());
}

// One bandwidth through the sweep's plan is the single test's plan, exactly: fad_kad_permutation_test_k runs the sweep's driver with one
// bandwidth (kad.hip perm_run), so perm_sweep_walks(1, NL) with perm_sweep_launches must give perm_launches' groups (their number, w0
// and nw), the slots of each group and the sequence of (group, u0, cnt, grid).
static void check_single(int64_t TZ, int64_t NL, int64_t depth, bool f32, int64_t cap) {
    char label[128];
    snprintf(label, sizeof(label), "single: TZ %lld NL %lld depth %lld f32 %d cap %lld budget %lld", (long long)TZ, (long long)NL, (long long)depth,
             (int)f32, (long long)cap, (long long)launch_budget());
    std::vector<int64_t> gslots, wslots;
    const std::vector<PermLaunch> single = perm_launches(TZ, NL, depth, f32, cap, &gslots);
    const std::vector<PermSweepWalk> walks = perm_sweep_walks(1, NL);
    const std::vector<PermSweepLaunch> ls = perm_sweep_launches(TZ, walks, depth, f32, cap, &wslots);
    const int64_t W = perm_words(NL), ng = perm_groups(W);
    CHECK((int64_t)walks.size() == ng && (int64_t)gslots.size() == ng, "%s: %zu walks, %zu groups, perm_groups %lld", label, walks.size(),
          gslots.size(), (long long)ng);
    for (size_t g = 0; g < walks.size() && g < gslots.size(); ++g) {
        const PermSweepWalk& w = walks[g];
        const int64_t w0 = perm_group_start((int64_t)g, ng, W), nw = perm_group_start((int64_t)g + 1, ng, W) - w0;
        CHECK(w.b0 == 0 && w.nb == 1 && w.kernel_nb == 1 && w.wg == (int64_t)g && w.wgs == ng, "%s: walk %zu is not word group %zu of one bandwidth",
              label, g, g);
        CHECK(w.w0 == w0 && w.nw == nw, "%s: walk %zu words [%lld, +%lld), group [%lld, +%lld)", label, g, (long long)w.w0, (long long)w.nw,
              (long long)w0, (long long)nw);
        CHECK(wslots[g] == gslots[g], "%s: walk %zu has %lld slots, the group %lld", label, g, (long long)wslots[g], (long long)gslots[g]);
    }
    CHECK(single.size() == ls.size(), "%s: %zu launches, the single test %zu", label, ls.size(), single.size());
    for (size_t i = 0; i < single.size() && i < ls.size(); ++i) {
        const PermLaunch& a = single[i];
        const PermSweepLaunch& b = ls[i];
        CHECK(a.group == b.walk && a.u0 == b.u0 && a.cnt == b.cnt && a.grid == b.grid, "%s: launch %zu is (%lld, %lld, %lld, %lld), the single test's "
              "(%lld, %lld, %lld, %lld)", label, i, (long long)b.walk, (long long)b.u0, (long long)b.cnt, (long long)b.grid, (long long)a.group,
              (long long)a.u0, (long long)a.cnt, (long long)a.grid);
        if (b.walk >= 0 && b.walk < (int64_t)walks.size())
            CHECK(a.w0 == walks[(size_t)b.walk].w0 && a.nw == walks[(size_t)b.walk].nw, "%s: launch %zu takes other words than the single test's", label, i);
    }
}

int main() {
    for (int B = 1; B <= kPermSweepMax; ++B)
        for (int64_t P : {1, 31, 32, 199, 255, 256, 300, 511, 512, 999, 1023, 1024, 2048})
            check(512, B, P + 1, 128, false, 512, "n + m = 512");
    check(4, 4, 2, 128, false, 512, "n = m = 2, P = 1, B = 4");
    check(512, 3, 301, 64, true, 64, "f32, B = 3, P = 300");
    check(5000, 16, 65537, 2048, false, 512, "P = 65536, B = 16");
    check(200000, 4, 200, 512, false, 512, "config-3, B = 4, P = 199");
    check(200000, 4, 1000, 128, false, 512, "config-3, B = 4, P = 999");
    check(200000, 5, 200, 512, false, 512, "config-3, B = 5, P = 199");
    check(2000000, 2, 400, 128, false, 512, "N = 2e6, B = 2, P = 399");
    check(2000000, 3, 2049, 2048, true, 64, "N = 2e6 f32, B = 3, P = 2048");
    // the plans the GPU tests rely on: 4 x 7 words share one walk; 10 words force several
    CHECK(perm_sweep_walks(4, 200).size() == 1 && perm_sweep_walks(4, 200)[0].kernel_nb == 4, "B = 4, P = 199 is not one walk of 4");
    CHECK(perm_sweep_walks(4, 301).size() == 2 && perm_sweep_walks(4, 301)[0].kernel_nb == 2, "B = 4, P = 300 is not two walks of 2");
    CHECK(perm_sweep_walks(3, 200).size() == 1 && perm_sweep_walks(3, 200)[0].nb == 3, "B = 3, P = 199 is not one walk of 3 in the kernel of 4");
    CHECK(perm_sweep_walks(5, 200).size() == 2 && perm_sweep_walks(5, 200)[1].kernel_nb == 1, "B = 5, P = 199 is not 4 + 1");
    // under a small launch budget (kad::set_launch_budget, what FAD_KAD_LAUNCH_BUDGET sets in kad.hip): the shapes of the GPU test of the cut
    for (int64_t budget : {(int64_t)1, (int64_t)1 << 18}) {
        fad::kad::set_launch_budget(budget);
        check(2700, 3, 34, 128, false, 512, "cut test, B = 3, P = 33");
        check(2700, 3, 34, 24, true, 512, "cut test f32, B = 3, P = 33");
        check(2700, 5, 301, 80, false, 512, "cut test, B = 5, P = 300");
    }
    fad::kad::set_launch_budget(0);
    // the single test through the sweep's plan, under the default budget and under one at which the largest case (820 tiles) takes 13 launches
    int64_t most = 0;
    for (int64_t budget : {(int64_t)0, (int64_t)1}) {
        fad::kad::set_launch_budget(budget);
        for (int64_t NL : {2, 32, 33, 1024, 1025, 2049, 65537})
            for (int64_t TZ : {1, 2, 3, 9, 40})
                for (int64_t depth : {16, 512, 2048})
                    for (bool f32 : {false, true})
                        for (int64_t cap : {8, 504}) check_single(TZ, NL, depth, f32, cap);
        const std::vector<PermSweepWalk> one = perm_sweep_walks(1, 2);
        most = (int64_t)perm_sweep_launches(40, one, 2048, true, 504).size();
    }
    CHECK(most > 1, "the small budget does not cut the largest case into several launches (%lld)", (long long)most);
    fad::kad::set_launch_budget(0);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK\n");
    return 0;
}
