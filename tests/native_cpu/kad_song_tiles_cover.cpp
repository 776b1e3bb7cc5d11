// CPU check of fadtk_amd/csrc/kad_song_tiles.h, the work units of the per-song KAD passes (fad_kad_individual, kad.hip): over the
// launches a pass is cut into and the persistent walk of each launch's workgroups, the cross units take every tile of the X x Y
// rectangle exactly once (so every (x, y) pair once), the band units with band_pair_counted count every pair i < j inside a song
// exactly once and no pair across songs, a column block's band units are the contiguous run band_start[J] .. band_start[J + 1],
// and no launch takes more tiles than kad::tiles_per_launch allows.
#include "../../fadtk_amd/csrc/kad_song_tiles.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fad::kad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// every unit a pass's launches (the host's launch cut) hand out, as the workgroups of each launch meet them; `tiles(u)` is a unit's
// tile count
template <typename T, typename F>
static void walk_units(int64_t total, int64_t per_launch, int64_t cap, int64_t tile_cap, T&& tiles, F&& take) {
    for (const Launch& l : launches(total, per_launch, cap)) {
        const int64_t u0 = l.u0, cnt = l.cnt, G = l.grid;
        CHECK(G % kXcds == 0 && G >= kXcds && G <= launch_slots(cnt), "grid %lld for %lld units", (long long)G, (long long)cnt);
        int64_t launch_tiles = 0;
        for (int64_t w = 0; w < G; ++w)
            for (int64_t L = w; L < launch_slots(cnt); L += G) {
                bool live;
                const int64_t v = slot_tile(L, cnt, &live);
                if (!live) continue;
                CHECK(v >= 0 && v < cnt, "slot %lld -> %lld of %lld", (long long)L, (long long)v, (long long)cnt);
                launch_tiles += tiles(u0 + v);
                take(u0 + v);
            }
        CHECK(launch_tiles <= tile_cap, "a launch of %lld tiles, cap %lld", (long long)launch_tiles, (long long)tile_cap);
    }
}

static void check_cross(int64_t n, int64_t m, int64_t depth, bool f32, int64_t cap) {
    const int64_t TI = blocks(n), TJ = blocks(m), per = tiles_per_launch(depth, f32);
    const int64_t rr = cross_rows_per_unit(TI, TJ, per), NR = cross_ranges(TI, rr);
    CHECK(rr >= 1 && rr <= per && NR * rr >= TI && (NR - 1) * rr < TI, "n %lld m %lld: rr %lld NR %lld", (long long)n, (long long)m,
          (long long)rr, (long long)NR);
    std::vector<unsigned char> seen((size_t)(TI * TJ), 0);
    walk_units(NR * TJ, units_per_launch(rr, depth, f32), cap, per,
               [&](int64_t u) { const Unit t = cross_unit(u, TI, TJ, rr); return t.I1 - t.I0; },
               [&](int64_t u) {
                   const Unit t = cross_unit(u, TI, TJ, rr);
                   CHECK(t.J >= 0 && t.J < TJ && t.I0 >= 0 && t.I0 < t.I1 && t.I1 <= TI && t.I0 == (u / TJ) * rr,
                         "unit %lld -> J %lld rows [%lld, %lld)", (long long)u, (long long)t.J, (long long)t.I0, (long long)t.I1);
                   for (int64_t I = t.I0; I < t.I1; ++I) seen[(size_t)(I * TJ + t.J)]++;
               });
    for (size_t k = 0; k < seen.size(); ++k)
        CHECK(seen[k] == 1, "n %lld m %lld: tile (%lld, %lld) taken %d times", (long long)n, (long long)m, (long long)(k / TJ),
              (long long)(k % TJ), seen[k]);
}

// songs of the given lengths, concatenated; every pair counted by the band units, checked against the songs
static void check_band(const std::vector<int64_t>& lens, int64_t depth, bool f32, int64_t cap, const char* label) {
    std::vector<int64_t> off(1, 0);
    for (int64_t l : lens) off.push_back(off.back() + l);
    const int64_t S = (int64_t)lens.size(), M = off.back();
    if (M == 0) return;
    const int64_t TJ = blocks(M);
    std::vector<int64_t> song((size_t)(TJ * kTile), -1), end((size_t)(TJ * kTile), 0);      // per row; padding: no song, end 0
    for (int64_t s = 0; s < S; ++s)
        for (int64_t i = off[s]; i < off[s + 1]; ++i) { song[(size_t)i] = s; end[(size_t)i] = off[s + 1]; }
    for (int64_t i = 0; i < M; i += 37) CHECK(off[song_of_row(off.data(), S, i) + 1] == end[(size_t)i], "%s: song_of_row(%lld)", label, (long long)i);

    std::vector<Unit> units;
    std::vector<int64_t> start;
    band_units(off.data(), S, &units, &start);
    CHECK((int64_t)start.size() == TJ + 1 && start[0] == 0 && start[TJ] == (int64_t)units.size(), "%s: band_start", label);
    for (int64_t J = 0; J < TJ; ++J)
        for (int64_t u = start[J]; u < start[J + 1]; ++u)
            CHECK(units[u].J == J && units[u].I0 < units[u].I1 && units[u].I1 <= J + 1 && units[u].I1 - units[u].I0 <= kBandPiece,
                  "%s: unit %lld of J %lld", label, (long long)u, (long long)J);

    const bool full = M <= 4096;                   // small sets: every pair has a counter; large ones: counts and per-pair checks
    std::vector<unsigned char> seen(full ? (size_t)(M * M) : 0, 0);
    std::vector<unsigned char> tile_seen((size_t)(TJ * TJ), 0);
    int64_t counted = 0;
    walk_units((int64_t)units.size(), units_per_launch(kBandPiece, depth, f32), cap, tiles_per_launch(depth, f32),
               [&](int64_t u) { return units[u].I1 - units[u].I0; },
               [&](int64_t u) {
                   const Unit t = units[u];
                   for (int64_t I = t.I0; I < t.I1; ++I) {
                       CHECK(tile_seen[(size_t)(I * TJ + t.J)]++ == 0, "%s: tile (%lld, %lld) twice", label, (long long)I, (long long)t.J);
                       // the kernel's one-song tile (no compare: every pair, or c > r on the diagonal)
                       const bool one_song = end[(size_t)(I * kTile)] >= (t.J + 1) * kTile;
                       const int64_t one_song_pairs = I < t.J ? (int64_t)kTile * kTile : (int64_t)kTile * (kTile - 1) / 2;
                       if (one_song) CHECK(song[(size_t)(I * kTile)] == song[(size_t)(t.J * kTile + kTile - 1)], "%s: one-song tile", label);
                       if (!full && one_song) {
                           counted += one_song_pairs;
                           continue;
                       }
                       const int64_t before = counted;
                       for (int r = 0; r < kTile; ++r)
                           for (int c = 0; c < kTile; ++c) {
                               const int64_t i = I * kTile + r, j = t.J * kTile + c;
                               if (!band_pair_counted(I, t.J, r, c, end[(size_t)i])) continue;
                               CHECK(i < j && j < M && song[(size_t)i] == song[(size_t)j] && song[(size_t)i] >= 0,
                                     "%s: pair (%lld, %lld) of songs %lld / %lld counted", label, (long long)i, (long long)j,
                                     (long long)song[(size_t)i], (long long)song[(size_t)j]);
                               ++counted;
                               if (full && i < M && j < M) seen[(size_t)(i * M + j)]++;
                           }
                       if (one_song) CHECK(counted - before == one_song_pairs, "%s: one-song tile (%lld, %lld)", label, (long long)I, (long long)t.J);
                   }
               });
    int64_t want = 0;
    for (int64_t l : lens) want += l * (l - 1) / 2;
    CHECK(counted == want, "%s: %lld pairs counted, %lld inside songs", label, (long long)counted, (long long)want);
    if (full)
        for (int64_t i = 0; i < M; ++i)
            for (int64_t j = i + 1; j < M; ++j)
                CHECK(seen[(size_t)(i * M + j)] == (song[(size_t)i] == song[(size_t)j] ? 1 : 0), "%s: pair (%lld, %lld) counted %d times",
                      label, (long long)i, (long long)j, seen[(size_t)(i * M + j)]);
}

int main() {
    // cross: small and ragged, the 10 000 two-frame songs against 10^5 rows, 2 000 x 2 250 frames, a one-row song set
    const int64_t cross[][2] = {{2, 1}, {129, 300}, {3000, 5000}, {100000, 20000}, {100000, 48000}, {100000, 4500000}, {1000000, 129}};
    for (auto& c : cross) {
        check_cross(c[0], c[1], 768, false, 512);
        check_cross(c[0], c[1], 2048, true, 512);
    }
    check_cross(100000, 4500000, 128, false, 8);

    srand(7);
    std::vector<int64_t> edge = {0, 1, 2, 127, 128, 129, 0, 3, 300, 1, 2, 127, 128, 129};
    check_band(edge, 768, false, 512, "edge lengths");
    check_band(edge, 2048, true, 8, "edge lengths f32");
    std::vector<int64_t> straddle;
    for (int k = 0; k < 20; ++k) straddle.push_back(k % 2 ? 2 : 127);          // songs that cross every tile edge
    check_band(straddle, 128, false, 512, "straddling");
    std::vector<int64_t> many;
    for (int k = 0; k < 700; ++k) many.push_back(rand() % 6);                 // many songs per tile, empty ones among them
    check_band(many, 512, false, 512, "many per tile");
    std::vector<int64_t> two(3000, 2);
    check_band(two, 768, false, 512, "two-frame songs");
    check_band({3, 100000, 129, 0, 1, 2}, 768, false, 512, "one 10^5-frame song");
    check_band({100000}, 2048, true, 512, "one 10^5-frame song alone, f32");
    std::vector<int64_t> mixed = {1, 100000};
    for (int k = 0; k < 300; ++k) mixed.push_back(rand() % 400);
    check_band(mixed, 128, false, 512, "a long song among short ones");

    // under a small launch budget (kad::set_launch_budget, what FAD_KAD_LAUNCH_BUDGET sets in kad.hip): the shapes of the GPU test of the cut
    for (int64_t budget : {(int64_t)1, (int64_t)1 << 18}) {
        set_launch_budget(budget);
        CHECK(units_per_launch(1, 128, false) == tiles_per_launch(128, false) && units_per_launch(kBandPiece, 128, false) == tiles_per_launch(128, false) / kBandPiece,
              "units_per_launch reads the budget");
        if (budget == 1) CHECK(units_per_launch(1, 128, false) == 64 && units_per_launch(kBandPiece, 2048, true) == 2, "the floor at budget 1");
        check_cross(1290, 1410, 128, false, 512);
        check_cross(1290, 1410, 24, true, 512);
        check_band({0, 1, 2, 127, 129, 300, 851}, 128, false, 512, "the cut test's songs");
        check_band({0, 1, 2, 127, 129, 300, 851}, 24, true, 512, "the cut test's songs f32");
    }
    set_launch_budget(0);
    printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
