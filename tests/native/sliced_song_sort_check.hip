// The resident song sort of fadtk_amd/csrc/sliced_song_sort.h on its own, below fad_sliced_individual: this file includes that header
// (which stands on sliced_sort.h) and nothing else of the library.  Every song's range of every direction is compared bit for bit with
// std::sort of the mapped uint32 keys (mapped back), over the key sets of sliced_sort_check -- denormals, -0 and +0 together, +-FLT_MAX,
// infinities and NaN bit patterns, keys that share three of their four bytes (per byte position), all keys equal, sorted and reversed
// input, raw random words -- at 1, 3 and 65 directions and over song-length patterns on every edge of the unit table: one key, 600
// one-key songs (more than a unit may hold), lengths round the wave and round sizes, C - 1, C, {C, 1}, {1, C}, a run that sums to
// exactly C followed by one key, and songs without keys first, in the middle and last.  The words after each row (the pitch is longer
// than the rows) and the guard words around the buffer must come back untouched.  The unit table itself is checked on the host.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/sliced_song_sort_check tests/native/sliced_song_sort_check.hip
#include "../../fadtk_amd/csrc/sliced_song_sort.h"

#include "sliced_keys.h"

using namespace fad;

static const int64_t C = songsort::kCapacity;

// sliced_keys.h's key set `kind` for direction s, element i of n, with NaN bit patterns let in: among the special values of kind 2,
// wherever the shared bytes of kinds 3 .. 6 make one, and kind 10 is any word at all
static uint32_t song_key(int kind, int64_t s, int64_t i, int64_t n, std::mt19937& rng) {
    switch (kind) {
        case 2: {
            static const uint32_t nan[] = {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu};
            const uint32_t r = rng() % 16;
            return r < 12 ? bits_of(kSpecial[r]) : nan[r - 12];
        }
        case 3: case 4: case 5: case 6: return shared_bytes_key(kind, s, rng);
        case 10: return rng();
        default: return make_key(kind, s, i, n, rng);
    }
}

static int run(int kind, int pat, const std::vector<int64_t>& lens, int64_t dirs) {
    const int64_t n_songs = (int64_t)lens.size();
    std::vector<int64_t> off((size_t)n_songs + 1, 0);
    for (int64_t s = 0; s < n_songs; ++s) off[(size_t)s + 1] = off[(size_t)s] + lens[(size_t)s];
    const int64_t n = off[(size_t)n_songs];
    const songsort::Table t = songsort::build_units(off.data(), n_songs);
    if (!t.long_songs.empty()) { printf("pattern %d has a song beyond the capacity\n", pat); return 2; }
    const int64_t pitch = n + 5, guard = 64, total = dirs * pitch + 2 * guard;
    std::mt19937 rng((uint32_t)(kind * 1000003 + pat * 7919 + dirs));
    std::vector<uint32_t> host((size_t)total, kGuard), back((size_t)total);
    for (int64_t l = 0; l < dirs; ++l)
        for (int64_t i = 0; i < n; ++i) host[(size_t)(guard + l * pitch + i)] = song_key(kind, l, i, n, rng);
    uint32_t* keys;
    songsort::Unit* units_d;
    int32_t* ends_d;
    CK(hipMalloc(&keys, (size_t)total * 4));
    CK(hipMalloc(&units_d, t.units.size() * sizeof(songsort::Unit)));
    CK(hipMalloc(&ends_d, t.ends.size() * sizeof(int32_t)));
    CK(hipMemcpy(keys, host.data(), (size_t)total * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(units_d, t.units.data(), t.units.size() * sizeof(songsort::Unit), hipMemcpyHostToDevice));
    CK(hipMemcpy(ends_d, t.ends.data(), t.ends.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    CK(songsort::sort_units(reinterpret_cast<float*>(keys + guard), pitch, dirs, units_d, ends_d, (int64_t)t.units.size(), nullptr));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(back.data(), keys, (size_t)total * 4, hipMemcpyDeviceToHost));
    CK(hipFree(keys)); CK(hipFree(units_d)); CK(hipFree(ends_d));

    int bad = 0;
    std::vector<uint32_t> want;
    for (int64_t l = 0; l < dirs; ++l) {
        const size_t row = (size_t)(guard + l * pitch);
        for (int64_t s = 0; s < n_songs; ++s) {
            const int64_t o = off[(size_t)s], m = lens[(size_t)s];
            want.resize((size_t)m);
            for (int64_t i = 0; i < m; ++i) want[(size_t)i] = ssort::key_image(host[row + (size_t)(o + i)]);
            std::sort(want.begin(), want.end());
            for (int64_t i = 0; i < m; ++i) bad += back[row + (size_t)(o + i)] != ssort::key_bits(want[(size_t)i]);
        }
        for (int64_t i = n; i < pitch; ++i) bad += back[row + (size_t)i] != kGuard;
    }
    for (int64_t i = 0; i < guard; ++i) bad += back[(size_t)i] != kGuard || back[(size_t)(total - 1 - i)] != kGuard;
    expect_none(bad, "pattern x directions", kind, pat, dirs);
    return 0;
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    std::vector<std::vector<int64_t>> pats = {
        {1},
        std::vector<int64_t>(600, 1),
        {1, 2, 3, 255, 256, 257, 300},
        {C - 1},
        {C},
        {C, 1},
        {1, C},
        {C / 2, C / 4 - 7, C / 4 + 7, 1},
        {0, 0, 5, 0, 0, 700, 513, 0},
    };
    // the unit table on the host: no song cut, no unit over the capacity or the slot count, long songs apart
    {
        auto table = [](const std::vector<int64_t>& lens) {
            std::vector<int64_t> off(lens.size() + 1, 0);
            for (size_t s = 0; s < lens.size(); ++s) off[s + 1] = off[s] + lens[s];
            return songsort::build_units(off.data(), (int64_t)lens.size());
        };
        songsort::Table t = table(pats[1]);
        expect(t.units.size() == 3 && t.most_songs == songsort::kMaxSlots && t.units[2].ns == 600 - 2 * songsort::kMaxSlots, "600 one-key songs");
        t = table(pats[5]);
        expect(t.units.size() == 2 && t.units[0].nk == C && t.units[1].nk == 1 && t.units[1].k0 == C, "{C, 1}");
        t = table(pats[6]);
        expect(t.units.size() == 2 && t.units[0].nk == 1 && t.units[1].nk == C && t.units[1].k0 == 1, "{1, C}");
        t = table(pats[7]);
        expect(t.units.size() == 2 && t.units[0].nk == C && t.units[0].ns == 3 && t.units[1].nk == 1, "a run of exactly C, then one key");
        t = table(pats[8]);
        expect(t.units.size() == 1 && t.units[0].k0 == 0 && t.units[0].nk == 1218 && t.units[0].ns == 3 && t.ends.size() == 3, "empty songs");
        t = table({5, C + 1, 0, 2 * C + 5, 6});
        expect(t.units.size() == 2 && t.long_songs.size() == 2 && t.long_songs[0] == 1 && t.long_songs[1] == 3 && t.units[1].k0 == 3 * C + 11,
               "long songs end the run");
        t = table({0, 0});
        expect(t.units.empty() && t.ends.empty() && t.long_songs.empty(), "no keys at all");
    }
    const int64_t counts[] = {1, 3, 65};
    for (int kind = 0; kind < 11; ++kind)
        for (int pat = 0; pat < (int)pats.size(); ++pat)
            for (int64_t dirs : counts) {
                const int rc = run(kind, pat, pats[(size_t)pat], dirs);
                if (rc) return rc;
            }
    return report();
}
