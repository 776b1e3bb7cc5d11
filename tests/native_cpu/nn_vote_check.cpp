// Stand-alone check of the bit-sliced votes of fad_nn_test (fadtk_amd/csrc/nn_vote.h): for every odd k <= 15 the majority word equals
// the per-bit popcount majority on all 2^k vote patterns of one bit lane with pseudo-random other lanes, the planes hold every lane's
// count, and the correct rows split by the row's own label -- built with g++ by tests/test_nn_test_host.py (once more with
// -fsanitize=address,undefined) and run on the CPU.
#include "../../fadtk_amd/csrc/nn_vote.h"

#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t next() {                                  // xorshift64*
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return (uint32_t)((state * 0x2545f4914f6cdd1dull) >> 32);
}

int main() {
    using namespace fad::nnv;
    for (int k = 1; k <= kMaxVotes; k += 2)
        for (int lane = 0; lane < 32; lane += (k > 9 ? 13 : 1))               // every lane for small k, lanes 0, 13, 26 for the long ones
            for (uint32_t pat = 0; pat < (1u << k); ++pat) {
                std::vector<uint32_t> words((size_t)k);
                int count[32] = {0};
                Planes p = planes_zero();
                for (int q = 0; q < k; ++q) {
                    uint32_t w = next() & ~(1u << lane);
                    w |= ((pat >> q) & 1u) << lane;                            // the lane under test walks all 2^k patterns
                    words[(size_t)q] = w;
                    for (int l = 0; l < 32; ++l) count[l] += (w >> l) & 1u;
                    add_word(p, w);
                }
                uint32_t want = 0;
                for (int l = 0; l < 32; ++l) {
                    const int got = (int)((p.c[0] >> l) & 1u) + 2 * (int)((p.c[1] >> l) & 1u) + 4 * (int)((p.c[2] >> l) & 1u) +
                                    8 * (int)((p.c[3] >> l) & 1u);
                    CHECK(got == count[l], "k = %d lane %d: planes hold %d, popcount %d", k, l, got, count[l]);
                    want |= (uint32_t)(2 * count[l] > k) << l;
                }
                const uint32_t maj = majority(p, k);
                CHECK(maj == want, "k = %d lane %d pattern %x: majority %08x, not %08x", k, lane, pat, maj, want);
                const uint32_t own = next();
                uint32_t okx = 1u, oky = 1u;
                split_correct(maj, own, &okx, &oky);
                for (int l = 0; l < 32; ++l) {
                    const bool m = (want >> l) & 1u, o = (own >> l) & 1u;
                    CHECK((bool)((okx >> l) & 1u) == (m == o && o), "k = %d lane %d: okx", k, l);
                    CHECK((bool)((oky >> l) & 1u) == (m == o && !o), "k = %d lane %d: oky", k, l);
                }
                CHECK((okx & oky) == 0u && (okx | oky) == ~(maj ^ own), "k = %d: okx and oky do not split the correct lanes", k);
            }
    // the extremes: no vote, every vote
    for (int k = 1; k <= kMaxVotes; k += 2) {
        Planes none = planes_zero(), all = planes_zero();
        for (int q = 0; q < k; ++q) { add_word(none, 0u); add_word(all, ~0u); }
        CHECK(majority(none, k) == 0u, "k = %d: a majority of no votes", k);
        CHECK(majority(all, k) == ~0u, "k = %d: no majority of all votes", k);
    }
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK\n");
    return 0;
}
