// Stand-alone check of kad::perm_aggregate (fadtk_amd/csrc/kad_perm_sweep_tiles.h), the counting behind fad_kad_aggregate, against the
// definition evaluated by brute force -- built with -fsanitize=address,undefined by tests/test_kad_aggregate_host.py and run on the CPU.
#include "../../fadtk_amd/csrc/kad_perm_sweep_tiles.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t state = 0x9e3779b97f4a7c15ull;
static double next() {                                    // xorshift64*: uniform in [0, 1)
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return (double)((state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

static void brute(const std::vector<double>& t, int B, int64_t L, std::vector<double>* pv, double* pa) {
    std::vector<int64_t> least((size_t)L, L + 1);
    pv->assign((size_t)B, 0.0);
    for (int b = 0; b < B; ++b)
        for (int64_t j = 0; j < L; ++j) {
            int64_t ge = 0;
            for (int64_t i = 0; i < L; ++i) ge += t[(size_t)(b * L + i)] >= t[(size_t)(b * L + j)];
            if (j == 0) (*pv)[(size_t)b] = (double)ge / (double)L;
            if (ge < least[(size_t)j]) least[(size_t)j] = ge;
        }
    int64_t le = 0;
    for (int64_t j = 0; j < L; ++j) le += least[(size_t)j] <= least[0];
    *pa = (double)le / (double)L;
}

static void check(int B, int64_t L, int levels, bool nan, const char* label) {
    std::vector<double> t((size_t)(B * L));
    for (double& v : t) v = levels ? std::floor(next() * levels) : next();      // levels > 0: exact ties
    if (nan) t[(size_t)(next() * (double)t.size())] = NAN;
    std::vector<double> want, got((size_t)B, -1.0);
    double want_a, got_a = -1.0;
    brute(t, B, L, &want, &want_a);
    fad::kad::perm_aggregate(t.data(), B, L, got.data(), &got_a);
    for (int b = 0; b < B; ++b) CHECK(got[(size_t)b] == want[(size_t)b], "%s: p_values[%d] = %.17g, not %.17g", label, b, got[(size_t)b], want[(size_t)b]);
    CHECK(got_a == want_a, "%s: p_aggregated = %.17g, not %.17g", label, got_a, want_a);
    if (B == 1) CHECK(got_a == got[0], "%s: one bandwidth, p_aggregated %.17g != p_value %.17g", label, got_a, got[0]);
}

int main() {
    for (int rep = 0; rep < 20; ++rep) {
        check(1, 2, 0, false, "B = 1, P = 1");
        check(1, 200, 0, false, "B = 1");
        check(5, 200, 0, false, "B = 5");
        check(16, 1000, 0, false, "B = 16, P = 999");
        check(4, 2, 2, false, "P = 1 with ties");
        check(7, 100, 3, false, "ties on 3 levels");
        check(3, 64, 1, false, "all equal");
        check(4, 50, 0, true, "a NaN");
    }
    // NULL outputs are skipped, not written
    double t[4] = {1.0, 0.0, 0.5, 2.0}, pa = -1.0;
    fad::kad::perm_aggregate(t, 2, 2, nullptr, &pa);
    CHECK(pa == 1.0, "p_aggregated %.17g", pa);      // each labelling is the extreme one at one bandwidth: min counts 1 and 1
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK\n");
    return 0;
}
