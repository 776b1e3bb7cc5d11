// The stable split of fadtk_amd/csrc/sliced_split.h on its own, below fad_sliced_permutation_test: this file includes that header and
// nothing else of the library.  The count, scan and split kernels run on given keys (one segment of N per direction), a random
// permutation of 0 .. N - 1 per direction as the row at every rank, and the label words of NL labellings; both outputs of every
// (direction, labelling) pair are compared bit for bit with std::stable_partition of the segment's keys by the label of the row at
// their rank.
//   segments 1, 3 and 65;  N in {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4100, 10 007} -- the lane, wave, row and
//   workgroup boundaries at which a prefix can go wrong;  NL in {1, 32, 33, 70}: a full word, a last word with one and with six
//   labellings;  ones counts 1, N - 1 and N / 2 (all three at 1 and 3 segments; at 65 segments one of the three per run, in turn);
//   labelling q of a run: ones first, ones last, alternating, random, by q % 4.
// Every buffer the kernels write has guard words in front and behind, and every pair's segment a few words after it (the pitch is
// longer than the segment): nothing outside [0, n1) and [0, n0) may be written.  Keys, rows and label words must come back untouched.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/sliced_split_check tests/native/sliced_split_check.hip
#include "../../fadtk_amd/csrc/sliced_split.h"

#include "sliced_keys.h"

#include <numeric>
#include <utility>

using namespace fad;

static int run(int64_t segs, int64_t N, int64_t NL, int64_t n1) {
    const int64_t n0 = N - n1, W = (NL + 31) / 32, G = ssplit::groups(N), guard = 64;
    const int64_t kpitch = N + 5, cpitch = N + 7, pitch1 = n1 + 3, pitch0 = n0 + 5, pairs = segs * NL;
    std::mt19937 rng((uint32_t)(segs * 1000003 + N * 131 + NL * 7 + n1));

    // labels[q][row], then the words: bit b of cols[w][row] = labelling 32 w + b; bits past NL are set, and must be skipped
    std::vector<std::vector<uint8_t>> lab((size_t)NL, std::vector<uint8_t>((size_t)N, 0));
    for (int64_t q = 0; q < NL; ++q) {
        std::vector<uint8_t>& u = lab[(size_t)q];
        switch (q % 4) {
            case 0: for (int64_t j = 0; j < n1; ++j) u[(size_t)j] = 1; break;
            case 1: for (int64_t j = 0; j < n1; ++j) u[(size_t)(N - 1 - j)] = 1; break;
            case 2: {
                int64_t left = n1;
                for (int64_t j = 0; j < N && left > 0; j += 2, --left) u[(size_t)j] = 1;
                for (int64_t j = 1; j < N && left > 0; j += 2, --left) u[(size_t)j] = 1;
                break;
            }
            default: {
                std::vector<int64_t> rows((size_t)N);
                std::iota(rows.begin(), rows.end(), 0);
                std::shuffle(rows.begin(), rows.end(), rng);
                for (int64_t j = 0; j < n1; ++j) u[(size_t)rows[(size_t)j]] = 1;
            }
        }
    }
    std::vector<uint32_t> cols((size_t)(W * cpitch + 2 * guard), kGuard);
    for (int64_t w = 0; w < W; ++w)
        for (int64_t j = 0; j < N; ++j) {
            uint32_t v = 0;
            for (int b = 0; b < 32; ++b) v |= (uint32_t)(32 * w + b < NL ? lab[(size_t)(32 * w + b)][(size_t)j] : 1) << b;
            cols[(size_t)(guard + w * cpitch + j)] = v;
        }
    std::vector<uint32_t> keys((size_t)(segs * kpitch + 2 * guard), kGuard), idx(keys.size(), kGuard);
    for (int64_t s = 0; s < segs; ++s) {
        std::vector<uint32_t> perm((size_t)N);
        std::iota(perm.begin(), perm.end(), 0u);
        std::shuffle(perm.begin(), perm.end(), rng);
        for (int64_t r = 0; r < N; ++r) {
            uint32_t k = rng();
            if (k == kGuard) k = 0;
            keys[(size_t)(guard + s * kpitch + r)] = k;
            idx[(size_t)(guard + s * kpitch + r)] = perm[(size_t)r];
        }
    }
    const int64_t one_total = pairs * pitch1 + 2 * guard, zero_total = pairs * pitch0 + 2 * guard;
    const int64_t nc = ssplit::counts_elems(N, segs, W), count_total = nc + 2 * guard;
    std::vector<uint32_t> fill((size_t)std::max(std::max(one_total, zero_total), count_total), kGuard);

    uint32_t *keys_d, *idx_d, *cols_d, *one_d, *zero_d, *counts_d;
    CK(hipMalloc(&keys_d, keys.size() * 4)); CK(hipMalloc(&idx_d, idx.size() * 4)); CK(hipMalloc(&cols_d, cols.size() * 4));
    CK(hipMalloc(&one_d, (size_t)one_total * 4)); CK(hipMalloc(&zero_d, (size_t)zero_total * 4)); CK(hipMalloc(&counts_d, (size_t)count_total * 4));
    CK(hipMemcpy(keys_d, keys.data(), keys.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(idx_d, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(cols_d, cols.data(), cols.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(one_d, fill.data(), (size_t)one_total * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(zero_d, fill.data(), (size_t)zero_total * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(counts_d, fill.data(), (size_t)count_total * 4, hipMemcpyHostToDevice));

    const ssplit::Args a{reinterpret_cast<const float*>(keys_d + guard), idx_d + guard, kpitch, N, cols_d + guard, cpitch, segs, W, G, NL,
                         counts_d + guard, reinterpret_cast<float*>(one_d + guard), reinterpret_cast<float*>(zero_d + guard),
                         pitch1, pitch0, n1, n0};
    CK(ssplit::split_segments(a, nullptr));
    CK(hipDeviceSynchronize());

    std::vector<uint32_t> one((size_t)one_total), zero((size_t)zero_total), counts((size_t)count_total), keys_b(keys.size()), idx_b(idx.size()),
        cols_b(cols.size());
    CK(hipMemcpy(one.data(), one_d, one.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(zero.data(), zero_d, zero.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(counts.data(), counts_d, counts.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(keys_b.data(), keys_d, keys.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(idx_b.data(), idx_d, idx.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(cols_b.data(), cols_d, cols.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(keys_d)); CK(hipFree(idx_d)); CK(hipFree(cols_d)); CK(hipFree(one_d)); CK(hipFree(zero_d)); CK(hipFree(counts_d));

    int bad = 0;
    std::vector<std::pair<uint32_t, uint8_t>> want((size_t)N);
    for (int64_t s = 0; s < segs; ++s)
        for (int64_t q = 0; q < NL; ++q) {
            for (int64_t r = 0; r < N; ++r)
                want[(size_t)r] = {keys[(size_t)(guard + s * kpitch + r)], lab[(size_t)q][idx[(size_t)(guard + s * kpitch + r)]]};
            std::stable_partition(want.begin(), want.end(), [](const auto& e) { return e.second != 0; });
            const int64_t pair = s * NL + q;
            for (int64_t i = 0; i < pitch1; ++i) bad += one[(size_t)(guard + pair * pitch1 + i)] != (i < n1 ? want[(size_t)i].first : kGuard);
            for (int64_t i = 0; i < pitch0; ++i) bad += zero[(size_t)(guard + pair * pitch0 + i)] != (i < n0 ? want[(size_t)(n1 + i)].first : kGuard);
        }
    for (int64_t i = 0; i < guard; ++i) {
        bad += one[(size_t)i] != kGuard || one[(size_t)(one_total - 1 - i)] != kGuard;
        bad += zero[(size_t)i] != kGuard || zero[(size_t)(zero_total - 1 - i)] != kGuard;
        bad += counts[(size_t)i] != kGuard || counts[(size_t)(count_total - 1 - i)] != kGuard;
    }
    bad += keys_b != keys;
    bad += idx_b != idx;
    bad += cols_b != cols;
    char what[64];
    snprintf(what, sizeof(what), "%lld labellings, %lld ones, segments x N", (long long)NL, (long long)n1);
    expect_none(bad, what, 0, segs, N);
    return 0;
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    const int64_t lengths[] = {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4100, 10007};
    const int64_t counts[] = {1, 3, 65};
    const int64_t labellings[] = {1, 32, 33, 70};
    int turn = 0;
    for (int64_t segs : counts)
        for (int64_t N : lengths)
            for (int64_t NL : labellings) {
                std::vector<int64_t> ones{1};                                         // N = 1, 2, 3: fewer than three different counts
                for (int64_t c : {N - 1, N / 2})
                    if (c >= 1 && std::find(ones.begin(), ones.end(), c) == ones.end()) ones.push_back(c);
                for (size_t c = 0; c < ones.size(); ++c) {
                    if (segs == 65 && c != (size_t)turn % ones.size()) continue;
                    const int rc = run(segs, N, NL, ones[c]);
                    if (rc) return rc;
                }
                ++turn;
            }
    return report();
}
