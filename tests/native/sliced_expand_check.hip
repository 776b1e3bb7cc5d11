// The stable expansion of fadtk_amd/csrc/sliced_expand.h on its own, below fad_sliced_bootstrap: this file includes that header and
// nothing else of the library.  The count, scan and expand kernels run on given keys (one segment of N per direction), a random
// permutation of 0 .. N - 1 per direction as the row at every rank, and the count words of NB replicates; the output of every
// (direction, replicate) pair is compared bit for bit with a host loop that writes the key at rank r count[row at r] times.
//   segments 1, 3 and 17, each with its own rank -> row map;  N in {1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 6145} -- the
//   lane, wave, row and workgroup boundaries at which a prefix can go wrong;  NB in {1, 3, 4, 5, 9}: a full word, last words with
//   one and with three replicates;  replicate q of a run, by q % 6, with ranks those of segment 0:
//     0  all ones                       1  all zeros but one row (count 3, the middle rank)
//     2  a run of zeros across the first workgroup boundary (ranks 1948 .. 2147; the middle third of a shorter segment), 0 .. 3 elsewhere
//     3  255 on rank 0, on the last rank of every workgroup and on the last rank, 0 .. 2 elsewhere
//     4  0 .. 5 at random                5  0 .. 255 on a tenth of the rows, 0 elsewhere
//   The bytes of a last word past NB are 255, and must be skipped.
// Every buffer the kernels write has guard words in front and behind, and every pair's segment a few words after it (the pitch is
// longer than the largest total): nothing at or past a pair's total may be written.  Keys, rows, count words and totals must come back
// untouched.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/sliced_expand_check tests/native/sliced_expand_check.hip
#include "../../fadtk_amd/csrc/sliced_expand.h"

#include "sliced_keys.h"

#include <numeric>

using namespace fad;

static int run(int64_t segs, int64_t N, int64_t NB) {
    const int64_t W = sexpand::words(NB), G = sexpand::groups(N), guard = 64, kpitch = N + 5, cpitch = N + 7, pairs = segs * NB;
    std::mt19937 rng((uint32_t)(segs * 1000003 + N * 131 + NB * 7));

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
    const uint32_t* row0 = idx.data() + guard;                                        // the row at every rank of segment 0

    // cnt[q][row], then the words: byte b of cols[w][row] = replicate 4 w + b
    std::vector<std::vector<uint8_t>> cnt((size_t)NB, std::vector<uint8_t>((size_t)N, 0));
    for (int64_t q = 0; q < NB; ++q) {
        std::vector<uint8_t>& c = cnt[(size_t)q];
        switch (q % 6) {
            case 0: std::fill(c.begin(), c.end(), (uint8_t)1); break;
            case 1: c[row0[N / 2]] = 3; break;
            case 2: {
                const int64_t z0 = N > 2148 ? 1948 : N / 3, z1 = N > 2148 ? 2148 : 2 * N / 3;
                for (int64_t r = 0; r < N; ++r) c[row0[r]] = r >= z0 && r < z1 ? 0 : (uint8_t)(rng() % 4);
                break;
            }
            case 3:
                for (int64_t r = 0; r < N; ++r)
                    c[row0[r]] = r == 0 || r == N - 1 || r % sexpand::kShare == sexpand::kShare - 1 ? 255 : (uint8_t)(rng() % 3);
                break;
            case 4: for (int64_t r = 0; r < N; ++r) c[(size_t)r] = (uint8_t)(rng() % 6); break;
            default: for (int64_t r = 0; r < N; ++r) c[(size_t)r] = rng() % 10 == 0 ? (uint8_t)(rng() % 256) : 0;
        }
    }
    std::vector<uint32_t> cols((size_t)(W * cpitch + 2 * guard), kGuard);
    for (int64_t w = 0; w < W; ++w)
        for (int64_t j = 0; j < N; ++j) {
            uint32_t v = 0;
            for (int b = 0; b < 4; ++b) v |= (uint32_t)(4 * w + b < NB ? cnt[(size_t)(4 * w + b)][(size_t)j] : 255) << (8 * b);
            cols[(size_t)(guard + w * cpitch + j)] = v;
        }
    std::vector<uint32_t> total((size_t)(NB + 2 * guard), kGuard);
    int64_t most = 0;
    for (int64_t q = 0; q < NB; ++q) {
        const int64_t t = std::accumulate(cnt[(size_t)q].begin(), cnt[(size_t)q].end(), (int64_t)0);
        total[(size_t)(guard + q)] = (uint32_t)t;
        most = std::max(most, t);
    }
    const int64_t pitch = most + 5, out_total = pairs * pitch + 2 * guard;
    const int64_t nc = sexpand::counts_elems(N, segs, W), count_total = nc + 2 * guard;
    std::vector<uint32_t> fill((size_t)std::max(out_total, count_total), kGuard);

    uint32_t *keys_d, *idx_d, *cols_d, *total_d, *out_d, *counts_d;
    CK(hipMalloc(&keys_d, keys.size() * 4)); CK(hipMalloc(&idx_d, idx.size() * 4)); CK(hipMalloc(&cols_d, cols.size() * 4));
    CK(hipMalloc(&total_d, total.size() * 4)); CK(hipMalloc(&out_d, (size_t)out_total * 4)); CK(hipMalloc(&counts_d, (size_t)count_total * 4));
    CK(hipMemcpy(keys_d, keys.data(), keys.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(idx_d, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(cols_d, cols.data(), cols.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(total_d, total.data(), total.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(out_d, fill.data(), (size_t)out_total * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(counts_d, fill.data(), (size_t)count_total * 4, hipMemcpyHostToDevice));

    const sexpand::Args a{reinterpret_cast<const float*>(keys_d + guard), idx_d + guard, kpitch, N, cols_d + guard, cpitch, segs, W, G, NB,
                          counts_d + guard, reinterpret_cast<float*>(out_d + guard), pitch, reinterpret_cast<const int32_t*>(total_d + guard)};
    CK(sexpand::expand_segments(a, nullptr));
    CK(hipDeviceSynchronize());

    std::vector<uint32_t> out((size_t)out_total), counts((size_t)count_total), keys_b(keys.size()), idx_b(idx.size()), cols_b(cols.size()),
        total_b(total.size());
    CK(hipMemcpy(out.data(), out_d, out.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(counts.data(), counts_d, counts.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(keys_b.data(), keys_d, keys.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(idx_b.data(), idx_d, idx.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(cols_b.data(), cols_d, cols.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(total_b.data(), total_d, total.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(keys_d)); CK(hipFree(idx_d)); CK(hipFree(cols_d)); CK(hipFree(total_d)); CK(hipFree(out_d)); CK(hipFree(counts_d));

    int bad = 0;
    std::vector<uint32_t> want((size_t)pitch);
    for (int64_t s = 0; s < segs; ++s)
        for (int64_t q = 0; q < NB; ++q) {
            std::fill(want.begin(), want.end(), kGuard);
            int64_t at = 0;
            for (int64_t r = 0; r < N; ++r)
                for (int c = cnt[(size_t)q][idx[(size_t)(guard + s * kpitch + r)]]; c > 0; --c) want[(size_t)at++] = keys[(size_t)(guard + s * kpitch + r)];
            const int64_t pair = s * NB + q;
            for (int64_t i = 0; i < pitch; ++i) bad += out[(size_t)(guard + pair * pitch + i)] != want[(size_t)i];
        }
    for (int64_t i = 0; i < guard; ++i) {
        bad += out[(size_t)i] != kGuard || out[(size_t)(out_total - 1 - i)] != kGuard;
        bad += counts[(size_t)i] != kGuard || counts[(size_t)(count_total - 1 - i)] != kGuard;
    }
    bad += keys_b != keys;
    bad += idx_b != idx;
    bad += cols_b != cols;
    bad += total_b != total;
    char what[64];
    snprintf(what, sizeof(what), "%lld replicates, segments x N", (long long)NB);
    expect_none(bad, what, 0, segs, N);
    return 0;
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    const int64_t lengths[] = {1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 6145};
    const int64_t counts[] = {1, 3, 17};
    const int64_t replicates[] = {1, 3, 4, 5, 9};
    for (int64_t segs : counts)
        for (int64_t N : lengths)
            for (int64_t NB : replicates) {
                const int rc = run(segs, N, NB);
                if (rc) return rc;
            }
    return report();
}
