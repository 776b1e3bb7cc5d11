// The votes of the leave-one-out k-NN two-sample test (fad_nn_test): 32 labellings per 32-bit word, classified together.
//
// A word holds one pooled row's labels under 32 labellings (bit l = labelling 32 w + l; 1 = "baseline").  The k neighbours' words are
// added into a bit-sliced counter of four bit planes (plane b holds bit b of every lane's count, so 32 counts of 0 .. 15 take four
// words); one more word is added by a ripple of half-adders.  The majority word has bit l set when more than k / 2 of the k labels of
// lane l are 1 (k odd, 1 .. 15: no ties), by a bit-sliced compare of the planes with (k + 1) / 2.  A row is correct under labelling l
// when the majority bit equals its own: okx for own = 1 ("baseline" rows), oky for own = 0.
//
// The pure functions are host and device code, so that tests/native_cpu/nn_vote_check.cpp checks on the CPU the very code the kernel
// runs.  The kernel itself is compiled by hipcc alone.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define NNV_HD __host__ __device__
#else
#define NNV_HD
#endif

namespace fad {
namespace nnv {

constexpr int kMaxVotes = 15;                              // four planes count to 15
constexpr int kVoteRows = 4096;                            // pooled rows per workgroup of nn_vote_kernel

struct Planes { uint32_t c[4]; };                          // bit b of lane l's count is bit l of c[b]

NNV_HD inline Planes planes_zero() { return Planes{{0u, 0u, 0u, 0u}}; }

// count += a, lane by lane (at most kMaxVotes words: the carry out of plane 3 is dropped)
NNV_HD inline void add_word(Planes& p, uint32_t a) {
    uint32_t carry = a;
    for (int b = 0; b < 4; ++b) {
        const uint32_t t = p.c[b] & carry;
        p.c[b] ^= carry;
        carry = t;
    }
}

// bit l = (lane l's count >= (k + 1) / 2): the majority of k votes, k odd
NNV_HD inline uint32_t majority(const Planes& p, int k) {
    const int h = (k + 1) / 2;
    uint32_t gt = 0u, eq = ~0u;
    for (int b = 3; b >= 0; --b) {
        const uint32_t hb = (h >> b) & 1 ? ~0u : 0u;
        gt |= eq & p.c[b] & ~hb;
        eq &= ~(p.c[b] ^ hb);
    }
    return gt | eq;
}

// the lanes where the prediction is right, split by the row's own label
NNV_HD inline void split_correct(uint32_t maj, uint32_t own, uint32_t* okx, uint32_t* oky) {
    const uint32_t same = ~(maj ^ own);
    *okx = same & own;
    *oky = same & ~own;
}

#if defined(__HIPCC__)
// Workgroup (x: a range of kVoteRows rows, y: labelling word w).  A thread takes a row j < N: its own word and its k neighbours' words
// of cols[w * z_pad + .] (kad_perm_colbits_kernel's layout), the majority and the two correctness words.  The per-labelling counts
// over rows go through kad_perm_colbits_kernel's ballot transpose: for bit r the wave's popcount is added to the running count of
// lane r (correct_x) and of lane 32 + r (correct_y).  The workgroup's 64 sums are added to counts[(32 w + l) * 2 + {0: x, 1: y}] by
// integer atomics: the order does not matter.  A neighbour index outside [0, N) (never produced for k <= N - 1) votes 0.
__global__ void __launch_bounds__(256) nn_vote_kernel(const uint32_t* __restrict__ cols, int64_t z_pad, const int32_t* __restrict__ nn, int k,
                                                      int64_t N, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int red[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t w = blockIdx.y, j0 = (int64_t)blockIdx.x * kVoteRows, j1 = j0 + kVoteRows < N ? j0 + kVoteRows : N;
    const uint32_t* cw = cols + w * z_pad;
    unsigned int mine = 0;
    for (int64_t base = j0; base < j1; base += 256) {                                 // uniform over the workgroup
        const int64_t j = base + tid;
        uint32_t okx = 0u, oky = 0u;
        if (j < j1) {
            Planes p = planes_zero();
            for (int q = 0; q < k; ++q) {
                const uint32_t i = (uint32_t)nn[j * k + q];
                add_word(p, i < (uint64_t)N ? cw[i] : 0u);
            }
            split_correct(majority(p, k), cw[j], &okx, &oky);
        }
        for (int r = 0; r < 32; ++r) {
            const unsigned int bx = (unsigned int)__popcll(__ballot((okx >> r) & 1u));
            const unsigned int by = (unsigned int)__popcll(__ballot((oky >> r) & 1u));
            if ((lane & 31) == r) mine += lane < 32 ? bx : by;
        }
    }
    red[wave][lane] = mine;
    __syncthreads();
    if (wave == 0) {
        const unsigned long long s = (unsigned long long)red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
        if (s) atomicAdd(&counts[(32 * w + (lane & 31)) * 2 + (lane >> 5)], s);
    }
}
#endif

}  // namespace nnv
}  // namespace fad
