// The stable split of the sliced Wasserstein permutation test (fad_sliced_permutation_test): one sorted segment of N
// float32 keys per direction, the pooled row at every rank beside it, and per pooled row a word of 32 labels (bit b = labelling 32 w + b;
// 1 = the first group).  For every (direction, labelling) pair the keys go, in rank order, to the pair's label-1 buffer or to its
// label-0 buffer: a stable partition of a sorted array, so both buffers are sorted -- the sort of each group, with no sort.
//
//   - share:  a workgroup owns kShare = 2048 consecutive ranks of one (direction, labelling word), as the sort's workgroups do; wave v
//             owns the ranks [512 v, 512 v + 512) of them, read as 8 coalesced rows of 64.  A lane keeps its 8 keys and its 8 label
//             words (one gathered word per rank serves 32 labellings) in registers.
//   - count:  per (direction, word, workgroup) the ones of each of the 32 labellings, from 8 ballots per labelling and wave, the four
//             waves summed through LDS.  Stored whole: counts [D][W][G][32].
//   - scan:   one thread per (direction, word, labelling) walks the G workgroups in order into exclusive prefixes.  Integers.
//   - split:  the count's front half again, then for labelling b the key at rank r goes to
//                 ones(r) = prefix[workgroup][b] + ones in earlier waves + ones in this wave's earlier rows + ones in lower lanes
//             of the label-1 buffer when its bit is set, and to r - ones(r) of the label-0 buffer when not.  The place is a function of
//             the rank alone: nothing is placed by order of arrival, no atomic is used, the output does not depend on timing.
// Bits of labellings past the last one (nbits < 32 in the last word) are skipped.  Every store carries an index guard that is always
// true for labellings with n1 ones: a wrong label word cannot write outside its pair's buffers.
//
// Pairs are numbered direction-major within a launch: pair (dl, q) = dl * nq + q, q the labelling's index within the launch's words
// (0 .. nq - 1, nq = the launch's labellings), its buffers at one[pair * pitch1] and zero[pair * pitch0].
//
// This header stands alone (tests/native/sliced_split_check.hip includes only it).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fad {
namespace ssplit {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 8;                                   // rows of 64 ranks per wave
constexpr int kWaveShare = 64 * kRows;                     // ranks per wave
constexpr int kShare = kWaves * kWaveShare;                // ranks of a segment per workgroup: the sort's 2048

inline int64_t groups(int64_t N) { return (N + kShare - 1) / kShare; }
// uint32 of counts for D directions x W words
inline int64_t counts_elems(int64_t N, int64_t D, int64_t W) { return D * W * groups(N) * 32; }

#if defined(__HIPCC__)
struct Args {
    const float* keys; const uint32_t* idx;    // [D x kpitch]: the sorted keys and the pooled row at every rank
    int64_t kpitch, N;
    const uint32_t* cols;                      // [W x cpitch]: the label words of the launch's W labelling words, per pooled row
    int64_t cpitch;
    int64_t D, W, G;                           // directions, words, workgroups per segment: the grid is D * W * G
    int64_t nq;                                // labellings of the launch: 32 (W - 1) + (bits of the last word)
    uint32_t* counts;                          // [D][W][G][32]: the ones, then (scan) the ones before the workgroup
    float* one; float* zero;                   // [D nq x pitch1], [D nq x pitch0]
    int64_t pitch1, pitch0, n1, n0;            // n1 ones and n0 = N - n1 zeros per labelling
};

// The front half of count and split: the workgroup's place, this lane's 8 label words (0 past N) and, in wcnt[v][b], the ones of
// labelling b in wave v.  Ends behind a barrier.
struct Place { int64_t dl, w, g, r0; };                     // direction, word, workgroup of the segment, this wave's first rank
__device__ __forceinline__ Place front(const Args& a, uint32_t (&word)[kRows], unsigned int (*wcnt)[32]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Place p;
    p.g = blockIdx.x % a.G;
    const int64_t t = blockIdx.x / a.G;
    p.w = t % a.W; p.dl = t / a.W;
    p.r0 = p.g * kShare + wave * kWaveShare;
    const uint32_t* idx = a.idx + p.dl * a.kpitch;
    const uint32_t* cw = a.cols + p.w * a.cpitch;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int64_t r = p.r0 + k * 64 + lane;
        uint32_t v = 0u;
        if (r < a.N) {
            const uint32_t row = idx[r];
            if (row < a.N) v = cw[row];                                               // always true; keeps a wrong index inside the column
        }
        word[k] = v;
    }
    unsigned int mine = 0;
    for (int b = 0; b < 32; ++b) {
        unsigned int c = 0;
#pragma unroll
        for (int k = 0; k < kRows; ++k) c += (unsigned int)__popcll(__ballot((word[k] >> b) & 1u));
        if (lane == b) mine = c;
    }
    if (lane < 32) wcnt[wave][lane] = mine;
    __syncthreads();
    return p;
}

__global__ void __launch_bounds__(kThreads) count_kernel(Args a) {
    __shared__ unsigned int wcnt[kWaves][32];
    uint32_t word[kRows];
    const Place p = front(a, word, wcnt);
    if (threadIdx.x < 32) {
        unsigned int s = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) s += wcnt[v][threadIdx.x];
        a.counts[((p.dl * a.W + p.w) * a.G + p.g) * 32 + threadIdx.x] = s;
    }
}

// one thread per (direction, word, labelling bit): exclusive prefixes over the workgroups of the segment, in workgroup order
__global__ void __launch_bounds__(kThreads) scan_kernel(Args a) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= a.D * a.W * 32) return;
    uint32_t* c = a.counts + (t / 32) * a.G * 32 + (t % 32);
    unsigned int run = 0;
    for (int64_t g = 0; g < a.G; ++g) {
        const unsigned int v = c[g * 32];
        c[g * 32] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(kThreads) split_kernel(Args a) {
    __shared__ unsigned int wcnt[kWaves][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t word[kRows];
    const Place p = front(a, word, wcnt);
    float key[kRows];
    const float* keys = a.keys + p.dl * a.kpitch;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int64_t r = p.r0 + k * 64 + lane;
        key[k] = r < a.N ? keys[r] : 0.f;
    }
    const uint32_t* before = a.counts + ((p.dl * a.W + p.w) * a.G + p.g) * 32;
    const int64_t left = a.nq - 32 * p.w;                                             // labellings from this word on
    const int nbits = left < 32 ? (int)left : 32;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int b = 0; b < nbits; ++b) {
        int64_t ones = before[b];                                                     // ones before this wave's first rank
        for (int v = 0; v < wave; ++v) ones += wcnt[v][b];
        const int64_t pair = p.dl * a.nq + 32 * p.w + b;
        float* one = a.one + pair * a.pitch1;
        float* zero = a.zero + pair * a.pitch0;
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int64_t r = p.r0 + k * 64 + lane;
            const bool bit = (word[k] >> b) & 1u;
            const unsigned long long has = __ballot(bit);
            const int64_t at1 = ones + __popcll(has & below);
            if (r < a.N) {
                if (bit) {
                    if (at1 < a.n1) one[at1] = key[k];                                // always true; keeps a wrong count inside the pair
                } else {
                    const int64_t at0 = r - at1;
                    if (at0 < a.n0) zero[at0] = key[k];                               // always true, as above
                }
            }
            ones += __popcll(has);
        }
    }
}

// count, scan, split of one launch's (directions x words), enqueued on `st`
inline hipError_t split_segments(const Args& a, hipStream_t st) {
    if (a.D < 1 || a.W < 1 || a.N < 1) return hipSuccess;
    const unsigned int grid = (unsigned int)(a.D * a.W * a.G);
    count_kernel<<<grid, kThreads, 0, st>>>(a);
    scan_kernel<<<(unsigned int)((a.D * a.W * 32 + kThreads - 1) / kThreads), kThreads, 0, st>>>(a);
    split_kernel<<<grid, kThreads, 0, st>>>(a);
    return hipGetLastError();
}
#endif

}  // namespace ssplit
}  // namespace fad
