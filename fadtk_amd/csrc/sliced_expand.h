// The stable expansion of the sliced Wasserstein bootstrap (fad_sliced_bootstrap): one sorted segment of N float32 keys
// per direction, the row at every rank beside it, and per row a word of kPerWord = 4 byte counts (byte b = replicate 4 w + b: how often
// the resample takes the row, 0 .. 255).  For every (direction, replicate) pair the keys go, in rank order, to the pair's buffer, the
// key at rank r written c(r) times from E(r) on, E the exclusive prefix sum of the counts over the lower ranks: the sorted projections
// of np.repeat(rows, counts), with no sort and no gather of rows.
//
//   - share:   a workgroup owns kShare = 2048 consecutive ranks of one (direction, replicate word), as the split's and the sort's
//              workgroups do; wave v owns the ranks [512 v, 512 v + 512) of them, read as 8 coalesced rows of 64.  A lane keeps its 8
//              keys and its 8 count words (one gathered word per rank serves 4 replicates) in registers.
//   - count:   per (direction, word, workgroup) the sum of the counts of each of the 4 replicates: a lane's 8 words summed in two
//              packed halves (bytes 0 and 2, bytes 1 and 3, 16 bits each: at most 8 x 255), unpacked, four wave sums by shuffles, the
//              four waves summed through LDS.  Stored whole: counts [D][W][G][4].
//   - scan:    one thread per (direction, word, replicate) walks the G workgroups in order into exclusive prefixes.  Integers.
//   - expand:  the count's front half again, then per row of 64 ranks an inclusive scan over the lanes of the packed halves (a field
//              holds at most 64 x 255 = 16 320 < 2^16, so the two replicates of a half never meet), and the key at rank r goes to
//                  E(r) = prefix[workgroup][b] + counts in earlier waves + counts in this wave's earlier rows + counts in lower lanes
//              and the c(r) - 1 places behind it.  The place of every copy is a function of the rank alone: nothing is placed by order
//              of arrival, no atomic is used, the output does not depend on timing.
// Replicates past the last one (fewer than 4 in the last word) are skipped.  Every store carries an index guard (at < the pair's total)
// that is always true when total[q] is the sum of replicate q's counts: a wrong count cannot write outside its pair's buffer.
//
// Pairs are numbered direction-major within a launch: pair (dl, q) = dl * nq + q, q the replicate's index within the launch's words
// (0 .. nq - 1, nq = the launch's replicates), its buffer at out[pair * pitch], pitch >= every total.
//
// This header stands alone (tests/native/sliced_expand_check.hip includes only it).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fad {
namespace sexpand {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 8;                                   // rows of 64 ranks per wave
constexpr int kWaveShare = 64 * kRows;                     // ranks per wave
constexpr int kShare = kWaves * kWaveShare;                // ranks of a segment per workgroup: the sort's 2048
constexpr int kPerWord = 4;                                // replicates per gathered count word: one byte each
constexpr uint32_t kHalf = 0x00ff00ffu;                    // bytes 0 and 2 of a word, as two 16-bit fields

inline int64_t groups(int64_t N) { return (N + kShare - 1) / kShare; }
inline int64_t words(int64_t replicates) { return (replicates + kPerWord - 1) / kPerWord; }
// uint32 of counts for D directions x W words
inline int64_t counts_elems(int64_t N, int64_t D, int64_t W) { return D * W * groups(N) * kPerWord; }

#if defined(__HIPCC__)
struct Args {
    const float* keys; const uint32_t* idx;    // [D x kpitch]: the sorted keys and the row at every rank
    int64_t kpitch, N;
    const uint32_t* cols;                      // [W x cpitch]: the count words of the launch's W replicate words, per row
    int64_t cpitch;
    int64_t D, W, G;                           // directions, words, workgroups per segment: the grid is D * W * G
    int64_t nq;                                // replicates of the launch: 4 (W - 1) + (replicates of the last word)
    uint32_t* counts;                          // [D][W][G][4]: the sums of counts, then (scan) the sum before the workgroup
    float* out; int64_t pitch;                 // [D nq x pitch]
    const int32_t* total;                      // [nq]: the sum of every replicate's counts over the N rows
};

// The front half of count and expand: the workgroup's place, this lane's 8 count words (0 past N) and, in wcnt[v][b], the sum of the
// counts of replicate b in wave v.  Ends behind a barrier.
struct Place { int64_t dl, w, g, r0; };                     // direction, word, workgroup of the segment, this wave's first rank
__device__ __forceinline__ Place front(const Args& a, uint32_t (&word)[kRows], unsigned int (*wcnt)[kPerWord]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Place p;
    p.g = blockIdx.x % a.G;
    const int64_t t = blockIdx.x / a.G;
    p.w = t % a.W; p.dl = t / a.W;
    p.r0 = p.g * kShare + wave * kWaveShare;
    const uint32_t* idx = a.idx + p.dl * a.kpitch;
    const uint32_t* cw = a.cols + p.w * a.cpitch;
    uint32_t even = 0u, odd = 0u;                                                     // bytes 0, 2 and bytes 1, 3 over the lane's 8 ranks
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int64_t r = p.r0 + k * 64 + lane;
        uint32_t v = 0u;
        if (r < a.N) {
            const uint32_t row = idx[r];
            if (row < a.N) v = cw[row];                                               // always true; keeps a wrong index inside the column
        }
        word[k] = v;
        even += v & kHalf;
        odd += (v >> 8) & kHalf;
    }
    unsigned int s[kPerWord] = {even & 0xffffu, odd & 0xffffu, even >> 16, odd >> 16};
#pragma unroll
    for (int b = 0; b < kPerWord; ++b) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[b] += __shfl_xor(s[b], off, 64);
        if (lane == b) wcnt[wave][b] = s[b];
    }
    __syncthreads();
    return p;
}

__global__ void __launch_bounds__(kThreads) count_kernel(Args a) {
    __shared__ unsigned int wcnt[kWaves][kPerWord];
    uint32_t word[kRows];
    const Place p = front(a, word, wcnt);
    if (threadIdx.x < kPerWord) {
        unsigned int s = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) s += wcnt[v][threadIdx.x];
        a.counts[((p.dl * a.W + p.w) * a.G + p.g) * kPerWord + threadIdx.x] = s;
    }
}

// one thread per (direction, word, replicate byte): exclusive prefixes over the workgroups of the segment, in workgroup order
__global__ void __launch_bounds__(kThreads) scan_kernel(Args a) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= a.D * a.W * kPerWord) return;
    uint32_t* c = a.counts + (t / kPerWord) * a.G * kPerWord + (t % kPerWord);
    unsigned int run = 0;
    for (int64_t g = 0; g < a.G; ++g) {
        const unsigned int v = c[g * kPerWord];
        c[g * kPerWord] = run;
        run += v;
    }
}

// c copies of `key` from place `at` on in the pair's buffer
__device__ __forceinline__ void put(float* out, int64_t at, uint32_t c, int64_t total, float key) {
    for (uint32_t j = 0; j < c; ++j)
        if (at + j < total) out[at + j] = key;                                        // always true; keeps a wrong count inside the pair
}

__global__ void __launch_bounds__(kThreads) expand_kernel(Args a) {
    __shared__ unsigned int wcnt[kWaves][kPerWord];
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
    const uint32_t* before = a.counts + ((p.dl * a.W + p.w) * a.G + p.g) * kPerWord;
    const int64_t left = a.nq - kPerWord * p.w;                                       // replicates from this word on
    const int nrep = left < kPerWord ? (int)left : kPerWord;
    for (int h = 0; h < 2 && h < nrep; ++h) {                                         // replicates h and h + 2 share one packed scan
        const bool two = h + 2 < nrep;
        const int64_t q0 = kPerWord * p.w + h, q1 = two ? q0 + 2 : q0;
        int64_t e0 = before[h], e1 = before[h + 2];                                   // counts before this wave's first rank
        for (int v = 0; v < wave; ++v) { e0 += wcnt[v][h]; e1 += wcnt[v][h + 2]; }
        float* out0 = a.out + (p.dl * a.nq + q0) * a.pitch;
        float* out1 = a.out + (p.dl * a.nq + q1) * a.pitch;
        const int64_t total0 = a.total[q0], total1 = a.total[q1];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int64_t r = p.r0 + k * 64 + lane;
            const uint32_t mine = (word[k] >> (8 * h)) & kHalf;
            uint32_t inc = mine;                                                      // inclusive scan over the lanes, both fields at once
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_up(inc, off, 64);
                if (lane >= off) inc += up;
            }
            const uint32_t all = __shfl(inc, 63, 64), exc = inc - mine;
            if (r < a.N) {
                put(out0, e0 + (exc & 0xffffu), mine & 0xffffu, total0, key[k]);
                if (two) put(out1, e1 + (exc >> 16), mine >> 16, total1, key[k]);
            }
            e0 += all & 0xffffu;
            e1 += all >> 16;
        }
    }
}

// count, scan, expand of one launch's (directions x words), enqueued on `st`
inline hipError_t expand_segments(const Args& a, hipStream_t st) {
    if (a.D < 1 || a.W < 1 || a.N < 1) return hipSuccess;
    const unsigned int grid = (unsigned int)(a.D * a.W * a.G);
    count_kernel<<<grid, kThreads, 0, st>>>(a);
    scan_kernel<<<(unsigned int)((a.D * a.W * kPerWord + kThreads - 1) / kThreads), kThreads, 0, st>>>(a);
    expand_kernel<<<grid, kThreads, 0, st>>>(a);
    return hipGetLastError();
}
#endif

}  // namespace sexpand
}  // namespace fad
