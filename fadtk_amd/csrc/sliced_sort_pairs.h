// The key-index form of sliced_sort.h's segmented sort (fad_sliced_shares): every key carries a uint32 payload, the
// position it had in its segment before the sort, so that after the sort idx[r] is the row whose projection stands at rank r.
//
// The passes, the shares, count_kernel and scan_kernel are sliced_sort.h's, as they are: they read keys only.  The scatter here computes
// a key's place exactly as scatter_kernel does -- base[d] + prefix[workgroup][d] + keys of digit d in earlier rounds, earlier waves and
// lower lanes -- and stores the payload at the same place of a second index buffer.  On the first pass the payload is the key's own
// position (no buffer of 0 .. n - 1 is ever written or read); later passes read it beside the key.  The place is a function of the
// key's position alone, so the sort is stable: equal keys (equal float bits; -0 sorts before +0) keep their rows in ascending order, and
// nothing is placed by order of arrival.  Both index buffers have the keys' shape and pitch; like the keys, the result ends where it
// began (idx), and idx need not be initialised.  n >= 1, n < 2^32.
//
// Scratch: as sort_segments.  This header stands on sliced_sort.h alone (tests/native/sliced_sort_pairs_check.hip includes only it).
#pragma once

#include "sliced_sort.h"

namespace fad {
namespace ssort {

#if defined(__HIPCC__)
struct PairArgs {
    Args k;                                    // the keys' side: what count_kernel and scan_kernel take
    const uint32_t* idx_in; uint32_t* idx_out; // [segs x pitch], beside k.in and k.out (idx_in is not read on the first pass)
};

template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kThreads) scatter_pairs_kernel(PairArgs p) {
    __shared__ unsigned int place[kRadix];                 // where the next key of digit d of this workgroup goes
    __shared__ unsigned int wcnt[kThreads / 64][kRadix];   // this round's keys of digit d in wave w
    const Args& a = p.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t wg = blockIdx.x % a.W, s0 = (blockIdx.x / a.W) * a.G;
    for (int64_t s = s0; s < s0 + a.G && s < a.segs; ++s) {                           // uniform over the workgroup
        __syncthreads();
        place[tid] = a.bases[s * kRadix + tid] + a.counts[(s * a.W + wg) * kRadix + tid];
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) wcnt[w][tid] = 0;
        __syncthreads();
        const uint32_t* src = a.in + s * a.pitch;
        const uint32_t* isrc = p.idx_in + s * a.pitch;
        uint32_t* dst = a.out + s * a.pitch;
        uint32_t* idst = p.idx_out + s * a.pitch;
        for (int r = 0; r < kRounds; ++r) {
            const int64_t i0 = wg * kShare + r * kThreads;
            if (i0 >= a.n) break;                                                     // uniform over the workgroup
            const bool live = i0 + tid < a.n;
            uint32_t k = live ? src[i0 + tid] : 0u;
            const uint32_t row = FIRST ? (uint32_t)(i0 + tid) : (live ? isrc[i0 + tid] : 0u);
            if (FIRST) k = key_image(k);
            const unsigned int d = (k >> a.shift) & 0xffu;
            unsigned long long peers = __ballot(live);     // the live lanes of the wave with this lane's digit
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const unsigned long long has = __ballot(live && bit);
                peers &= bit ? has : ~has;
            }
            const unsigned int below = (unsigned int)__popcll(peers & ((1ull << lane) - 1ull));
            if (live && below == 0) wcnt[wave][d] = (unsigned int)__popcll(peers);
            __syncthreads();
            if (live) {
                unsigned int at = place[d] + below;
                for (int w = 0; w < wave; ++w) at += wcnt[w][d];
                if (at < a.n) {                                                       // always true; keeps a wrong count inside the segment
                    dst[at] = LAST ? key_bits(k) : k;
                    idst[at] = row;
                }
            }
            __syncthreads();
            unsigned int add = 0;
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) { add += wcnt[w][tid]; wcnt[w][tid] = 0; }
            place[tid] += add;
            __syncthreads();
        }
    }
}

// sort_segments with a payload: `segs` segments of n float32 keys at keys + s * pitch sorted ascending in place, and idx + s * pitch
// filled with the positions 0 .. n - 1 of the segment in the sorted order (equal keys: ascending).  `tmp` and `idx_tmp` are second
// buffers of the same shape; counts and bases as sort_segments.  Enqueued on `st`; the first error of a launch is returned.
inline hipError_t sort_segment_pairs(float* keys, float* tmp, uint32_t* idx, uint32_t* idx_tmp, int64_t pitch, int64_t n, int64_t segs,
                                     uint32_t* counts, uint32_t* bases, hipStream_t st) {
    if (n < 1 || segs < 1) return hipSuccess;
    const Plan pl = plan(n, segs);
    PairArgs p{};
    Args& a = p.k;
    a.pitch = pitch; a.n = n; a.segs = segs; a.W = pl.W; a.G = pl.G; a.counts = counts; a.bases = bases;
    const unsigned int grid = (unsigned int)(pl.groups * pl.W);
    uint32_t* buf[2] = {reinterpret_cast<uint32_t*>(keys), reinterpret_cast<uint32_t*>(tmp)};
    uint32_t* ibuf[2] = {idx, idx_tmp};
    for (int pass = 0; pass < kPasses; ++pass) {
        a.in = buf[pass & 1]; a.out = buf[(pass & 1) ^ 1]; a.shift = 8 * pass;
        p.idx_in = ibuf[pass & 1]; p.idx_out = ibuf[(pass & 1) ^ 1];
        if (pass == 0) count_kernel<true><<<grid, kThreads, 0, st>>>(a);
        else count_kernel<false><<<grid, kThreads, 0, st>>>(a);
        scan_kernel<<<(unsigned int)segs, kRadix, 0, st>>>(a);
        if (pass == 0) scatter_pairs_kernel<true, false><<<grid, kThreads, 0, st>>>(p);
        else if (pass == kPasses - 1) scatter_pairs_kernel<false, true><<<grid, kThreads, 0, st>>>(p);
        else scatter_pairs_kernel<false, false><<<grid, kThreads, 0, st>>>(p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
#endif

}  // namespace ssort
}  // namespace fad
