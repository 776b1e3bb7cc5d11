// The key-index form of sliced_sort.h's segmented sort (fad_sliced_shares): every key carries a uint32 payload, the
// position it had in its segment before the sort, so that after the sort idx[r] is the row whose projection stands at rank r.
//
// Everything but the kernel arguments is sliced_sort.h's: the passes, the shares, count_kernel, scan_kernel and the scatter body, here
// with PAIRS, which stores the payload at the key's place of a second index buffer.  No buffer of 0 .. n - 1 is ever written or read.
// The place is a function of the key's position alone, so the sort is stable: equal keys (equal float bits; -0 sorts before +0) keep
// their rows in ascending order.  Both index buffers have the keys' shape and pitch; like the keys, the result ends where it began
// (idx), and idx need not be initialised.  n >= 1, n < 2^32.
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
    scatter_body<FIRST, LAST, true>(p.k, p.idx_in, p.idx_out);
}

// sort_segments with a payload: `segs` segments of n float32 keys at keys + s * pitch sorted ascending in place, and idx + s * pitch
// filled with the positions 0 .. n - 1 of the segment in the sorted order (equal keys: ascending).  `tmp` and `idx_tmp` are second
// buffers of the same shape; counts and bases as sort_segments.
inline hipError_t sort_segment_pairs(float* keys, float* tmp, uint32_t* idx, uint32_t* idx_tmp, int64_t pitch, int64_t n, int64_t segs,
                                     uint32_t* counts, uint32_t* bases, hipStream_t st) {
    PairArgs p{};
    uint32_t* ibuf[2] = {idx, idx_tmp};
    return sort_passes(p.k, keys, tmp, pitch, n, segs, counts, bases, st, [&](int pass, unsigned int grid, auto first, auto last) {
        p.idx_in = ibuf[pass & 1]; p.idx_out = ibuf[(pass & 1) ^ 1];
        scatter_pairs_kernel<decltype(first)::value, decltype(last)::value><<<grid, kThreads, 0, st>>>(p);
    });
}
#endif

}  // namespace ssort
}  // namespace fad
