// The segmented key sort of the sliced Wasserstein distance (fad_sliced_wasserstein): `segs` segments of n float32 keys
// each, every segment sorted ascending on its own.  Keys only here; sliced_sort_pairs.h runs the same passes with a uint32 payload.
//
// An LSD radix sort with 8-bit digits: kPasses = 4 passes, each of three launches, between two buffers (the result ends where it began).
//   - map:     a float goes through the order-preserving map to uint32 (all bits of a negative flipped, the sign bit of the rest set),
//              so -0 sorts before +0 and the unsigned order of the images is the order of the floats.  The first pass maps as it reads,
//              the last one maps back as it writes: the buffers in between hold images.
//   - share:   a workgroup owns kShare = 2048 consecutive keys of one segment, taken in rounds of 256 (a key per thread).  A segment of
//              n keys takes W = ceil(n / kShare) workgroups; where one round holds a whole segment (n <= 256) a workgroup owns up to
//              kMaxSegs = 8 consecutive segments instead, one after the other, so that it still moves up to 2048 keys.
//   - count:   per (segment, workgroup) a 256-bin histogram of the pass's digit, in LDS with integer atomics, stored whole.
//   - scan:    per segment, thread d walks the W counts of digit d in workgroup order into exclusive prefixes, and the 256 digit totals
//              are scanned in LDS into the digit bases.
//   - scatter: a workgroup walks its share again in the same rounds.  A key's place is  base[d] + prefix[workgroup][d] + keys of digit
//              d in earlier rounds + in earlier waves of this round + in lower lanes of this wave: the last from 8 wave ballots (64 bits
//              wide), the others from LDS counts written by one lane per (wave, digit).  The place is a function of the key's index
//              alone: the sort is stable, nothing is placed by order of arrival, the output does not depend on timing.
// Every pass runs whatever the keys are: all-equal, sorted, reversed and two-valued inputs cost the same.  n >= 1.
//
// The scatter body and the pass loop exist once, below, for both forms.
//
// Scratch: counts_elems(n, segs) uint32 of counts and 256 per segment of bases.  Nothing here is a template of the callers' dtype: the
// header stands alone (tests/native/sliced_sort_check.hip includes only it).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace fad {
namespace ssort {

constexpr int kThreads = 256;                  // a round: one key per thread
constexpr int kRounds = 8;
constexpr int kShare = kThreads * kRounds;     // keys of a segment per workgroup
constexpr int kRadix = 256;
constexpr int kPasses = 4;
constexpr int kMaxSegs = 8;                    // segments per workgroup at most

__host__ __device__ inline uint32_t key_image(uint32_t float_bits) {
    return float_bits ^ ((float_bits >> 31) ? 0xffffffffu : 0x80000000u);
}
__host__ __device__ inline uint32_t key_bits(uint32_t image) {
    return image ^ ((image >> 31) ? 0x80000000u : 0xffffffffu);
}

// how `segs` segments of n keys are shared out: W workgroups per segment, G segments per workgroup (one of the two is 1)
struct Plan { int64_t n, segs, W, G, groups; };            // groups = ceil(segs / G); a launch has groups * W workgroups
inline Plan plan(int64_t n, int64_t segs) {
    Plan p;
    p.n = n; p.segs = segs;
    p.W = (n + kShare - 1) / kShare;
    p.G = n <= kThreads ? (segs < kMaxSegs ? segs : kMaxSegs) : 1;
    p.groups = (segs + p.G - 1) / p.G;
    return p;
}
inline int64_t counts_elems(int64_t n, int64_t segs) { return segs * ((n + kShare - 1) / kShare) * kRadix; }
inline int64_t bases_elems(int64_t segs) { return segs * kRadix; }

#if defined(__HIPCC__)
struct Args {
    const uint32_t* in; uint32_t* out;         // [segs x pitch]
    int64_t pitch, n, segs, W, G;
    int shift;
    uint32_t* counts;                          // [segs][W][256]: the histogram, then (scan) the exclusive prefix over workgroups
    uint32_t* bases;                           // [segs][256]: where digit d of the segment starts
};

template <bool FIRST>
__global__ void __launch_bounds__(kThreads) count_kernel(Args a) {
    __shared__ unsigned int hist[kRadix];
    const int tid = threadIdx.x;
    const int64_t wg = blockIdx.x % a.W, s0 = (blockIdx.x / a.W) * a.G;
    for (int64_t s = s0; s < s0 + a.G && s < a.segs; ++s) {                           // uniform over the workgroup
        hist[tid] = 0;
        __syncthreads();
        const uint32_t* src = a.in + s * a.pitch;
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int64_t i = wg * kShare + r * kThreads + tid;
            if (i < a.n) {
                uint32_t k = src[i];
                if (FIRST) k = key_image(k);
                atomicAdd(&hist[(k >> a.shift) & 0xffu], 1u);                         // integer counts: order does not matter
            }
        }
        __syncthreads();
        a.counts[(s * a.W + wg) * kRadix + tid] = hist[tid];
        __syncthreads();
    }
}

// one workgroup per segment
__global__ void __launch_bounds__(kRadix) scan_kernel(Args a) {
    __shared__ unsigned int tot[kRadix];
    const int d = threadIdx.x;
    uint32_t* c = a.counts + (int64_t)blockIdx.x * a.W * kRadix;
    unsigned int run = 0;
    for (int64_t w = 0; w < a.W; ++w) {
        const unsigned int v = c[w * kRadix + d];
        c[w * kRadix + d] = run;
        run += v;
    }
    tot[d] = run;
    __syncthreads();
    for (int off = 1; off < kRadix; off <<= 1) {                                      // inclusive scan over the digits
        const unsigned int v = d >= off ? tot[d - off] : 0u;
        __syncthreads();
        tot[d] += v;
        __syncthreads();
    }
    a.bases[(int64_t)blockIdx.x * kRadix + d] = tot[d] - run;
}

// The scatter of one workgroup.  With PAIRS every key carries a uint32 payload, the position it had in its segment before the sort
// (sliced_sort_pairs.h): stored at the key's place of a second buffer, idx_out; on the first pass it is the key's own position, later
// passes read it beside the key from idx_in.  Without PAIRS the two pointers are never touched.
template <bool FIRST, bool LAST, bool PAIRS>
__device__ __forceinline__ void scatter_body(const Args& a, const uint32_t* idx_in, uint32_t* idx_out) {
    __shared__ unsigned int place[kRadix];                 // where the next key of digit d of this workgroup goes
    __shared__ unsigned int wcnt[kThreads / 64][kRadix];   // this round's keys of digit d in wave w
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t wg = blockIdx.x % a.W, s0 = (blockIdx.x / a.W) * a.G;
    for (int64_t s = s0; s < s0 + a.G && s < a.segs; ++s) {                           // uniform over the workgroup
        __syncthreads();
        place[tid] = a.bases[s * kRadix + tid] + a.counts[(s * a.W + wg) * kRadix + tid];
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) wcnt[w][tid] = 0;
        __syncthreads();
        const uint32_t* src = a.in + s * a.pitch;
        uint32_t* dst = a.out + s * a.pitch;
        const uint32_t* isrc = PAIRS ? idx_in + s * a.pitch : nullptr;
        uint32_t* idst = PAIRS ? idx_out + s * a.pitch : nullptr;
        for (int r = 0; r < kRounds; ++r) {
            const int64_t i0 = wg * kShare + r * kThreads;
            if (i0 >= a.n) break;                                                     // uniform over the workgroup
            const bool live = i0 + tid < a.n;
            uint32_t k = live ? src[i0 + tid] : 0u;
            uint32_t row = 0u;
            if (PAIRS) row = FIRST ? (uint32_t)(i0 + tid) : (live ? isrc[i0 + tid] : 0u);
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
                    if (PAIRS) idst[at] = row;
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

template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kThreads) scatter_kernel(Args a) {
    scatter_body<FIRST, LAST, false>(a, nullptr, nullptr);
}

// The kPasses passes over `segs` segments of n keys at keys + s * pitch, between keys and tmp: count, scan, then the pass's scatter --
// scatter(pass, grid, first, last) launches it, first and last as std::bool_constant, after a.in, a.out and a.shift are set for the
// pass.  Enqueued on `st`; the first error of a launch is returned.
template <class Scatter>
inline hipError_t sort_passes(Args& a, float* keys, float* tmp, int64_t pitch, int64_t n, int64_t segs, uint32_t* counts, uint32_t* bases,
                              hipStream_t st, Scatter scatter) {
    if (n < 1 || segs < 1) return hipSuccess;
    const Plan p = plan(n, segs);
    a.pitch = pitch; a.n = n; a.segs = segs; a.W = p.W; a.G = p.G; a.counts = counts; a.bases = bases;
    const unsigned int grid = (unsigned int)(p.groups * p.W);
    uint32_t* buf[2] = {reinterpret_cast<uint32_t*>(keys), reinterpret_cast<uint32_t*>(tmp)};
    for (int pass = 0; pass < kPasses; ++pass) {
        a.in = buf[pass & 1]; a.out = buf[(pass & 1) ^ 1]; a.shift = 8 * pass;
        if (pass == 0) count_kernel<true><<<grid, kThreads, 0, st>>>(a);
        else count_kernel<false><<<grid, kThreads, 0, st>>>(a);
        scan_kernel<<<(unsigned int)segs, kRadix, 0, st>>>(a);
        if (pass == 0) scatter(pass, grid, std::true_type{}, std::false_type{});
        else if (pass == kPasses - 1) scatter(pass, grid, std::false_type{}, std::true_type{});
        else scatter(pass, grid, std::false_type{}, std::false_type{});
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// `segs` segments of n float32 keys at keys + s * pitch, sorted ascending in place; `tmp` is a second buffer of the same shape, `counts`
// and `bases` hold counts_elems(n, segs) and bases_elems(segs) uint32.
inline hipError_t sort_segments(float* keys, float* tmp, int64_t pitch, int64_t n, int64_t segs, uint32_t* counts, uint32_t* bases,
                                hipStream_t st) {
    Args a{};
    return sort_passes(a, keys, tmp, pitch, n, segs, counts, bases, st, [&](int, unsigned int grid, auto first, auto last) {
        scatter_kernel<decltype(first)::value, decltype(last)::value><<<grid, kThreads, 0, st>>>(a);
    });
}
#endif

}  // namespace ssort
}  // namespace fad
