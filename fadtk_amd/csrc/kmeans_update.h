// The glue of Lloyd's k-means around the fused nearest-row pass (fad_kmeans): the centroid operand, the deterministic
// centroid update, the stop rule's count and the inertia.  The assignment itself is kad.hip's nearest_cross_kernel, unchanged.
//
// Centroid operand.  A centroid is float32; the main loop of 16-bit rows multiplies 16-bit values.  write_planes splits c into P values
// of the rows' dtype that add up to c (float16: hi + lo, P = 2, which carries 11 + 11 bits and a sign: c to 2^-22; bfloat16: three,
// P = 3, exact; float32: itself, P = 1) and stores plane p at depth offset p * dp of the centroid's image row: a depth concatenation.
// The rows' image holds every row P times side by side (replicate_kernel), so the unchanged k loop of P * nchunks steps adds
// x . hi + x . lo (+ x . lo2) into one float32 accumulator chain.  h_c = -|c|^2 / 2 comes from the float32 values, in
// kad_pack_kernel's order.  float16 rows and their centroids are scaled by a power of two first (f16_scale).
//
// Update.  Labels are sorted with their row numbers by the stable key-index sort (sliced_sort_pairs.h; a label < 2^16 as a float32 bit
// pattern is a positive subnormal, so the keys order as the integers), which leaves every cluster's rows as one ascending run.  A run is
// cut into chunks of kChunkRows rows.  chunk_sum_kernel: one thread per (chunk, column) adds the chunk's rows in float64 in ascending
// row order.  centroid_finish_kernel: one wave per cluster adds the cluster's chunk partials in ascending order, divides by the count,
// rounds to float32 and writes the centroid, its planes and h.  An empty cluster is not touched.  No floating-point atomics: the counts
// are integers, and every sum has one fixed order that depends on the labels alone.
//
// This header stands on sliced_sort_pairs.h alone (tests/native/kmeans_update_check.hip includes only it).
#pragma once

#include "sliced_sort_pairs.h"

#include <cmath>
#include <cstdint>

namespace fad {
namespace kmeans {

constexpr int kChunkRows = 64;                 // rows of one cluster per partial sum
constexpr int kColBlock = 128;                 // columns per workgroup of chunk_sum_kernel
constexpr int kMaxClusters = 65536;
constexpr int kMaxSets = 8;

// planes of the rows' dtype that carry a float32 value exactly: element size 2 with an 11-bit significand (float16) -> 2,
// with an 8-bit one (bfloat16) -> 3, float32 -> 1
template <typename T> struct Planes { static constexpr int value = 1; };
template <> struct Planes<_Float16> { static constexpr int value = 2; };
template <> struct Planes<__bf16> { static constexpr int value = 3; };

// float16 rows are scaled by a power of two g before they meet the centroid planes, so that the low plane of a centroid never falls
// into float16's subnormal range whatever the scale of the data: g brings the largest row magnitude (max_bits: its float16 bit pattern
// without the sign) into [2^10, 2^11), which leaves a centroid entry 32x the headroom of the largest row entry.  Rows are never scaled
// down (that could round them): g = 1 from 2^10 on, and for rows that are all zero.  Scaling rows and centroids by a power of two then
// gives the same operands, so the same labels.
inline float f16_scale(unsigned int max_bits) {
    if (max_bits == 0) return 1.f;
    int e;
    if (max_bits >> 10) {
        e = (int)(max_bits >> 10) - 15;
    } else {
        e = -25;
        for (unsigned int b = max_bits; b; b >>= 1) ++e;
    }
    return e < 10 ? ldexpf(1.f, 10 - e) : 1.f;
}

// chunks of all clusters at most: every cluster's last chunk may be part-filled
inline int64_t chunks_bound(int64_t n, int64_t k) { return n / kChunkRows + k; }

// the sort's scratch beside keys / tmp / idx / idx_tmp [n] each
inline int64_t sort_counts_elems(int64_t n) { return ssort::counts_elems(n, 1); }

#if defined(__HIPCC__)
// keys[i] = labels[i] as the sort's key, counts[label] += 1 (integer atomics: the order does not matter).  counts is zero on entry.
__global__ void __launch_bounds__(256) label_count_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t k, uint32_t* __restrict__ keys,
                                                          uint32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = (uint32_t)labels[i];
    keys[i] = l;
    if ((int64_t)l < k) atomicAdd(&counts[l], 1u);
}

// One workgroup: starts[c] = rows of the clusters before c, chunk0[c] = their chunks (both k + 1 entries, exclusive prefixes in cluster
// order); stats[0] = the most chunks one cluster takes, stats[1] = the clusters without a row.
__global__ void __launch_bounds__(256) cluster_scan_kernel(const uint32_t* __restrict__ counts, int64_t k, uint32_t* __restrict__ starts,
                                                           uint32_t* __restrict__ chunk0, uint32_t* __restrict__ stats) {
    __shared__ unsigned int srow[256], schunk[256], smax[256], sempty[256];
    const int tid = threadIdx.x;
    const int64_t per = (k + 255) / 256, b = tid * per, e = b + per < k ? b + per : k;
    unsigned int rows = 0, chunks = 0, most = 0, empty = 0;
    for (int64_t c = b; c < e; ++c) {
        const unsigned int n = counts[c], ch = (n + kChunkRows - 1) / kChunkRows;
        rows += n; chunks += ch;
        most = ch > most ? ch : most;
        empty += n == 0;
    }
    srow[tid] = rows; schunk[tid] = chunks; smax[tid] = most; sempty[tid] = empty;
    __syncthreads();
    if (tid == 0) {                                                                   // 256 entries: a serial scan costs nothing
        unsigned int r = 0, c = 0, m = 0, z = 0;
        for (int t = 0; t < 256; ++t) {
            const unsigned int pr = srow[t], pc = schunk[t];
            srow[t] = r; schunk[t] = c;
            r += pr; c += pc;
            m = smax[t] > m ? smax[t] : m;
            z += sempty[t];
        }
        starts[k] = r; chunk0[k] = c;
        stats[0] = m; stats[1] = z;
    }
    __syncthreads();
    rows = srow[tid]; chunks = schunk[tid];
    for (int64_t c = b; c < e; ++c) {
        starts[c] = rows; chunk0[c] = chunks;
        const unsigned int n = counts[c];
        rows += n; chunks += (n + kChunkRows - 1) / kChunkRows;
    }
}

// partial[chunk * d + col] = the chunk's rows of column col summed in float64, in ascending row order.  blockIdx.x: the chunk (the grid
// covers chunks_bound; chunks past chunk0[k] do nothing), blockIdx.y: the column block.  img: the rows' image, `pitch` elements a row;
// idx: the rows of every cluster as one ascending run (the sort's payload), n rows in all.
template <typename T>
__global__ void __launch_bounds__(kColBlock) chunk_sum_kernel(const T* __restrict__ img, int64_t pitch, int64_t n, const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ starts, const uint32_t* __restrict__ chunk0, int64_t k,
                                                              int64_t d, double* __restrict__ partial) {
    const uint32_t c = blockIdx.x;
    if (c >= chunk0[k]) return;                                                       // uniform over the workgroup
    int64_t lo = 0, hi = k;                                                           // the cluster: the last one with chunk0[cl] <= c
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t cl = lo;
    const int64_t r0 = (int64_t)starts[cl] + (int64_t)(c - chunk0[cl]) * kChunkRows;
    int64_t r1 = r0 + kChunkRows;
    if (r1 > (int64_t)starts[cl + 1]) r1 = starts[cl + 1];
    if (r1 > n) r1 = n;                                                               // always false; keeps a wrong table inside idx
    const int64_t col = (int64_t)blockIdx.y * kColBlock + threadIdx.x;
    if (col >= d) return;
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t row = idx[r];
        if (row < n) s += (double)(float)img[row * pitch + col];
    }
    partial[(int64_t)c * d + col] = s;
}

// c -> its P planes at img[p * dp] (p = 0 .. P - 1, stride in elements); false where a plane is not finite (|c| past the dtype's range)
template <typename T>
__device__ __forceinline__ bool write_planes(float c, T* img, int64_t dp) {
    bool ok = true;
    float r = c;
#pragma unroll
    for (int p = 0; p < Planes<T>::value; ++p) {
        const T v = (T)r;
        const float f = (float)v;
        img[p * dp] = v;
        ok = ok && isfinite(f);
        r -= f;
    }
    return ok;
}

// One wave per row of the centroid image (k_pad rows, Planes<T> * dp elements each):
// (planes and h are those of g c, g the power of two the rows' image is scaled by: 1 but for float16 rows)
//   partial == nullptr  every row from cent [k x d] as given: planes, zero padding columns, h = -|c|^2 / 2 (-inf on rows >= k);
//                       *bad counts the centroids whose h or planes are not finite;
//   partial != nullptr  every cluster with rows: cent = float32(sum of its chunk partials in ascending order / count), then as above.
//                       A cluster without rows keeps cent, its planes and h.
template <typename T>
__global__ void __launch_bounds__(256) centroid_finish_kernel(const double* __restrict__ partial, const uint32_t* __restrict__ starts,
                                                              const uint32_t* __restrict__ chunk0, int64_t k, int64_t k_pad, int64_t d, int64_t dp,
                                                              float* __restrict__ cent, T* __restrict__ img, float* __restrict__ h, float g,
                                                              unsigned long long* __restrict__ bad) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= k_pad) return;
    uint32_t c0 = 0, c1 = 0;
    double count = 0.0;
    if (partial) {
        if (row >= k) return;
        count = (double)(starts[row + 1] - starts[row]);
        if (count == 0.0) return;
        c0 = chunk0[row]; c1 = chunk0[row + 1];
    }
    T* out = img + row * (Planes<T>::value * dp);
    float s = 0.f;
    bool ok = true;
    for (int64_t col = lane; col < dp; col += 64) {
        float c = 0.f;
        if (row < k && col < d) {
            if (partial) {
                double sum = 0.0;
                for (uint32_t q = c0; q < c1; ++q) sum += partial[(int64_t)q * d + col];
                c = (float)(sum / count);
                cent[row * d + col] = c;
            } else {
                c = cent[row * d + col];
            }
        }
        const float cg = c * g;
        ok = write_planes<T>(cg, out + col, dp) && ok;
        s = fmaf(cg, cg, s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float hv = row < k ? -0.5f * s : -INFINITY;
    const bool wrong = row < k && (!ok || !isfinite(hv));
    const unsigned long long any = __ballot(wrong);
    if (lane == 0) {
        h[row] = hv;
        if (any && bad) atomicAdd(bad, 1ull);
    }
}

// out: every row of img (n_pad rows of dp elements, dp * sizeof(T) a multiple of 16 bytes) times g, Planes<T> times side by side.  g is a
// power of two that keeps every element in range (kmeans_scale), so the products are exact.  A thread moves 16 bytes.
template <typename T>
__global__ void __launch_bounds__(256) replicate_kernel(const T* __restrict__ img, int64_t n_pad, int64_t dp, float g, T* __restrict__ out) {
    constexpr int kVec = 16 / (int)sizeof(T);
    const int64_t row_vecs = dp / kVec, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad * row_vecs) return;
    const int64_t row = i / row_vecs, v = i % row_vecs;
    union { uint4 u; T e[kVec]; } x;
    x.u = *reinterpret_cast<const uint4*>(img + i * kVec);
#pragma unroll
    for (int q = 0; q < kVec; ++q) x.e[q] = (T)((float)x.e[q] * g);
    for (int p = 0; p < Planes<T>::value; ++p) *reinterpret_cast<uint4*>(out + ((row * Planes<T>::value + p) * row_vecs + v) * kVec) = x.u;
}

// *out = max(*out, the largest |bits| of count float16 values): for finite values the bit patterns without the sign order as the
// magnitudes (an integer atomic: the order does not matter)
__global__ void __launch_bounds__(256) absmax_f16_kernel(const uint16_t* __restrict__ img, int64_t count, unsigned int* __restrict__ out) {
    __shared__ unsigned int red[256];
    unsigned int m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const unsigned int b = img[i] & 0x7fffu;
        m = b > m ? b : m;
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x + w] > red[threadIdx.x] ? red[threadIdx.x + w] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicMax(out, red[0]);
}

// out[i] = in[i] * s (s a power of two; in == out is fine)
__global__ void __launch_bounds__(256) scale_kernel(const float* __restrict__ in, float s, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i] * s;
}

// *changed += the rows whose two labels differ (integer arithmetic: one count per workgroup, one integer atomic)
__global__ void __launch_bounds__(256) labels_changed_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t n,
                                                             unsigned long long* __restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = __syncthreads_count(i < n && a[i] != b[i]);
    if (threadIdx.x == 0 && c) atomicAdd(changed, (unsigned long long)c);
}

// *out = the n values summed in float64 in a fixed order (one workgroup: thread t adds t, t + 256, ...; then a tree over the threads)
__global__ void __launch_bounds__(256) inertia_kernel(const float* __restrict__ dist2, int64_t n, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)dist2[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// What one update works in: everything but cent / img / h, which are the caller's centroid operand.
struct UpdateScratch {
    uint32_t* keys; uint32_t* keys_tmp; uint32_t* idx; uint32_t* idx_tmp;             // [n] each
    uint32_t* sort_counts; uint32_t* sort_bases;                                      // sort_counts_elems(n), 256
    uint32_t* counts; uint32_t* starts; uint32_t* chunk0; uint32_t* stats;            // [k], [k + 1], [k + 1], [2]
    double* partial;                                                                  // chunks_bound(n, k) * d
};

// M(A): cent / img / h of every cluster with rows from `labels` [n] (values in 0 .. k - 1) and the rows' image `rows` (`pitch` elements
// a row).  Enqueued on st.  After it counts, starts, chunk0 and stats describe the labels.
template <typename T>
inline hipError_t update(const int32_t* labels, int64_t n, int64_t k, int64_t k_pad, int64_t d, int64_t dp, const T* rows, int64_t pitch,
                         const UpdateScratch& w, float* cent, T* img, float* h, float g, hipStream_t st) {
    hipError_t e = hipMemsetAsync(w.counts, 0, (size_t)k * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    label_count_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(labels, n, k, w.keys, w.counts);
    cluster_scan_kernel<<<1, 256, 0, st>>>(w.counts, k, w.starts, w.chunk0, w.stats);
    e = ssort::sort_segment_pairs(reinterpret_cast<float*>(w.keys), reinterpret_cast<float*>(w.keys_tmp), w.idx, w.idx_tmp, n, n, 1,
                                  w.sort_counts, w.sort_bases, st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)chunks_bound(n, k), (unsigned)((d + kColBlock - 1) / kColBlock));
    chunk_sum_kernel<T><<<grid, kColBlock, 0, st>>>(rows, pitch, n, w.idx, w.starts, w.chunk0, k, d, w.partial);
    centroid_finish_kernel<T><<<(unsigned)((k_pad + 3) / 4), 256, 0, st>>>(w.partial, w.starts, w.chunk0, k, k_pad, d, dp, cent, img, h, g, nullptr);
    return hipGetLastError();
}
#endif

}  // namespace kmeans
}  // namespace fad
