// Kernel Audio Distance: the unbiased Gaussian-kernel MMD^2 between two sets of embedding rows, and the median pairwise distance
// of one set (the default bandwidth).  DESIGN.md 4.6.  Per-song KAD (4.7), the k-NN precision / recall / density / coverage (4.8),
// KAD's standard errors (4.9), its permutation test (4.10), the nearest baseline rows with authenticity (4.11), KAD at several
// bandwidths in one pass (4.12), the permutation test at several bandwidths, aggregated (4.13), the leave-one-out k-NN two-sample
// test on the pooled rows (4.14), the polynomial-kernel distance of the KID protocol (4.15) and the Sinkhorn divergence (4.16) run on
// the same main loop; the sliced Wasserstein distance (4.17) takes its projections from it, and Lloyd's k-means (4.22) its assignment
// (the nearest pass of 4.11 with the centroids as the row operand; csrc/kmeans_update.h has the rest).
//
// Every pass is one GEMM-shaped walk over 128 x 128 tiles of a pair space (kad_tiles.h) whose n x m matrix is never stored:
//   - pack:   each set is copied once into a zero-padded [n_pad x dp] image of its own dtype (dp: D rounded up to 128 bytes, n_pad:
//             whole tiles) and h[i] = -|x_i|^2 / 2 in float32 from the same 16-bit values (-inf on the padding rows);
//   - sums:   the dot products run on v_mfma_f32_32x32x16_{f16,bf16} (v_mfma_f32_32x32x2_f32 for float32 rows) into accumulators
//             that START at h[i] + h[j], so the chain ends at S' = x.y - (|x|^2 + |y|^2) / 2 = -d^2 / 2 and the epilogue is
//             k = exp2(min(c * S', 0)), c = log2(e) / sigma^2 -- a padding row's -inf gives k = 0 with no mask;
//             per lane float32 over one tile, float64 from there on, one float64 slot per workgroup, slots summed in a fixed order:
//             bitwise the same result on every run (no float atomics);
//   - median: the same walk over the baseline's triangle with a histogram epilogue -- an exact radix select on the bit patterns
//             of the clamped float32 d^2 (11 / 11 / 10 bits, LDS histograms, integer global counts).
// The _k entry points take the kernel: FAD_KAD_GAUSSIAN as above, or the heavy-tailed FAD_KAD_IQ k = 1 / (1 + t) and FAD_KAD_IMQ
// k = 1 / sqrt(1 + t), t = d^2 / (2 sigma^2) = -c S' with c = 1 / sigma^2 -- a compile-time parameter of the epilogues (kernel_value).
// The cross pass always runs with the larger set (by rows, then by sum of row norms) as the row operand, so that swapping the
// arguments adds exactly the same tile sums.  KAD's code object is loaded at its first call, not by check_device's warm-up.
#include "fad_common.h"
#include "kad_tiles.h"
#include "kad_song_tiles.h"
#include "kad_unc_tiles.h"
#include "kad_perm_tiles.h"
#include "kad_perm_sweep_tiles.h"
#include "kid_tiles.h"
#include "nn_vote.h"
#include "sliced_sort.h"
#include "sliced_sort_pairs.h"
#include "sliced_song_sort.h"
#include "sliced_split.h"
#include "sliced_expand.h"
#include "kmeans_update.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <optional>
#include <type_traits>
#include <vector>

namespace fad {
namespace {

using kad::kTile;
constexpr int kThreads = 256;                  // 4 waves, 2 x 2 over the tile, 64 x 64 each (2 x 2 MFMA blocks of 32 x 32)
constexpr int kChunk = 128;                    // bytes of a row per k step of the main loop (64 halves / 32 floats)
constexpr int kLdsRow = kChunk + 16;           // padded LDS row
constexpr int kOpBytes = kTile * kLdsRow;      // one operand's LDS image
constexpr int kHistBins = 2048;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

enum Mode { MODE_SUM = 0, MODE_HIST = 1 };

struct PassArgs {
    const char* a; const char* b;              // packed images (row pitch `pitch` bytes)
    const float* ha; const float* hb;          // -|row|^2 / 2, -inf on padding rows
    int64_t pitch, n_a, n_b;                   // n_b == n_a for a triangle
    int64_t u0, cnt, tiles_j;                  // launch's tiles [u0, u0 + cnt); triangle: T, rectangle: TJ
    int tri, nchunks;
    float c;                                   // log2(e) / sigma^2, 1 / sigma^2 for iq and imq (MODE_SUM)
    double* slots;                             // MODE_SUM: one per workgroup of the launch
    unsigned long long* hist;                  // MODE_HIST: [2][kHistBins] integer counts
    unsigned int pref0, pref1; int two, hi_shift, lo_shift, bits;
};

// One k step of 128 bytes of both operands, from LDS, into the wave's four accumulators.
template <int DT>
__device__ __forceinline__ void chunk_mfma(const char* la, const char* lb, int lane, f32x16 (&acc)[2][2]) {
    const int r = lane & 31, h = lane >> 5;
    if constexpr (DT == FAD_F32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {                      // lane half h holds k = 8q + 4h + e for step e: the same k order in A and B
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[t] = *reinterpret_cast<const f32x4*>(la + (t * 32 + r) * kLdsRow + q * 32 + h * 16);
                fb[t] = *reinterpret_cast<const f32x4*>(lb + (t * 32 + r) * kLdsRow + q * 32 + h * 16);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj)
                        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[bi][e], fb[bj][e], acc[bi][bj], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {                      // 16 elements a step, lane half h the 8 at byte 32s + 16h
            u32x4 fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[t] = *reinterpret_cast<const u32x4*>(la + (t * 32 + r) * kLdsRow + s * 32 + h * 16);
                fb[t] = *reinterpret_cast<const u32x4*>(lb + (t * 32 + r) * kLdsRow + s * 32 + h * 16);
            }
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) {
                    if constexpr (DT == FAD_F16)
                        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[bi]), __builtin_bit_cast(f16x8, fb[bj]),
                                                                             acc[bi][bj], 0, 0, 0);
                    else
                        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[bi]), __builtin_bit_cast(bf16x8, fb[bj]),
                                                                              acc[bi][bj], 0, 0, 0);
                }
        }
    }
}

// k(S') of one accumulator element, KF one of FAD_KAD_*.  Three instructions either way: mul / min / exp2, or fma / max / rcp (rsq).
template <int KF>
__device__ __forceinline__ float kernel_value(float acc, float c) {
    if constexpr (KF == FAD_KAD_GAUSSIAN) {
        // c > 0, so min(S', 0) * c == min(S' * c, 0).  The multiply is an ordinary VALU op that reads the MFMA result, so the
        // compiler places the MFMA -> VALU wait states before it; the clamp then reads only that VALU result.  (An inline-asm read
        // of the accumulator itself would get no wait states: the hazard recognizer does not look inside asm.)  The clamp is asm so
        // that no canonicalising v_max comes with it.
        float v = acc * c, w;
        asm("v_min_f32 %0, 0, %1" : "=v"(w) : "v"(v));
        return __builtin_amdgcn_exp2f(w);
    } else {
        // u = 1 + t, t = -c S' >= 0 up to rounding; the same two properties: the fma is the ordinary op that reads the MFMA result, the
        // clamp to u >= 1 is asm on the fma's result.  A padding row's -inf gives u = +inf and k = 0; a NaN clamps to 1, so k = 1 (as
        // the Gaussian's min does).
        float u = fmaf(acc, -c, 1.0f), w;
        asm("v_max_f32 %0, 1.0, %1" : "=v"(w) : "v"(u));
        return KF == FAD_KAD_IQ ? __builtin_amdgcn_rcpf(w) : __builtin_amdgcn_rsqf(w);
    }
}

// k(S') summed over the wave's 64 x 64 pairs of a tile; MASK: a diagonal tile of a triangle counts only column > row
template <bool MASK, int KF>
__device__ __forceinline__ float tile_sum(const f32x16 (&acc)[2][2], float c, int rbase, int cbase, int lane) {
    // The row offset of the lane, opaque to the compiler: the 64 mask comparisons are made here, per diagonal tile, instead of being
    // hoisted out of the tile loop as 64 lane masks (128 SGPRs, spilled to VGPR lanes around the whole loop).
    int lrow = rbase + 4 * (lane >> 5) - (cbase + (lane & 31));
    if (MASK) asm volatile("" : "+v"(lrow));
    float s = 0.f;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                float e = kernel_value<KF>(acc[bi][bj][g], c);
                if (MASK) e = (bj * 32 - bi * 32 - (g & 3) - 8 * (g >> 2)) > lrow ? e : 0.f;     // column > row
                s += e;
            }
    return s;
}

// The main loop of every pass: tile (I, J) -- row block I of `a` against column block J of `b` -- into the wave's accumulators, which
// start at h[i] + h[j].  A barrier first (the previous tile is done with LDS), then h of the tile's rows and columns into LDS, where the
// threads of the rows (tid < kTile) also run `row_lds(tid)`, a pass's own per-row LDS entry; then the k loop, 128 bytes of a row per
// step: global -> registers (one step ahead) -> LDS (padded rows) -> chunk_mfma.
template <int DT, typename RowLds>
__device__ __forceinline__ void tile_mfma(const char* a, const char* b, const float* ha, const float* hb, int64_t pitch, int nchunks,
                                          int64_t I, int64_t J, char* lds, RowLds&& row_lds, f32x16 (&acc)[2][2]) {
    char* la = lds;
    char* lb = lds + kOpBytes;
    float* lh = reinterpret_cast<float*>(lds + 2 * kOpBytes);                          // [0, 128): rows, [128, 256): columns
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const char* ga = a + I * kTile * pitch;
    const char* gb = b + J * kTile * pitch;

    __syncthreads();                                                                  // the previous tile is done with LDS
    if (tid < kTile) {
        lh[tid] = ha[I * kTile + tid];
        row_lds(tid);
    } else {
        lh[tid] = hb[J * kTile + tid - kTile];
    }

    // global -> registers: 128 rows x 128 bytes per operand = 1024 pieces of 16 B, 4 per thread
    u32x4 ra[4], rb[4];
    auto load = [&](int ch) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = (tid >> 3) + 32 * q, col = (tid & 7) * 16;
            ra[q] = *reinterpret_cast<const u32x4*>(ga + row * pitch + ch * kChunk + col);
            rb[q] = *reinterpret_cast<const u32x4*>(gb + row * pitch + ch * kChunk + col);
        }
    };
    load(0);
    __syncthreads();

#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const float hc = lh[kTile + wn * 64 + bj * 32 + (lane & 31)];
#pragma unroll
            for (int g = 0; g < 16; ++g)
                acc[bi][bj][g] = lh[wm * 64 + bi * 32 + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5)] + hc;
        }

    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch) __syncthreads();                                                      // everybody is through the last chunk
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = (tid >> 3) + 32 * q, col = (tid & 7) * 16;
            *reinterpret_cast<u32x4*>(la + row * kLdsRow + col) = ra[q];
            *reinterpret_cast<u32x4*>(lb + row * kLdsRow + col) = rb[q];
        }
        __syncthreads();
        if (ch + 1 < nchunks) load(ch + 1);                                           // in flight under this chunk's MFMAs
        chunk_mfma<DT>(la + wm * 64 * kLdsRow, lb + wn * 64 * kLdsRow, lane, acc);
    }
}

template <int DT, int MODE, int KF = FAD_KAD_GAUSSIAN>
__global__ void __launch_bounds__(kThreads, 2) kad_pass_kernel(PassArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    unsigned int* lhist = reinterpret_cast<unsigned int*>(lds + 2 * kOpBytes + 2 * kTile * 4);   // MODE_HIST: [2][kHistBins]
    double* lred = reinterpret_cast<double*>(lds + 2 * kOpBytes + 2 * kTile * 4);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);
    if (MODE == MODE_HIST) {
        for (int i = tid; i < 2 * kHistBins; i += kThreads) lhist[i] = 0;
    }
    double dsum = 0.0;

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const kad::Tile t = p.tri ? kad::tri_tile(p.u0 + v, p.tiles_j) : kad::rect_tile(p.u0 + v, p.tiles_j);
        f32x16 acc[2][2];
        tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, t.I, t.J, lds, [](int) {}, acc);

        const int rbase = wm * 64, cbase = wn * 64;
        if (MODE == MODE_SUM) {
            const float s = (p.tri && t.I == t.J) ? tile_sum<true, KF>(acc, p.c, rbase, cbase, lane) : tile_sum<false, KF>(acc, p.c, rbase, cbase, lane);
            dsum += (double)s;
        } else {
            const uint64_t mask = (1ull << p.bits) - 1;
            int lr = rbase + 4 * (lane >> 5), lc = cbase + (lane & 31);
            asm volatile("" : "+v"(lr), "+v"(lc));            // per tile, not hoisted out of the tile loop as 64 lane masks (tile_sum)
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        const int r = lr + bi * 32 + (g & 3) + 8 * (g >> 2), c = lc + bj * 32;
                        if (!kad::pair_counted(p.tri, t.I, t.J, r, c, p.n_a, p.n_b)) continue;
                        const float d2 = fmaxf(-2.f * acc[bi][bj][g], 0.f);
                        const uint64_t key = __float_as_uint(d2);
                        const unsigned int bin = (unsigned int)((key >> p.lo_shift) & mask);
                        if ((key >> p.hi_shift) == p.pref0) atomicAdd(&lhist[bin], 1u);
                        if (p.two && (key >> p.hi_shift) == p.pref1) atomicAdd(&lhist[kHistBins + bin], 1u);
                    }
        }
    }

    __syncthreads();
    if (MODE == MODE_SUM) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off, 64);
        if (lane == 0) lred[wave] = dsum;
        __syncthreads();
        if (tid == 0) p.slots[blockIdx.x] = ((lred[0] + lred[1]) + lred[2]) + lred[3];
    } else {
        for (int i = tid; i < 2 * kHistBins; i += kThreads)
            if (lhist[i]) atomicAdd(&p.hist[i], (unsigned long long)lhist[i]);     // integer counts: order does not matter
    }
}

constexpr size_t kLdsSum = 2 * kOpBytes + 2 * kTile * 4 + 4 * sizeof(double);
constexpr size_t kLdsHist = 2 * kOpBytes + 2 * kTile * 4 + 2 * kHistBins * 4;

// One wave per row: the zero-padded image row, h = -|row|^2 / 2 in float32 (-inf on rows >= n).
template <typename T>
__global__ void __launch_bounds__(256) kad_pack_kernel(const T* __restrict__ x, int64_t n, int64_t ld, int64_t d, T* __restrict__ out,
                                                       int64_t dp, int64_t n_pad, float* __restrict__ h) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n_pad) return;
    float s = 0.f;
    for (int64_t c = lane; c < dp; c += 64) {
        T v = T(0.f);
        if (row < n && c < d) v = x[row * ld + c];
        out[row * dp + c] = v;
        const float f = (float)v;
        s = fmaf(f, f, s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) h[row] = row < n ? -0.5f * s : -INFINITY;
}

// info[0] = sum of |row|^2 in float64 (fixed order), info[1] = rows whose norm is not finite
__global__ void __launch_bounds__(256) kad_norm_info_kernel(const float* __restrict__ h, int64_t n, double* __restrict__ info) {
    __shared__ double ssum[256];
    __shared__ double sbad[256];
    double s = 0.0, bad = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float v = h[i];
        if (isfinite(v)) s += -2.0 * (double)v; else bad += 1.0;
    }
    ssum[threadIdx.x] = s; sbad[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { ssum[threadIdx.x] += ssum[threadIdx.x + w]; sbad[threadIdx.x] += sbad[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { info[0] = ssum[0]; info[1] = sbad[0]; }
}

// out[p] = the slots [off[p], off[p + 1]) summed in a fixed order (one workgroup per pass)
__global__ void __launch_bounds__(256) kad_slots_sum_kernel(const double* __restrict__ slots, const int64_t* __restrict__ off,
                                                            double* __restrict__ out) {
    __shared__ double red[256];
    const int64_t b = off[blockIdx.x], e = off[blockIdx.x + 1];
    double s = 0.0;
    for (int64_t i = b + threadIdx.x; i < e; i += 256) s += slots[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// ------------------------------------------------------------------------------------------------- bandwidth sweep
// fad_kad_sweep's sum pass: kad_pass_kernel<DT, MODE_SUM, KF> with NB constants c[b] instead of one.  The pair GEMM does not depend on
// sigma, so a tile's accumulators are formed once and read NB times: element by element in tile_sum's order (bi, bj, g), bandwidth b's
// kernel value into b's own per-lane float partial, per tile into b's own double, and at the end b's own butterfly and
// ((l0 + l1) + l2) + l3 into b's own slot of the workgroup, slots[b * stride + workgroup].  Bandwidth b therefore adds exactly what
// kad_pass_kernel adds with c = c[b], in the same order: the same bits wherever the two make the same launch cut.
template <int NB>
struct SweepArgs {
    PassArgs p;                                // p.c is not read; p.slots: the pass's slots of bandwidth 0 from this launch on
    int64_t stride;                            // slots of the whole pass per bandwidth
    float c[NB];
};

template <bool MASK, int KF, int NB>
__device__ __forceinline__ void tile_sum_sweep(const f32x16 (&acc)[2][2], const float (&c)[NB], int rbase, int cbase, int lane,
                                               float (&s)[NB]) {
    int lrow = rbase + 4 * (lane >> 5) - (cbase + (lane & 31));
    if (MASK) asm volatile("" : "+v"(lrow));                                          // as tile_sum
#pragma unroll
    for (int b = 0; b < NB; ++b) s[b] = 0.f;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const bool keep = !MASK || (bj * 32 - bi * 32 - (g & 3) - 8 * (g >> 2)) > lrow;       // column > row
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float e = kernel_value<KF>(acc[bi][bj][g], c[b]);     // every read of the accumulator is kernel_value's mul / fma
                    if (MASK) e = keep ? e : 0.f;
                    s[b] += e;
                }
            }
}

template <int DT, int KF, int NB>
__global__ void __launch_bounds__(kThreads, 2) kad_sweep_kernel(SweepArgs<NB> q) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double* lred = reinterpret_cast<double*>(lds + 2 * kOpBytes + 2 * kTile * 4);     // [NB][4]
    const PassArgs& p = q.p;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);
    double dsum[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) dsum[b] = 0.0;
    // Thread b < NB writes bandwidth b's slot at the end.  Its address is formed here and made opaque, so it waits in two VGPRs, of which
    // there are enough; left to the end, the slots pointer and the stride wait in SGPRs, two of which were spilled around the tile loop.
    double* dst = p.slots + (tid * q.stride + blockIdx.x);
    asm volatile("" : "+v"(dst));

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const kad::Tile t = p.tri ? kad::tri_tile(p.u0 + v, p.tiles_j) : kad::rect_tile(p.u0 + v, p.tiles_j);
        f32x16 acc[2][2];
        tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, t.I, t.J, lds, [](int) {}, acc);

        const int rbase = wm * 64, cbase = wn * 64;
        float s[NB];
        if (p.tri && t.I == t.J) tile_sum_sweep<true, KF, NB>(acc, q.c, rbase, cbase, lane, s);
        else tile_sum_sweep<false, KF, NB>(acc, q.c, rbase, cbase, lane, s);
#pragma unroll
        for (int b = 0; b < NB; ++b) dsum[b] += (double)s[b];
    }

    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum[b] += __shfl_xor(dsum[b], off, 64);
        if (lane == 0) lred[4 * b + wave] = dsum[b];
    }
    __syncthreads();
    if (tid < NB) *dst = ((lred[4 * tid] + lred[4 * tid + 1]) + lred[4 * tid + 2]) + lred[4 * tid + 3];
}

constexpr int kSweepGroup = 8;                 // bandwidths per pass at most: the largest NB instantiated (4 and 8)
template <int NB>
constexpr size_t lds_sweep() { return 2 * kOpBytes + 2 * kTile * 4 + NB * 4 * sizeof(double); }

// ------------------------------------------------------------------------------------------------- per-song passes
// fad_kad_individual's cross (X x Y) and band (Y x Y inside each song) passes: tile_mfma, with an epilogue that keeps per-column
// sums (kad_song_tiles.h).  In the 32 x 32 MFMA layout a lane owns its column, so a column's sum over a tile
// is 32 in-register adds per lane; the two lane halves and the two wm waves of a column meet once, at the end of a work unit.
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct ColArgs {
    const char* a; const char* b;              // row operand (X, or Y for the band), column operand (Y)
    const float* ha; const float* hb;
    int64_t pitch;
    int nchunks;
    float c;                                   // log2(e) / sigma^2, 1 / sigma^2 for iq and imq
    int64_t u0, cnt;                           // the launch's units [u0, u0 + cnt)
    int64_t TI, TJ, rr;                        // cross: the unit map
    const kad::Unit* units;                    // band: (J, I0, I1) per unit
    const int* row_end;                        // band: offsets[song(i) + 1] per row of Y, 0 on padding rows
    double* slots; int64_t slot_pitch;         // cross: slots[R * slot_pitch + j]; band: slots[u * kTile + c]
};

// k(S') of the wave's 64 rows of a tile added into the lane's two columns (cbase + 32 bj + lane % 32); MASK 0: every pair, 1: a
// diagonal tile (column > row), 2: a band tile holding more than one song (column < end of the row's song, and on a diagonal tile
// column > row), 3: a diagonal tile of a full square (column != row).  Masks are selects: a NaN row that the clamp turned into k = 1
// still adds nothing where it is masked.
template <int MASK, int KF>
__device__ __forceinline__ void col_sums(const f32x16 (&acc)[2][2], float c, int rbase, int cbase, int lane, const int* lend, bool diag,
                                         double (&dcol)[2]) {
    int lrow = rbase + 4 * (lane >> 5), lcol = cbase + (lane & 31);
    if (MASK) asm volatile("" : "+v"(lrow), "+v"(lcol));         // per tile, not hoisted out of the tile loop as lane masks (tile_sum)
    i32x4 le[2][4];
    if (MASK == 2) {
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int q = 0; q < 4; ++q) le[bi][q] = *reinterpret_cast<const i32x4*>(lend + lrow + bi * 32 + 8 * q);
    }
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        float s = 0.f;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                float e = kernel_value<KF>(acc[bi][bj][g], c);    // as tile_sum
                const int r = lrow + bi * 32 + (g & 3) + 8 * (g >> 2), col = lcol + bj * 32;
                if (MASK == 1) e = col > r ? e : 0.f;
                if (MASK == 2) e = (col < le[bi][g >> 2][g & 3] && (!diag || col > r)) ? e : 0.f;
                if (MASK == 3) e = col != r ? e : 0.f;
                s += e;
            }
        dcol[bj] += (double)s;
    }
}

template <int DT, bool BAND, int KF>
__global__ void __launch_bounds__(kThreads, 2) kad_cols_kernel(ColArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int* lend = reinterpret_cast<int*>(lds + 2 * kOpBytes + 2 * kTile * 4);           // BAND: end of each row's song - J * 128, in [0, 128]
    double* lx = reinterpret_cast<double*>(lds + 2 * kOpBytes + 3 * kTile * 4);       // the wm = 1 waves' column sums of a unit

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, cbase = wn * 64;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = BAND ? p.units[u] : kad::cross_unit(u, p.TI, p.TJ, p.rr);
        double dcol[2] = {0.0, 0.0};

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [&](int r) {
                if constexpr (BAND) {
                    const int64_t e = (int64_t)p.row_end[I * kTile + r] - un.J * kTile;
                    lend[r] = e < 0 ? 0 : e > kTile ? kTile : (int)e;
                }
            }, acc);

            if (BAND) {
                const bool diag = I == un.J;
                if (lend[0] >= kTile) {                                               // the tile lies inside one song (uniform)
                    if (diag) col_sums<1, KF>(acc, p.c, rbase, cbase, lane, lend, true, dcol);
                    else col_sums<0, KF>(acc, p.c, rbase, cbase, lane, lend, false, dcol);
                } else {
                    col_sums<2, KF>(acc, p.c, rbase, cbase, lane, lend, diag, dcol);
                }
            } else {
                col_sums<0, KF>(acc, p.c, rbase, cbase, lane, lend, false, dcol);
            }
        }

        // a column: the two lane halves, then the wm = 0 and wm = 1 waves, in this order
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) dcol[bj] += __shfl_xor(dcol[bj], 32, 64);
        if (wm == 1 && lane < 32) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) lx[cbase + bj * 32 + lane] = dcol[bj];
        }
        __syncthreads();
        if (wm == 0 && lane < 32) {
            double* slot = BAND ? p.slots + u * kTile : p.slots + (u / p.TJ) * p.slot_pitch + un.J * kTile;
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) slot[cbase + bj * 32 + lane] = dcol[bj] + lx[cbase + bj * 32 + lane];
        }
    }
}

constexpr size_t kLdsCols = 2 * kOpBytes + 3 * kTile * 4 + kTile * sizeof(double);

// row_end[i] = offsets[song(i) + 1] for the rows of Y (the last song s with offsets[s] <= i), 0 on the padding rows
__global__ void __launch_bounds__(256) kad_row_end_kernel(const int64_t* __restrict__ offsets, int64_t n_songs, int64_t m, int64_t m_pad,
                                                          int* __restrict__ row_end) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m_pad) return;
    if (i >= m) { row_end[i] = 0; return; }
    row_end[i] = (int)offsets[kad::song_of_row(offsets, n_songs, i) + 1];
}

// One workgroup per song: r_xy(j) = sum over the cross slot rows, r_yy(j) = sum over the band units of j's column block, both in a
// fixed order, then summed over the song's rows in a fixed order -> Kxy, Kyy and a status (too few rows, a non-finite row norm).
__global__ void __launch_bounds__(256) kad_song_reduce_kernel(const double* __restrict__ cross, int64_t nr, int64_t pitch,
                                                              const double* __restrict__ band, const int64_t* __restrict__ band_start,
                                                              const float* __restrict__ hy, const int64_t* __restrict__ offsets, double n,
                                                              double* __restrict__ kyy, double* __restrict__ kxy, int* __restrict__ status) {
    __shared__ double rx[256];
    __shared__ double ry[256];
    __shared__ int rbad[256];
    const int64_t s = blockIdx.x, b = offsets[s], e = offsets[s + 1], m = e - b;
    double sx = 0.0, sy = 0.0;
    int bad = 0;
    for (int64_t j = b + threadIdx.x; j < e; j += 256) {
        double x = 0.0, y = 0.0;
        for (int64_t R = 0; R < nr; ++R) x += cross[R * pitch + j];
        const int64_t J = j / kTile;
        for (int64_t u = band_start[J]; u < band_start[J + 1]; ++u) y += band[u * kTile + (j - J * kTile)];
        sx += x;
        sy += y;
        bad |= !isfinite(hy[j]);
    }
    rx[threadIdx.x] = sx; ry[threadIdx.x] = sy; rbad[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            rx[threadIdx.x] += rx[threadIdx.x + w];
            ry[threadIdx.x] += ry[threadIdx.x + w];
            rbad[threadIdx.x] |= rbad[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double md = (double)m;
        if (m < 2 || rbad[0]) {
            status[s] = m < 2 ? FAD_ERR_TOO_FEW_ROWS : FAD_ERR_NOT_FINITE;
            kyy[s] = kxy[s] = NAN;
        } else {
            status[s] = FAD_OK;
            kxy[s] = rx[0] / (n * md);
            kyy[s] = 2.0 * ry[0] / (md * (md - 1.0));
        }
    }
}

// ------------------------------------------------------------------------------------------ Sinkhorn divergence
// One Sinkhorn half-step is the cross pass above with a soft-min epilogue: for every column j, LSE_i((p_i + S'_ij) / eps) over the rows
// i, S' = a.b + h_a + h_b = -C.  The row potential rides in the row operand's h vector (ha[i] = h_a[i] + p_i, still -inf on padding
// rows), so the main loop is tile_mfma's, unchanged, and the accumulators end at v = p_i - C_ij.  No clamp of C at 0: no root is taken.
// A column's state is the pair (M, S) = (max v, sum of exp2((v - M) c)), c = log2(e) / eps: M stays in the units of v, so it enters the
// new potential unscaled, and the exponent is formed from the difference to the maximum, never from v / eps itself.  A state with
// nothing in it is (-inf, 0); merges take the reference 0 in place of a maximum of -inf, so -inf - (-inf) is never formed and a
// padding row adds exp2(-inf) = 0 exactly.
struct SoftminArgs {
    const char* a; const char* b;              // row operand (reduced over), column operand
    const float* ha; const float* hb;          // ha: h + potential of the rows; hb: h of the columns
    int64_t pitch;
    int nchunks;
    float c;                                   // log2(e) / eps
    int64_t u0, cnt;                           // the launch's units [u0, u0 + cnt)
    int64_t TI, TJ, rr;                        // the cross unit map
    float2* slots; int64_t slot_pitch;         // slots[R * slot_pitch + j] = (M, S) of column j over row range R
};

__device__ __forceinline__ float lse_ref(float m) { return m == -INFINITY ? 0.f : m; }

// (M, S) <- (M, S) merged with (m2, s2), in this order
__device__ __forceinline__ void lse_merge(float& M, float& S, float m2, float s2, float c) {
    const float nm = fmaxf(M, m2), ref = lse_ref(nm);
    S = S * __builtin_amdgcn_exp2f((M - ref) * c) + s2 * __builtin_amdgcn_exp2f((m2 - ref) * c);
    M = nm;
}

// the wave's 64 rows of a tile merged into the states of the lane's two columns: the maximum of the lane's 32 values of a column, their
// sum against it, one merge into the running state
__device__ __forceinline__ void col_softmin(const f32x16 (&acc)[2][2], float c, float (&M)[2], float (&S)[2]) {
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        float tm = -INFINITY;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int g = 0; g < 16; ++g) tm = fmaxf(tm, acc[bi][bj][g]);
        const float ref = lse_ref(tm);
        float ts = 0.f;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int g = 0; g < 16; ++g) ts += __builtin_amdgcn_exp2f((acc[bi][bj][g] - ref) * c);
        lse_merge(M[bj], S[bj], tm, ts, c);
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads, 2) sinkhorn_cols_kernel(SoftminArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float2* lx = reinterpret_cast<float2*>(lds + 2 * kOpBytes + 2 * kTile * 4);       // the wm = 1 waves' column states of a unit

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int cbase = wn * 64;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = kad::cross_unit(u, p.TI, p.TJ, p.rr);
        float M[2] = {-INFINITY, -INFINITY}, S[2] = {0.f, 0.f};

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [](int) {}, acc);
            col_softmin(acc, p.c, M, S);
        }

        // a column: the lower lane half merged with the upper, then the wm = 0 wave with the wm = 1 wave, in this order
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const float om = __shfl_xor(M[bj], 32, 64), os = __shfl_xor(S[bj], 32, 64);
            const bool lo = lane < 32;
            float m1 = lo ? M[bj] : om, s1 = lo ? S[bj] : os;
            lse_merge(m1, s1, lo ? om : M[bj], lo ? os : S[bj], p.c);
            M[bj] = m1; S[bj] = s1;
        }
        if (wm == 1 && lane < 32) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) lx[cbase + bj * 32 + lane] = make_float2(M[bj], S[bj]);
        }
        __syncthreads();
        if (wm == 0 && lane < 32) {
            float2* slot = p.slots + (u / p.TJ) * p.slot_pitch + un.J * kTile;
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                const float2 o = lx[cbase + bj * 32 + lane];
                lse_merge(M[bj], S[bj], o.x, o.y, p.c);
                slot[cbase + bj * 32 + lane] = make_float2(M[bj], S[bj]);
            }
        }
    }
}

constexpr size_t kLdsSoftmin = 2 * kOpBytes + 2 * kTile * 4 + kTile * sizeof(float2);

// One thread per column: the nr row ranges' states merged in unit order, in float64, into the new potential
//   pot[j] = -(M + eps ln S) + eps log(rows)      (= -eps (LSE_i((p_i - C_ij) / eps) - log rows))
// kept in float64 for the outputs, and hp[j] = h[j] + (float)pot[j] for the next half-step, where these columns are the rows (-inf on
// the padding columns; hp NULL: the diagnostic step, whose potential is not adopted).
__global__ void __launch_bounds__(256) sinkhorn_reduce_kernel(const float2* __restrict__ slots, int64_t nr, int64_t pitch,
                                                              const float* __restrict__ h, int64_t n_cols, int64_t n_pad, double c,
                                                              double eps, double eps_log_rows, double* __restrict__ pot,
                                                              float* __restrict__ hp) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_pad) return;
    if (j >= n_cols) {
        pot[j] = 0.0;
        if (hp) hp[j] = -INFINITY;
        return;
    }
    double M = -INFINITY, S = 0.0;
    for (int64_t R = 0; R < nr; ++R) {
        const float2 v = slots[R * pitch + j];
        const double m2 = (double)v.x, nm = fmax(M, m2);
        if (nm == -INFINITY) continue;                                                // nothing in either state yet
        S = S * exp2((M - nm) * c) + (double)v.y * exp2((m2 - nm) * c);
        M = nm;
    }
    const double f = -(M + eps * log(S)) + eps_log_rows;
    pot[j] = f;
    if (hp) hp[j] = h[j] + (float)f;
}

// One problem's sums, each in a fixed order: out[0] = sum f, out[1] = sum g, out[2] = sum_i |exp((f_i - f'_i) / eps) - 1|
__global__ void __launch_bounds__(256) sinkhorn_finish_kernel(const double* __restrict__ f, const double* __restrict__ g,
                                                              const double* __restrict__ f2, int64_t n, int64_t m, double inv_eps,
                                                              double* __restrict__ out) {
    __shared__ double red[3][256];
    double sf = 0.0, sg = 0.0, se = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        sf += f[i];
        se += fabs(expm1((f[i] - f2[i]) * inv_eps));
    }
    for (int64_t j = threadIdx.x; j < m; j += 256) sg += g[j];
    red[0][threadIdx.x] = sf; red[1][threadIdx.x] = sg; red[2][threadIdx.x] = se;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 3) out[threadIdx.x] = red[threadIdx.x][0];
}

// ------------------------------------------------------------------------------------- sliced Wasserstein distance
// The projection pass: P[l, i] = theta_l . x_i for the directions of one chunk, direction-major (a direction's n values are contiguous,
// the segment the sort takes).  tile_mfma with the directions' image as the row operand and the set's image as the column operand, so
// that a wave's 32 lanes of one accumulator element store 32 consecutive floats; both h vectors are one vector of zeros.  The image of
// the directions has kTile rows of zeros after the last direction, so a chunk may start at any direction: its tiles read on into the
// next chunk's rows or into the zeros, and only l < lc and i < n are stored -- no padding row or column reaches the sort.  A value that
// is not finite sets *flag (every writer stores the same word).
struct ProjArgs {
    const char* th; const char* rows;          // the chunk's first direction in the directions' image; the set's image
    const float* zeros;
    int64_t pitch;
    int nchunks;
    int64_t TI, TJ;                            // direction blocks of the chunk, row blocks of the set
    int64_t lc, n;
    float* P; int64_t ppitch;
    unsigned int* flag;
};

template <int DT>
__global__ void __launch_bounds__(kThreads, 2) sliced_project_kernel(ProjArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t total = p.TI * p.TJ;
    bool bad = false;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int64_t I = t / p.TJ, J = t % p.TJ;
        f32x16 acc[2][2];
        tile_mfma<DT>(p.th, p.rows, p.zeros, p.zeros, p.pitch, p.nchunks, I, J, lds, [](int) {}, acc);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                const int64_t i = J * kTile + wn * 64 + bj * 32 + (lane & 31);
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int64_t l = I * kTile + wm * 64 + bi * 32 + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5);
                    const float v = acc[bi][bj][g];
                    if (l < p.lc && i < p.n) {
                        p.P[l * p.ppitch + i] = v;
                        bad |= !(fabsf(v) < INFINITY);
                    }
                }
            }
    }
    if (bad) *p.flag = 1u;
}

constexpr size_t kLdsProject = 2 * kOpBytes + 2 * kTile * 4;
constexpr int kMatchBlock = 256;

// One term of the quantile match: w (a - b)^2 in float64, w an exact integer; the difference, the square and the product are each
// rounded once (contraction into a fused multiply-add is switched off, here and where the terms are added).  (a - b)^2 has the bits
// of (b - a)^2.
__device__ __forceinline__ double sliced_term(int64_t w, double a, double b) {
#pragma clang fp contract(off)
    const double diff = a - b;
    const double sq = diff * diff;
    return (double)w * sq;
}

// One element's side of the match: element e of a sorted set of ne elements, value v, against the sorted other set o [no].  It meets
// the elements j0 .. j1 of o whose quantile interval [j ne, (j + 1) ne) meets [e, e + 1) no (in units of 1 / (ne no)), each with the
// overlap as its weight; the terms are summed over j ascending.  Either set may be the element's.
__device__ __forceinline__ double sliced_overlap_sum(double v, int64_t e, int64_t ne, const float* __restrict__ o, int64_t no) {
#pragma clang fp contract(off)
    const int64_t lo = e * no, hi = lo + no, j0 = lo / ne, j1 = (hi - 1) / ne;
    double s = 0.0;
    for (int64_t j = j0; j <= j1 && j < no; ++j)
        s += sliced_term((hi < (j + 1) * ne ? hi : (j + 1) * ne) - (lo > j * ne ? lo : j * ne), v, (double)o[j]);
    return s;
}

// the workgroup's halving tree over every thread's s, stored in the workgroup's slot
__device__ __forceinline__ void sliced_tree_store(double s, double* __restrict__ slots) {
    __shared__ double red[kMatchBlock];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kMatchBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) slots[blockIdx.x] = red[0];
}

// The quantile match of one chunk: workgroup (direction l, block k) takes the elements i in [256 k, 256 k + 256) of the sorted larger
// set a [na], each its sliced_overlap_sum against the sorted smaller set b [nb], then the tree, one slot per workgroup.  With COST
// (fad_sliced_shares) every element's sum is kept as well: divided once by den[l] = (double)(n m) q_l it goes to
// cost[l][ra[l][i]], ra the row at rank i (ssort::sort_segment_pairs).  ra is a permutation of 0 .. na - 1, so every row of a direction
// is written exactly once: plain 8-byte stores.  Without COST ra, den and cost are never touched; the slots are the same either way.
template <bool COST>
__global__ void __launch_bounds__(kMatchBlock) sliced_match_kernel(const float* __restrict__ a, const uint32_t* __restrict__ ra, int64_t pa,
                                                                   int64_t na, const float* __restrict__ b, int64_t pb, int64_t nb,
                                                                   int64_t nblk, const double* __restrict__ den,
                                                                   double* __restrict__ slots, double* __restrict__ cost) {
    const int64_t l = blockIdx.x / nblk, k = blockIdx.x % nblk, i = k * kMatchBlock + threadIdx.x;
    double s = 0.0;
    if (i < na) {
        s = sliced_overlap_sum((double)a[l * pa + i], i, na, b + l * pb, nb);
        if (COST) {
            const int64_t row = ra[l * pa + i];
            if (row < na) cost[l * pa + row] = s / den[l];                             // always true; keeps a wrong index inside the row
        }
    }
    sliced_tree_store(s, slots);
}

// S[l] = the nblk slots of direction l summed in index order, one thread per direction of the chunk
__global__ void __launch_bounds__(256) sliced_finish_kernel(const double* __restrict__ slots, int64_t nblk, int64_t lc, double* __restrict__ S) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= lc) return;
    double s = 0.0;
    for (int64_t k = 0; k < nblk; ++k) s += slots[l * nblk + k];
    S[l] = s;
}

// ------------------------------------------------------------------------------- sliced Wasserstein bootstrap
// sliced_match_kernel<false> with sizes per pair: pair p = blockIdx.x / nblk is replicate q = p % nq of its direction, its sorted sets
// x + p px [nx[q]] and y + p py [ny[q]].  The larger set leads, x at a tie, as in sliced_sets; block k takes the leading elements
// [256 k, 256 k + 256), each its sliced_overlap_sum, then the tree into slot p nblk + k.  nblk is the launch's (the largest leading set's):
// a pair's blocks past its own ceil(na / 256) leave at once and their slots are never read.
__global__ void __launch_bounds__(kMatchBlock) sliced_match_sized_kernel(const float* __restrict__ x, int64_t px, const float* __restrict__ y,
                                                                         int64_t py, const int32_t* __restrict__ nx,
                                                                         const int32_t* __restrict__ ny, int64_t nq, int64_t nblk,
                                                                         double* __restrict__ slots) {
    const int64_t p = blockIdx.x / nblk, k = blockIdx.x % nblk, i = k * kMatchBlock + threadIdx.x;
    const int64_t n = nx[p % nq], m = ny[p % nq];
    const bool x_larger = n >= m;
    const int64_t na = x_larger ? n : m, nb = x_larger ? m : n;
    if (k * kMatchBlock >= na) return;                                                 // the whole workgroup
    const float* a = x_larger ? x + p * px : y + p * py;
    const float* b = x_larger ? y + p * py : x + p * px;
    double s = 0.0;
    if (i < na) s = sliced_overlap_sum((double)a[i], i, na, b, nb);
    sliced_tree_store(s, slots);
}

// S[p] = the pair's own ceil(na / 256) slots summed in index order, one thread per pair of the launch
__global__ void __launch_bounds__(256) sliced_finish_sized_kernel(const double* __restrict__ slots, int64_t nblk, const int32_t* __restrict__ nx,
                                                                  const int32_t* __restrict__ ny, int64_t nq, int64_t pairs,
                                                                  double* __restrict__ S) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    const int64_t n = nx[p % nq], m = ny[p % nq], na = n >= m ? n : m;
    int64_t mine = (na + kMatchBlock - 1) / kMatchBlock;
    if (mine > nblk) mine = nblk;                                                      // always false; keeps a wrong size inside the pair's slots
    double s = 0.0;
    for (int64_t k = 0; k < mine; ++k) s += slots[p * nblk + k];
    S[p] = s;
}

// ------------------------------------------------------------------------------------ sliced Wasserstein per-row shares
// The other side of sliced_match_kernel<true>: one thread per element j of the sorted smaller set b (y at n == m) sums the same terms
// w_ij (a_i - b_j)^2 over its i0 .. i1 of the sorted larger set a, i ascending, and stores the sum / den[l] at cost[l][rb[l][j]].
// Grid: lc * jblk workgroups.
__global__ void __launch_bounds__(kMatchBlock) sliced_other_cost_kernel(const float* __restrict__ a, int64_t pa, int64_t na,
                                                                        const float* __restrict__ b, const uint32_t* __restrict__ rb,
                                                                        int64_t pb, int64_t nb, int64_t jblk,
                                                                        const double* __restrict__ den, double* __restrict__ cost) {
    const int64_t l = blockIdx.x / jblk, j = (blockIdx.x % jblk) * kMatchBlock + threadIdx.x;
    if (j >= nb) return;
    const double s = sliced_overlap_sum((double)b[l * pb + j], j, nb, a + l * pa, na);
    const int64_t row = rb[l * pb + j];
    if (row < nb) cost[l * pb + row] = s / den[l];                                     // always true; keeps a wrong index inside the row
}

// acc[row] += cost[l][row] over the lc directions of the chunk, l ascending: one thread per row, one running float64 sum per row that
// lives across the chunks
__global__ void __launch_bounds__(256) sliced_share_sum_kernel(const double* __restrict__ cost, int64_t pitch, int64_t n, int64_t lc,
                                                               double* __restrict__ acc) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    double s = acc[row];
    for (int64_t l = 0; l < lc; ++l) s += cost[l * pitch + row];
    acc[row] = s;
}

// ------------------------------------------------------------------------------- per-song sliced Wasserstein distance
// bad[s] = 1 for the song of every row whose h is not finite (a NaN/Inf squared norm): one thread per row, the song by bisection
__global__ void __launch_bounds__(256) sliced_song_norm_kernel(const float* __restrict__ h, int64_t n_rows, const int64_t* __restrict__ off,
                                                               int64_t n_songs, unsigned int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows || isfinite(h[i])) return;
    int64_t lo = 0, hi = n_songs - 1;                      // the first song that ends beyond row i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    bad[lo] = 1u;                                          // every writer stores the same word
}

// The quantile match of one chunk, per song: workgroup (direction l, song s) is sliced_match_kernel and sliced_finish_kernel of the pair
// (x, song s) in one: it walks the blocks of 256 elements of the sorted larger set (x at a tie) in index order, sums each block's terms
// as that kernel does -- per element over its j ascending, the block by the halving tree -- and adds the block's sum to a running
// float64 sum, the finish kernel's order.  The tree needs one barrier a block: every thread stores its sum, then wave 0 forms
// (red[t] + red[t + 128]) + (red[t + 64] + red[t + 192]), the tree's steps 128 and 64 in its own pairing, and the last six steps as lane
// shifts that pair the same elements; the stores alternate between two buffers, so the next block's stores cannot reach what wave 0
// still reads.  The integers are found without a division in the loop: the smaller set never has more elements than the larger, so
// with i nb = j0 na + r (0 <= r < na) element i meets j0 with the weight min(nb, na - r) and, when r + nb > na, j0 + 1 with r + nb - na
// -- sliced_match_kernel's j0 .. j1 and its weights -- and a thread's (j0, r) move from block to block by a fixed step.  Integers, so
// no floating-point result depends on how they were found.  A sorted song whose first or last key is not finite holds a projection
// that is not finite (key_image puts NaNs and infinities at the two ends): it sets bad[s].  Songs without rows are skipped.
struct SongMatchArgs {
    const float* px; int64_t px_pitch, n;                  // the chunk's sorted baseline projections
    const float* pr; int64_t pr_pitch;                     // the songs'
    const int64_t* off; int64_t n_songs;
    double* S;                                             // [chunk directions x n_songs]
    unsigned int* bad;
};

__global__ void __launch_bounds__(kMatchBlock) sliced_song_match_kernel(SongMatchArgs p) {
#pragma clang fp contract(off)
    __shared__ double red[2][kMatchBlock];
    const int tid = threadIdx.x;
    const int64_t l = blockIdx.x / p.n_songs, sg = blockIdx.x % p.n_songs;
    const int64_t o = p.off[sg], m = p.off[sg + 1] - o;
    if (m == 0) return;                                    // uniform over the workgroup
    const float* xs = p.px + l * p.px_pitch;
    const float* ys = p.pr + l * p.pr_pitch + o;
    const bool x_leads = p.n >= m;
    const float* __restrict__ a = x_leads ? xs : ys;
    const float* __restrict__ b = x_leads ? ys : xs;
    const int64_t na = x_leads ? p.n : m, nb = x_leads ? m : p.n, nblk = (na + kMatchBlock - 1) / kMatchBlock;
    if (tid == 0 && (!(fabsf(ys[0]) < INFINITY) || !(fabsf(ys[m - 1]) < INFINITY))) p.bad[sg] = 1u;
    const int64_t step_q = (kMatchBlock * nb) / na, step_r = (kMatchBlock * nb) % na;
    int64_t j0 = ((int64_t)tid * nb) / na, r = ((int64_t)tid * nb) % na;              // of element i = tid; then i += 256 a block
    double run = 0.0;
    for (int64_t k = 0; k < nblk; ++k) {
        const int64_t i = k * kMatchBlock + tid;
        double s = 0.0;
        if (i < na) {
            const double ai = (double)a[i];
            s += sliced_term(nb < na - r ? nb : na - r, ai, (double)b[j0]);
            if (r + nb > na) s += sliced_term(r + nb - na, ai, (double)b[j0 + 1]);
        }
        j0 += step_q; r += step_r;
        if (r >= na) { r -= na; ++j0; }
        double* buf = red[k & 1];
        buf[tid] = s;
        __syncthreads();
        if (tid < 64) {
            const double lo = buf[tid] + buf[tid + 128], hi = buf[tid + 64] + buf[tid + 192];
            double v = lo + hi;
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) v += __shfl_down(v, w, 64);
            if (tid == 0) run += v;
        }
    }
    if (tid == 0) p.S[l * p.n_songs + sg] = run;
}

// ---------------------------------------------------------------------------------------- KAD standard errors
// fad_kad_uncertainty's pass: Z x Z over the units of kad_unc_tiles.h, tile_mfma with col_sums -- every pair on an off-diagonal tile,
// column != row on a diagonal one -- one float64 slot per (unit, column).  Then four small float64 kernels, each in a fixed order:
// the row sums and projections a, b per row of Z; per-set means and the spread of b; the centred cross products of a in partial sums
// over fixed row ranges; those partials summed.
template <int DT, int KF>
__global__ void __launch_bounds__(kThreads, 2) kad_unc_cols_kernel(ColArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double* lx = reinterpret_cast<double*>(lds + 2 * kOpBytes + 2 * kTile * 4);       // the wm = 1 waves' column sums of a unit

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, cbase = wn * 64;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = p.units[u];
        double dcol[2] = {0.0, 0.0};

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [](int) {}, acc);
            if (I == un.J) col_sums<3, KF>(acc, p.c, rbase, cbase, lane, nullptr, true, dcol);
            else col_sums<0, KF>(acc, p.c, rbase, cbase, lane, nullptr, false, dcol);
        }

        // a column: the two lane halves, then the wm = 0 and wm = 1 waves, in this order (kad_cols_kernel)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) dcol[bj] += __shfl_xor(dcol[bj], 32, 64);
        if (wm == 1 && lane < 32) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) lx[cbase + bj * 32 + lane] = dcol[bj];
        }
        __syncthreads();
        if (wm == 0 && lane < 32) {
            double* slot = p.slots + u * kTile;
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) slot[cbase + bj * 32 + lane] = dcol[bj] + lx[cbase + bj * 32 + lane];
        }
    }
}

constexpr size_t kLdsUnc = 2 * kOpBytes + 2 * kTile * 4 + kTile * sizeof(double);

// fad_kad_permutation_sweep's r pass: kad_unc_cols_kernel with NB constants.  A tile's accumulators are formed once and
// col_sums runs on them once per bandwidth, into that bandwidth's own dcol; at the unit's end bandwidth b's columns meet as above and go
// to slots[b * bstride + u * kTile + column].  Bandwidth b therefore adds what kad_unc_cols_kernel adds under c[b], in the same order,
// whatever the launch cut: a unit's slot is written by one workgroup.  Rows b >= nb of the kernel are idle (a uniform branch).
template <int NB>
struct ColSweepArgs {
    ColArgs p;                                 // p.c is not read; p.slots: bandwidth 0's unit slots
    int nb;
    int64_t bstride;                           // doubles between two bandwidths' unit slots
    float c[NB];
};

template <int DT, int KF, int NB>
__global__ void __launch_bounds__(kThreads, 2) kad_unc_cols_sweep_kernel(ColSweepArgs<NB> q) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double* lx = reinterpret_cast<double*>(lds + 2 * kOpBytes + 2 * kTile * 4);       // [NB][kTile]: the wm = 1 waves' column sums of a unit
    const ColArgs& p = q.p;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, cbase = wn * 64;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = p.units[u];
        double dcol[NB][2];
#pragma unroll
        for (int b = 0; b < NB; ++b) dcol[b][0] = dcol[b][1] = 0.0;

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [](int) {}, acc);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (b >= q.nb) continue;                                              // uniform
                if (I == un.J) col_sums<3, KF>(acc, q.c[b], rbase, cbase, lane, nullptr, true, dcol[b]);
                else col_sums<0, KF>(acc, q.c[b], rbase, cbase, lane, nullptr, false, dcol[b]);
            }
        }

#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) dcol[b][bj] += __shfl_xor(dcol[b][bj], 32, 64);
            if (wm == 1 && lane < 32) {
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) lx[b * kTile + cbase + bj * 32 + lane] = dcol[b][bj];
            }
        }
        __syncthreads();
        if (wm == 0 && lane < 32) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (b >= q.nb) continue;
                double* slot = p.slots + b * q.bstride + u * kTile;
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) slot[cbase + bj * 32 + lane] = dcol[b][bj] + lx[b * kTile + cbase + bj * 32 + lane];
            }
        }
    }
}

template <int NB>
constexpr size_t lds_unc_sweep() { return 2 * kOpBytes + 2 * kTile * 4 + NB * kTile * sizeof(double); }

// the sets of an uncertainty call as the reduction kernels see them (passed by value)
struct UncSets {
    int64_t n, TX;
    int S;
    int64_t blk[kad::kUncMaxSets + 1];         // first row block of each set in Z (blk[S] = TZ)
    int64_t m[kad::kUncMaxSets];
    int64_t yoff[kad::kUncMaxSets + 1];        // first row of each set in the concatenated per-row outputs
};

// v summed over the workgroup's 256 threads in a fixed order (all threads get it); `red` is 256 doubles of LDS
__device__ __forceinline__ double block_sum256(double v, double* red) {
    __syncthreads();                                                                  // red is free
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// One thread per column j of Z: its segments' unit slots summed in unit order, then
//   j = row i of X:        rxx[i] = sum_{j != i} k(x_i, x_j),  a[s * n + i] = rxx[i] / (n - 1) - sum_l k(x_i, y^s_l) / m_s
//   j = row l of set s:    ryy[l'] = sum_{l2 != l} k(y_l, y_l2),  ryx[l'] = sum_i k(x_i, y_l),  b[l'] = ryy / (m_s - 1) - ryx / n
// (l' = yoff[s] + l); padding columns write nothing.
__global__ void __launch_bounds__(256) kad_unc_rows_kernel(const double* __restrict__ slots, const int64_t* __restrict__ seg_start,
                                                           UncSets q, double* __restrict__ a, double* __restrict__ b,
                                                           double* __restrict__ rxx, double* __restrict__ ryy, double* __restrict__ ryx) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, J = j / kTile, c = j % kTile;
    if (J >= q.blk[q.S]) return;
    auto seg_sum = [&](int g) {
        const int64_t k = kad::unc_segment(J, g, q.TX, q.S);
        double s = 0.0;
        for (int64_t u = seg_start[k]; u < seg_start[k + 1]; ++u) s += slots[u * kTile + c];
        return s;
    };
    const double n = (double)q.n;
    if (J < q.TX) {
        if (j >= q.n) return;
        const double xx = seg_sum(0), mx = xx / (n - 1.0);
        rxx[j] = xx;
        for (int s = 0; s < q.S; ++s) a[s * q.n + j] = mx - seg_sum(s + 1) / (double)q.m[s];
    } else {
        int s = 0;
        while (J >= q.blk[s + 1]) ++s;
        const int64_t l = j - q.blk[s] * kTile;
        if (l >= q.m[s]) return;
        const double yy = seg_sum(s + 1), yx = seg_sum(0);
        const int64_t o = q.yoff[s] + l;
        ryy[o] = yy;
        ryx[o] = yx;
        b[o] = yy / ((double)q.m[s] - 1.0) - yx / n;
    }
}

// Workgroup s < S: stats[5 s ..] = mean a^s, mean b^s, sum (b^s - mean b^s)^2, sum ryy, sum ryx over set s.  Workgroup S:
// stats[5 S] = sum rxx.  Every sum in a fixed order.
__global__ void __launch_bounds__(256) kad_unc_sets_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                           const double* __restrict__ rxx, const double* __restrict__ ryy,
                                                           const double* __restrict__ ryx, UncSets q, double* __restrict__ stats) {
    __shared__ double red[256];
    const int s = blockIdx.x;
    if (s == q.S) {
        double v = 0.0;
        for (int64_t i = threadIdx.x; i < q.n; i += 256) v += rxx[i];
        v = block_sum256(v, red);
        if (threadIdx.x == 0) stats[5 * q.S] = v;
        return;
    }
    const int64_t m = q.m[s];
    const double* as = a + s * q.n;
    const double* bs = b + q.yoff[s];
    double va = 0.0, vb = 0.0, vyy = 0.0, vyx = 0.0;
    for (int64_t i = threadIdx.x; i < q.n; i += 256) va += as[i];
    for (int64_t l = threadIdx.x; l < m; l += 256) {
        vb += bs[l];
        vyy += ryy[q.yoff[s] + l];
        vyx += ryx[q.yoff[s] + l];
    }
    const double ma = block_sum256(va, red) / (double)q.n;
    const double mb = block_sum256(vb, red) / (double)m;
    const double syy = block_sum256(vyy, red), syx = block_sum256(vyx, red);
    double vv = 0.0;
    for (int64_t l = threadIdx.x; l < m; l += 256) {
        const double e = bs[l] - mb;
        vv += e * e;
    }
    vv = block_sum256(vv, red);
    if (threadIdx.x == 0) {
        stats[5 * s + 0] = ma;
        stats[5 * s + 1] = mb;
        stats[5 * s + 2] = vv;
        stats[5 * s + 3] = syy;
        stats[5 * s + 4] = syx;
    }
}

// Workgroup (w, y) of a fixed grid of W x ceil(S^2 / 256): the row tiles w, w + W, ... of 32 rows of X, and the pairs
// p = 256 y + thread: part[w][p = s S + t] = sum over its rows of (a^s_i - mean a^s)(a^t_i - mean a^t), rows in order.  s and t
// swapped multiply the same two values: the matrix comes out symmetric.
constexpr int kUncCovRows = 32;
__global__ void __launch_bounds__(256) kad_unc_cov_kernel(const double* __restrict__ a, const double* __restrict__ stats, UncSets q,
                                                          double* __restrict__ part) {
    __shared__ double la[kUncCovRows * kad::kUncMaxSets];
    const int S = q.S, P = S * S, p = blockIdx.y * 256 + threadIdx.x, s = p / S, u = p % S;
    double acc = 0.0;
    const int64_t tiles = (q.n + kUncCovRows - 1) / kUncCovRows;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        __syncthreads();                                                              // la is free
        for (int idx = threadIdx.x; idx < kUncCovRows * S; idx += 256) {
            const int r = idx % kUncCovRows, c = idx / kUncCovRows;
            const int64_t i = t * kUncCovRows + r;
            la[r * S + c] = i < q.n ? a[c * q.n + i] - stats[5 * c] : 0.0;
        }
        __syncthreads();
        if (p < P) {
#pragma unroll 8
            for (int r = 0; r < kUncCovRows; ++r) acc += la[r * S + s] * la[r * S + u];
        }
    }
    if (p < P) part[(int64_t)blockIdx.x * P + p] = acc;
}

// out[p] = the W partials of pair p summed in order
__global__ void __launch_bounds__(256) kad_unc_cov_sum_kernel(const double* __restrict__ part, int64_t W, int P, double* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int64_t w = 0; w < W; ++w) s += part[w * P + p];
    out[p] = s;
}

// ------------------------------------------------------------------------------------- KAD permutation test
// fad_kad_permutation_test's pass: Z's upper tile triangle once per permutation group (kad_perm_tiles.h), tile_mfma, then per wave its
// 64 x 64 part of the kernel tile as the A operand of a second product.  In the 32 x 32 accumulator layout lane (j, h) holds column j
// and rows (g & 3) + 8 (g >> 2) + 4 h in register g, so registers 8s .. 8s + 7 converted to f16 are k-step s of an A operand whose k
// index is the tile's row (cdna_hip_programming.md: "An accumulator tile as the next MFMA's operand"):
//   V^T[j, p] = sum_{i < j} k'_ij u_p(i),   k'_ij = f16(k_ij - c0) (0 below the diagonal of a diagonal tile)
// with B the labels of the tile's rows for 32 labellings p in the same permuted k order.  Labels enter as the f16 bit pattern 0x0400
// (2^-14) rather than 1.0, so a fragment is a shift and a mask of a prepared label word (kad_perm_rowbits_kernel); every product is
// scaled by the same power of two, undone in float64.  The output has the labelling on the lane and column j in the registers, so
// sum_j u_p(j) V^T[j, p] is a select against a wave-wide mask per register (the column words of kad_perm_colbits_kernel, loaded as
// scalars) and an add, into one float per lane per word.  float32 over one tile, float64 from there on; the lane halves and the waves
// meet once per workgroup at the launch's end, in a fixed order.  Padding rows and columns carry label 0, so their k - c0 = -c0
// never counts.
#define kConst __attribute__((address_space(4)))  // the constant address space: a uniform address there is a scalar load
constexpr uint32_t kLabelOne = 0x04000400u;    // a label pair of 1s as two f16 of 2^-14
constexpr double kLabelScale = 16384.0;        // 2^14

struct PermArgs {
    const char* z; const float* h;             // Z's image and -|row|^2 / 2 (-inf on the padding rows)
    int64_t pitch;
    int nchunks, nw;                           // nw: words of the launch's group
    float c, c0;                               // log2(e) / sigma^2 (1 / sigma^2 for iq and imq), the shift
    int64_t TZ, u0, cnt;                       // the triangle and the launch's tiles [u0, u0 + cnt)
    const uint32_t* rowbits;                   // the group's row words: [nw][NWZ][32] (kad_perm_rowbits_kernel)
    const uint32_t* colbits;                   // the group's column words: [nw][z_pad] (kad_perm_colbits_kernel)
    int64_t nwz, z_pad;
    double* slots;                             // the group's slots: [group slots][32 nw], added into
};

template <int DT, int KF>
__global__ void __launch_bounds__(kThreads, 2) kad_perm_kernel(PermArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, cbase = wn * 64, hh = lane >> 5, pl = lane & 31;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);
    double dq[kad::kPermWords];
#pragma unroll
    for (int w = 0; w < kad::kPermWords; ++w) dq[w] = 0.0;

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const kad::Tile t = kad::tri_tile(p.u0 + v, p.TZ);
        f32x16 acc[2][2];
        tile_mfma<DT>(p.z, p.z, p.h, p.h, p.pitch, p.nchunks, t.I, t.J, lds, [](int) {}, acc);

        // the A operands: k - c0 in f16, [bi][bj][k-step s]; a diagonal tile counts column > row only (tile_sum's mask)
        const bool diag = t.I == t.J;
        int lrow = rbase + 4 * hh - (cbase + pl);
        asm volatile("" : "+v"(lrow));                        // per tile, not hoisted out of the tile loop as lane masks (tile_sum)
        f16x8 af[2][2][2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    float e = kernel_value<KF>(acc[bi][bj][g], p.c) - p.c0;           // as tile_sum
                    if (diag) e = (bj * 32 - bi * 32 - (g & 3) - 8 * (g >> 2)) > lrow ? e : 0.f;
                    af[bi][bj][g >> 3][g & 7] = (_Float16)e;
                }

        // the second product, word by word: B from the row words of the wave's 64 rows, the masked column sum from the column words
        // The word strides, opaque per tile and the pointers advanced word by word: the 64 per-word offsets are not hoisted out of the
        // tile loop into SGPRs (spilled).
        const int64_t b0 = t.I * 4 + wm * 2;                                          // the wave's first 32-row word of Z
        int64_t rstride = p.z_pad, cstride = p.z_pad;                                 // [nwz][32] row words, z_pad column words
        int nw = p.nw;
        asm volatile("" : "+s"(rstride), "+s"(cstride), "+s"(nw));
        const uint32_t* rw = p.rowbits + b0 * 32 + pl;
        int64_t cb = t.J * kTile + cbase;                                             // uniform: scalar loads from the constant space
#pragma unroll
        for (int w = 0; w < kad::kPermWords; ++w, rw += rstride, cb += cstride) {
            if (w >= nw) continue;                                                    // uniform
            u32x4 bf[2][2];                                                           // [bi][s]
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) {
                const uint32_t th = rw[bi * 32] >> (8 * hh);
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int q = 0; q < 4; ++q) bf[bi][s][q] = (th << (10 - (4 * s + q))) & kLabelOne;
            }
            float sq = 0.f;
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                // opaque per (word, bj): the 32 column words are loaded here, not hoisted out of the loop as 2048 SGPRs (spilled)
                int64_t co = cb + bj * 32;
                asm volatile("" : "+s"(co));
                const kConst uint32_t* cw = (const kConst uint32_t*)p.colbits + co;
                f32x16 v2 = {};
#pragma unroll
                for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        v2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[bi][bj][s], __builtin_bit_cast(f16x8, bf[bi][s]), v2, 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int jl = (g & 3) + 8 * (g >> 2);
                    const uint64_t mask = (uint64_t)cw[jl] | (uint64_t)cw[jl + 4] << 32;     // lane half 0: column jl, half 1: jl + 4
                    sq += __builtin_amdgcn_inverse_ballot_w64(mask) ? v2[g] : 0.f;
                }
            }
            dq[w] += (double)sq;
        }
    }

    // a labelling: the two lane halves, then the four waves in order, into the workgroup's slot (LDS of the tiles is free after the barrier)
    double* lq = reinterpret_cast<double*>(lds);                                      // [4][32 kPermWords]
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kad::kPermWords; ++w) {
        if (w >= p.nw) continue;
        const double s = dq[w] + __shfl_xor(dq[w], 32, 64);
        if (lane < 32) lq[wave * 32 * kad::kPermWords + w * 32 + pl] = s;
    }
    __syncthreads();
    double* slot = p.slots + (int64_t)blockIdx.x * 32 * p.nw;                      // the group's slot w: launches add in order
    for (int i = tid; i < 32 * p.nw; i += kThreads) {
        const int o = 32 * kad::kPermWords;
        slot[i] += ((lq[i] + lq[o + i]) + lq[2 * o + i]) + lq[3 * o + i];
    }
}

constexpr size_t kLdsPerm = 2 * kOpBytes + 2 * kTile * 4;
static_assert(4 * 32 * kad::kPermWords * sizeof(double) <= kLdsPerm, "the slot reduction reuses the tiles' LDS");

// fad_kad_permutation_sweep's pass: kad_perm_kernel with NB pairs (c, c0).  One tile_mfma per tile; then bandwidth by
// bandwidth the A operands f16(k_b - c0_b) are built from the same accumulators as above and the word loop runs over that bandwidth's
// words, into row b of the lane's partials: dq[b * (kPermWords / NB) + w], the same kPermWords float64 values per lane.  At the end
// bandwidth b's partials meet as above and are added into b's own slots, slots[b * bstride + workgroup * 32 nw ..].  Bandwidth b
// therefore adds what kad_perm_kernel adds under (c[b], c0[b]), in the same order: the same bits wherever the two make the same launch
// cut.  Rows b >= nb of the kernel are idle (a uniform branch): a run of 3 bandwidths takes the kernel of 4.
template <int NB>
struct PermSweepArgs {
    PermArgs p;                                // p.c and p.c0 are not read; p.nw <= kPermWords / NB; p.slots: bandwidth 0's slots of the walk
    int nb;
    int64_t bstride;                           // doubles between two bandwidths' slots: the walk's slots x 32 nw
    float c[NB], c0[NB];
};

template <int DT, int KF, int NB>
__global__ void __launch_bounds__(kThreads, 2) kad_perm_sweep_kernel(PermSweepArgs<NB> q) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int NWB = kad::kPermWords / NB;                                         // words per bandwidth at most
    const PermArgs& p = q.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, cbase = wn * 64, hh = lane >> 5, pl = lane & 31;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);
    double dq[kad::kPermWords];
#pragma unroll
    for (int w = 0; w < kad::kPermWords; ++w) dq[w] = 0.0;

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const kad::Tile t = kad::tri_tile(p.u0 + v, p.TZ);
        f32x16 acc[2][2];
        tile_mfma<DT>(p.z, p.z, p.h, p.h, p.pitch, p.nchunks, t.I, t.J, lds, [](int) {}, acc);

        const bool diag = t.I == t.J;
        int lrow = rbase + 4 * hh - (cbase + pl);
        asm volatile("" : "+v"(lrow));                        // per tile, not hoisted out of the tile loop as lane masks (tile_sum)
        const int64_t b0 = t.I * 4 + wm * 2;                                          // the wave's first 32-row word of Z
        int nb = q.nb;
        asm volatile("" : "+s"(nb));                          // per tile: the NB tests b < nb are not kept as SGPR pairs around the tile loop
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b >= nb) continue;                                                    // uniform
            // the A operands of bandwidth b: k_b - c0_b in f16, [bi][bj][k-step s], as kad_perm_kernel builds them
            f16x8 af[2][2][2];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        float e = kernel_value<KF>(acc[bi][bj][g], q.c[b]) - q.c0[b];  // every read of the accumulator is kernel_value's
                        if (diag) e = (bj * 32 - bi * 32 - (g & 3) - 8 * (g >> 2)) > lrow ? e : 0.f;
                        af[bi][bj][g >> 3][g & 7] = (_Float16)e;
                    }

            // the word loop of kad_perm_kernel over this bandwidth's words (strides and offsets opaque, as there)
            int64_t rstride = p.z_pad, cstride = p.z_pad;
            int nw = p.nw;
            asm volatile("" : "+s"(rstride), "+s"(cstride), "+s"(nw));
            const uint32_t* rw = p.rowbits + b0 * 32 + pl;
            int64_t cb = t.J * kTile + cbase;
#pragma unroll
            for (int w = 0; w < NWB; ++w, rw += rstride, cb += cstride) {
                if (w >= nw) continue;                                                // uniform
                u32x4 bf[2][2];                                                       // [bi][s]
#pragma unroll
                for (int bi = 0; bi < 2; ++bi) {
                    const uint32_t th = rw[bi * 32] >> (8 * hh);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) bf[bi][s][qq] = (th << (10 - (4 * s + qq))) & kLabelOne;
                }
                float sq = 0.f;
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) {
                    int64_t co = cb + bj * 32;
                    asm volatile("" : "+s"(co));
                    const kConst uint32_t* cw = (const kConst uint32_t*)p.colbits + co;
                    f32x16 v2 = {};
#pragma unroll
                    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            v2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[bi][bj][s], __builtin_bit_cast(f16x8, bf[bi][s]), v2, 0, 0, 0);
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        const int jl = (g & 3) + 8 * (g >> 2);
                        const uint64_t mask = (uint64_t)cw[jl] | (uint64_t)cw[jl + 4] << 32;
                        sq += __builtin_amdgcn_inverse_ballot_w64(mask) ? v2[g] : 0.f;
                    }
                }
                dq[b * NWB + w] += (double)sq;
            }
        }
    }

    // a (bandwidth, labelling): the two lane halves, then the four waves in order, into the bandwidth's slot of the workgroup
    double* lq = reinterpret_cast<double*>(lds);                                      // [4][32 kPermWords]
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kad::kPermWords; ++i) {
        if ((i % NWB) >= p.nw || (i / NWB) >= q.nb) continue;
        const double s = dq[i] + __shfl_xor(dq[i], 32, 64);
        if (lane < 32) lq[wave * 32 * kad::kPermWords + i * 32 + pl] = s;
    }
    __syncthreads();
    for (int b = 0; b < q.nb; ++b) {
        double* slot = p.slots + b * q.bstride + (int64_t)blockIdx.x * 32 * p.nw;     // launches of a walk add in order
        const double* lb = lq + b * NWB * 32;
        for (int i = tid; i < 32 * p.nw; i += kThreads) {
            const int o = 32 * kad::kPermWords;
            slot[i] += ((lb[i] + lb[o + i]) + lb[2 * o + i]) + lb[3 * o + i];
        }
    }
}

// Row words: for labelling word w (labellings 32w .. 32w + 31), 32-row word b of Z and labelling 32w + l, the 32 labels of the rows of
// word b rearranged for the B fragments: pair k = 4s + q (k-step s, elements 2q, 2q + 1) of lane half h holds rows
// r = 16s + 8(q >> 1) + 4h + 2(q & 1) and r + 1; their labels go to bits k + 8h and 16 + k + 8h.  Labellings >= n_lab are all 0.
__global__ void __launch_bounds__(256) kad_perm_rowbits_kernel(const uint32_t* __restrict__ lab, int64_t n_lab, int64_t nwz, int64_t W,
                                                               uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= W * nwz * 32) return;
    const int64_t l = i % 32, b = (i / 32) % nwz, w = i / (32 * nwz), pz = 32 * w + l;
    const uint32_t x = pz < n_lab ? lab[pz * nwz + b] : 0u;
    uint32_t t = 0;
    for (int hh = 0; hh < 2; ++hh)
        for (int k = 0; k < 8; ++k) {
            const int s = k >> 2, q = k & 3, r = 16 * s + 8 * (q >> 1) + 4 * hh + 2 * (q & 1);
            t |= ((x >> r) & 1u) << (k + 8 * hh) | ((x >> (r + 1)) & 1u) << (16 + k + 8 * hh);
        }
    out[i] = t;
}

// Column words: out[w * z_pad + j] bit l = the label of row j of Z in labelling 32w + l.  One wave per (w, pair of 32-row words): lane
// (l, half) reads the word of labelling 32w + l, and one ballot per bit position transposes 64 rows.
__global__ void __launch_bounds__(256) kad_perm_colbits_kernel(const uint32_t* __restrict__ lab, int64_t n_lab, int64_t nwz, int64_t W,
                                                               uint32_t* __restrict__ out) {
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), npair = (nwz + 1) / 2;
    if (wv >= W * npair) return;                                                      // uniform over the wave
    const int lane = threadIdx.x & 63, l = lane & 31;
    const int64_t w = wv / npair, b = 2 * (wv % npair) + (lane >> 5), pz = 32 * w + l;
    const uint32_t x = (pz < n_lab && b < nwz) ? lab[pz * nwz + b] : 0u;
    uint32_t mine = 0;
    for (int r = 0; r < 32; ++r) {
        const uint64_t m = __ballot((x >> r) & 1u);
        if (l == r) mine = lane < 32 ? (uint32_t)m : (uint32_t)(m >> 32);
    }
    if (b < nwz) out[w * nwz * 32 + b * 32 + l] = mine;
}

// bad[0] += labellings 1 .. n_lab - 1 whose ones are not exactly n or that set a bit at or past N (integer atomics)
__global__ void __launch_bounds__(256) kad_perm_check_kernel(const uint32_t* __restrict__ lab, int64_t nwz, int64_t N, int64_t n,
                                                             unsigned long long* __restrict__ bad) {
    __shared__ long long red[256];
    const int64_t pz = 1 + blockIdx.x;
    long long ones = 0, stray = 0;
    for (int64_t b = threadIdx.x; b < nwz; b += 256) {
        const uint32_t x = lab[pz * nwz + b];
        const int64_t lo = 32 * b;
        const uint32_t valid = lo + 32 <= N ? 0xffffffffu : lo >= N ? 0u : (1u << (N - lo)) - 1u;
        ones += __popc(x & valid);
        stray += (x & ~valid) != 0;
    }
    red[threadIdx.x] = ones + (stray << 40);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0] != n) atomicAdd(bad, 1ull);
}

// r[j] = sum over j's column segment of the uncertainty pass's unit slots, in unit order (j < N; 0 on the padding rows)
__global__ void __launch_bounds__(256) kad_perm_rows_kernel(const double* __restrict__ slots, const int64_t* __restrict__ seg_start,
                                                            int64_t N, int64_t z_pad, double* __restrict__ r) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= z_pad) return;
    const int64_t J = j / kTile, c = j % kTile;
    double s = 0.0;
    if (j < N)
        for (int64_t u = seg_start[J]; u < seg_start[J + 1]; ++u) s += slots[u * kTile + c];
    r[j] = s;
}

// tot[0] = sum of r in a fixed order (one workgroup)
__global__ void __launch_bounds__(256) kad_perm_total_kernel(const double* __restrict__ r, int64_t N, double* __restrict__ tot) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < N; j += 256) s += r[j];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) tot[0] = s;
}

// the groups of a call as the statistics kernel sees them: first word, words and float64 slot offset of each group
struct PermGroup { int64_t w0, nw, slot_off, nslots; };

// One workgroup per labelling pz (0: the observed one): q = 2^15 * (its group's slots summed in order) + c0 n (n - 1), R = sum of r over its
// rows, then Sxx = q, Sxy = R - q, Syy = T - 2R + q and t.  Every sum in a fixed order.  obs[0 .. 2] = Sxx, Syy, Sxy of labelling 0.
__global__ void __launch_bounds__(256) kad_perm_stats_kernel(const double* __restrict__ slots, const PermGroup* __restrict__ groups, int ng,
                                                             const uint32_t* __restrict__ lab, int64_t nwz, const double* __restrict__ r,
                                                             const double* __restrict__ tot, double c0, int64_t n, int64_t m,
                                                             double* __restrict__ t_out, double* __restrict__ obs) {
    __shared__ double red[256];
    const int64_t pz = blockIdx.x, w = pz / 32;
    int g = 0;
    while (g + 1 < ng && groups[g + 1].w0 <= w) ++g;
    const PermGroup gr = groups[g];
    const int64_t width = 32 * gr.nw, li = pz - 32 * gr.w0;
    double sq = 0.0;
    for (int64_t s = threadIdx.x; s < gr.nslots; s += 256) sq += slots[gr.slot_off + s * width + li];
    sq = block_sum256(sq, red);
    double sr = 0.0;
    for (int64_t b = threadIdx.x; b < nwz; b += 256) {
        uint32_t x = lab[pz * nwz + b];
        while (x) {
            const int k = __ffs(x) - 1;
            sr += r[32 * b + k];
            x &= x - 1;
        }
    }
    sr = block_sum256(sr, red);
    if (threadIdx.x == 0) {
        const double nd = (double)n, md = (double)m, T = tot[0];
        const double q = 2.0 * kLabelScale * sq + c0 * nd * (nd - 1.0);
        const double sxx = q, sxy = sr - q, syy = T - 2.0 * sr + q;
        t_out[pz] = sxx / (nd * (nd - 1.0)) + syy / (md * (md - 1.0)) - 2.0 * sxy / (nd * md);
        if (pz == 0) { obs[0] = sxx; obs[1] = syy; obs[2] = sxy; }
    }
}

// ---------------------------------------------------------------------------------- precision, recall, density, coverage
// fad_prdc's passes: tile_mfma with two more epilogues, both on d^2 = max(-2 S', 0) as the median's histogram pass forms it.
//   radius: X x X (and Y x Y) over the full rectangle, per-column top-k.  A lane keeps the k smallest d^2 of each of its two columns in
//           registers (topk_insert); self is excluded by index on the diagonal tiles; padding rows give d^2 = +inf and never enter.  At
//           a unit's end the four lists of a column (two lane halves, two wm waves) merge into one list of k floats per (R, column)
//           slot; prdc_radius_reduce_kernel merges a column's NR slots into r^2.
//   cross:  X rows x Y columns, P1 = d^2 < r_X^2(i) (rows' radii staged in LDS by tile_mfma's row_lds hook) and P2 = d^2 < r_Y^2(j)
//           (the lane's column radii in registers).  Column counts of P1 per (R, column) slot, as kad_cols_kernel's sums; per row the
//           OR over columns of P2 (bit 0) and P1 (bit 1) by one ballot per accumulator element and integer atomics.
// Integers and float32 radii only: the same bits on every run.
constexpr int kMaxK = 16;

struct PrdcArgs {
    const char* a; const char* b;              // row operand, column operand (the same set in a radius pass)
    const float* ha; const float* hb;
    int64_t pitch;
    int nchunks, k;
    int64_t u0, cnt;                           // the launch's units [u0, u0 + cnt)
    int64_t TI, TJ, rr;                        // the unit map (kad::cross_unit)
    float* lists; int64_t list_pitch;          // radius: lists[(R * list_pitch + j) * k + q]
    const float* ra; const float* rb;          // cross: r^2 of the rows (0 on padding rows), of the columns
    int* counts; int64_t count_pitch;          // cross: counts[R * count_pitch + j]
    int* flags;                                // cross: per row of `a`, bit 0 recalled, bit 1 covered
};

// v into a lane's list t of the k smallest values seen (descending: t[0] is the k-th smallest; t[k .. 15] stay -inf):
// t[q] <- med3(t[q + 1], t[q], v) drops t[0] and puts v in its place in order; a v >= t[0] leaves the list as it is.  Fixed register
// indices, no scratch.
__device__ __forceinline__ void topk_insert(float (&t)[kMaxK], float v) {
#pragma unroll
    for (int q = 0; q < kMaxK - 1; ++q) t[q] = __builtin_amdgcn_fmed3f(t[q + 1], t[q], v);
    t[kMaxK - 1] = fminf(t[kMaxK - 1], v);
}

__device__ __forceinline__ void topk_init(float (&t)[kMaxK], int k) {
#pragma unroll
    for (int q = 0; q < kMaxK; ++q) t[q] = q < k ? INFINITY : -INFINITY;
}

// the wave's 64 rows of a tile into the lane's two column lists; DIAG: a tile I == J, where the pair of a row with itself is skipped
template <bool DIAG>
__device__ __forceinline__ void topk_tile(const f32x16 (&acc)[2][2], int rbase, int cbase, int lane, float (&t)[2][kMaxK]) {
    int lrow = rbase + 4 * (lane >> 5), lcol = cbase + (lane & 31);
    if (DIAG) asm volatile("" : "+v"(lrow), "+v"(lcol));         // per tile, not hoisted out of the tile loop as lane masks (tile_sum)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                float d2 = fmaxf(-2.f * acc[bi][bj][g], 0.f);
                if (DIAG) d2 = lcol + bj * 32 == lrow + bi * 32 + (g & 3) + 8 * (g >> 2) ? INFINITY : d2;
                if (__ballot(d2 < t[bj][0])) topk_insert(t[bj], d2);                   // wave-uniform skip
            }
}

template <int DT>
__global__ void __launch_bounds__(kThreads, 2) prdc_radius_kernel(PrdcArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* lx = reinterpret_cast<float*>(lds + 2 * kOpBytes + 2 * kTile * 4);       // the wm = 1 waves' lists of a unit [128][kMaxK]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, cbase = wn * 64;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = kad::cross_unit(u, p.TI, p.TJ, p.rr);
        float t[2][kMaxK];
        topk_init(t[0], p.k);
        topk_init(t[1], p.k);

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [](int) {}, acc);
            if (I == un.J) topk_tile<true>(acc, rbase, cbase, lane, t);
            else topk_tile<false>(acc, rbase, cbase, lane, t);
        }

        // a column: the two lane halves, then the wm = 0 and wm = 1 waves
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            float o[kMaxK];
#pragma unroll
            for (int q = 0; q < kMaxK; ++q) o[q] = __shfl_xor(t[bj][q], 32, 64);
#pragma unroll
            for (int q = 0; q < kMaxK; ++q) topk_insert(t[bj], q < p.k ? o[q] : INFINITY);
        }
        if (wm == 1 && lane < 32) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int q = 0; q < kMaxK; ++q) lx[(cbase + bj * 32 + lane) * kMaxK + q] = t[bj][q];
        }
        __syncthreads();
        if (wm == 0 && lane < 32) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                const int c = cbase + bj * 32 + lane;
#pragma unroll
                for (int q = 0; q < kMaxK; ++q) topk_insert(t[bj], q < p.k ? lx[c * kMaxK + q] : INFINITY);
                float* out = p.lists + ((u / p.TJ) * p.list_pitch + un.J * kTile + c) * p.k;
#pragma unroll
                for (int q = 0; q < kMaxK; ++q)
                    if (q < p.k) out[q] = t[bj][q];
            }
        }
    }
}

constexpr size_t kLdsRadius = 2 * kOpBytes + 2 * kTile * 4 + kTile * kMaxK * sizeof(float);

template <int DT>
__global__ void __launch_bounds__(kThreads, 2) prdc_cross_kernel(PrdcArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* lrad = reinterpret_cast<float*>(lds + 2 * kOpBytes + 2 * kTile * 4);     // r_X^2 of the tile's rows
    int* lcnt = reinterpret_cast<int*>(lds + 2 * kOpBytes + 3 * kTile * 4);         // the wm = 1 waves' column counts of a unit

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, cbase = wn * 64;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = kad::cross_unit(u, p.TI, p.TJ, p.rr);
        float ry[2];
        int cnt[2] = {0, 0};
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) ry[bj] = p.rb[un.J * kTile + cbase + bj * 32 + (lane & 31)];

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [&](int r) { lrad[r] = p.ra[I * kTile + r]; }, acc);

            int lrow = rbase + 4 * (lane >> 5);
            asm volatile("" : "+v"(lrow));                    // per tile, not hoisted out of the tile loop (tile_sum)
            // bit rl of the wave's rows rbase + rl: some column of the wave passes P1 (cov) / P2 (rec).  In the 32 x 32 layout the 32
            // columns of a row sit in one lane half, so a ballot's low and high words are the rows of lane halves 0 and 1.
            uint64_t cov = 0, rec = 0;
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 rx = *reinterpret_cast<const f32x4*>(lrad + lrow + bi * 32 + 8 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int g = 4 * q + e, rl = bi * 32 + e + 8 * q;
                        uint64_t b1 = 0, b2 = 0;
#pragma unroll
                        for (int bj = 0; bj < 2; ++bj) {
                            const float d2 = fmaxf(-2.f * acc[bi][bj][g], 0.f);
                            const bool p1 = d2 < rx[e], p2 = d2 < ry[bj];
                            cnt[bj] += p1;
                            b1 |= __ballot(p1);
                            b2 |= __ballot(p2);
                        }
                        cov |= (uint64_t)((uint32_t)b1 != 0) << rl | (uint64_t)((b1 >> 32) != 0) << (rl + 4);
                        rec |= (uint64_t)((uint32_t)b2 != 0) << rl | (uint64_t)((b2 >> 32) != 0) << (rl + 4);
                    }
                }
            if (cov | rec) {                                                          // uniform; lane l takes row rbase + l
                const int f = (int)((rec >> lane) & 1) | (int)((cov >> lane) & 1) << 1;
                if (f) atomicOr(&p.flags[I * kTile + rbase + lane], f);
            }
        }

#pragma unroll
        for (int bj = 0; bj < 2; ++bj) cnt[bj] += __shfl_xor(cnt[bj], 32, 64);
        if (wm == 1 && lane < 32) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) lcnt[cbase + bj * 32 + lane] = cnt[bj];
        }
        __syncthreads();
        if (wm == 0 && lane < 32) {
            int* slot = p.counts + (u / p.TJ) * p.count_pitch + un.J * kTile;
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) slot[cbase + bj * 32 + lane] = cnt[bj] + lcnt[cbase + bj * 32 + lane];
        }
    }
}

constexpr size_t kLdsCross = 2 * kOpBytes + 4 * kTile * 4;

// r2[j] = the k-th smallest of the NR lists of column j (j < n), 0 on the padding columns
__global__ void __launch_bounds__(256) prdc_radius_reduce_kernel(const float* __restrict__ lists, int64_t nr, int64_t pitch, int k, int64_t n,
                                                                 float* __restrict__ r2) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= pitch) return;
    if (j >= n) { r2[j] = 0.f; return; }
    float t[kMaxK];
    topk_init(t, k);
    for (int64_t R = 0; R < nr; ++R) {
        const float* l = lists + (R * pitch + j) * k;
#pragma unroll
        for (int q = 0; q < kMaxK; ++q) topk_insert(t, q < k ? l[q] : INFINITY);
    }
    r2[j] = t[0];
}

// balls[j] = column j's count slots summed (j < m)
__global__ void __launch_bounds__(256) prdc_balls_kernel(const int* __restrict__ counts, int64_t nr, int64_t pitch, int64_t m,
                                                         int* __restrict__ balls) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    int s = 0;
    for (int64_t R = 0; R < nr; ++R) s += counts[R * pitch + j];
    balls[j] = s;
}

// one workgroup: [0] columns with balls > 0, [1] the sum of balls, [2] rows with bit 0 (recalled), [3] rows with bit 1 (covered)
__global__ void __launch_bounds__(1024) prdc_stats_kernel(const int* __restrict__ balls, int64_t m, const int* __restrict__ flags, int64_t n,
                                                          unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[4][1024];
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int64_t j = threadIdx.x; j < m; j += 1024) {
        const int b = balls[j];
        s[0] += b > 0;
        s[1] += (unsigned long long)b;
    }
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int f = flags[i];
        s[2] += f & 1;
        s[3] += (f >> 1) & 1;
    }
    for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 4) out[threadIdx.x] = red[threadIdx.x][0];
}

// ------------------------------------------------------------------------------------ nearest baseline rows, authenticity
// fad_nearest's cross pass: X rows x Y columns on PRDC's cross map, tile_mfma with a per-column top-k of 64-bit keys
// (bits(d^2) << 32) | i, d^2 = max(-2 S', 0) with the sign bit cleared (the clamp may give -0.0), so that a key orders as (d^2, i) and
// the result is fully determined.  After each tile one v_permlane32_swap per pair of accumulator elements hands lane half h both row
// halves of column bj = h: a lane keeps ONE list (PRDC's two float lists' registers), and the row of every element is wave-uniform.
// The list (KB entries, KB >= k, a template bucket: 1, 4, 8, 16) is descending, t[0] the k-th smallest key, entries q >= k held at 0;
// a key enters by t[q] = max(t[q + 1], min(t[q], v)) (topk_insert's med3 on u64) behind topk_tile's wave-uniform skip, and KB = 1 is a
// plain u64 min.
// Padding rows give d^2 = +inf: their keys sort after every real row's and never reach an output (n >= k).  At a unit's end the wm = 1
// waves' lists merge into the wm = 0 waves' through LDS, one list of k keys per (row range R, column) slot; nearest_reduce_kernel
// merges a column's NR slots.  Integers and float32 bits only: the same result on every run.
template <int KB>
__device__ __forceinline__ void key_insert(uint64_t (&t)[KB], uint64_t v) {
#pragma unroll
    for (int q = 0; q < KB - 1; ++q) {
        const uint64_t lo = t[q] < v ? t[q] : v;
        t[q] = t[q + 1] > lo ? t[q + 1] : lo;
    }
    t[KB - 1] = t[KB - 1] < v ? t[KB - 1] : v;
}

template <int KB>
__device__ __forceinline__ void key_init(uint64_t (&t)[KB], int k) {
#pragma unroll
    for (int q = 0; q < KB; ++q) t[q] = q < k ? ~0ull : 0ull;
}

__device__ __forceinline__ uint64_t d2_key(float acc, uint32_t i) {
    const uint32_t b = __float_as_uint(fmaxf(-2.f * acc, 0.f)) & 0x7fffffffu;
    return (uint64_t)b << 32 | i;
}

template <int DT, int KB>
__global__ void __launch_bounds__(kThreads, 2) nearest_cross_kernel(PrdcArgs p, uint64_t* __restrict__ lists) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint64_t* lx = reinterpret_cast<uint64_t*>(lds + 2 * kOpBytes + 2 * kTile * 4);     // the wm = 1 waves' lists of a unit [128][KB]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, c = wn * 64 + (lane >> 5) * 32 + (lane & 31);          // the lane's column of the tile (after the swap)
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = kad::cross_unit(u, p.TI, p.TJ, p.rr);
        uint64_t t[KB];
        key_init(t, p.k);

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [](int) {}, acc);
            const uint32_t i0 = (uint32_t)(I * kTile + rbase);
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    // lanes 32..63 of column block 0 swap with lanes 0..31 of column block 1: lane half h then holds column bj = h at
                    // rows r (first) and r + 4 (second)
                    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[bi][0][g]), __float_as_uint(acc[bi][1][g]), false,
                                                                    false);
                    const uint32_t r = i0 + bi * 32 + (g & 3) + 8 * (g >> 2);
                    const uint64_t k0 = d2_key(__uint_as_float(s[0]), r), k1 = d2_key(__uint_as_float(s[1]), r + 4);
                    if constexpr (KB == 1) {
                        t[0] = k0 < t[0] ? k0 : t[0];
                        t[0] = k1 < t[0] ? k1 : t[0];
                    } else {
                        if (__ballot(k0 < t[0])) key_insert(t, k0);                  // wave-uniform skip
                        if (__ballot(k1 < t[0])) key_insert(t, k1);
                    }
                }
        }

        if (wm == 1) {
#pragma unroll
            for (int q = 0; q < KB; ++q) lx[c * KB + q] = t[q];
        }
        __syncthreads();
        if (wm == 0) {
#pragma unroll
            for (int q = 0; q < KB; ++q) key_insert(t, q < p.k ? lx[c * KB + q] : ~0ull);
            uint64_t* out = lists + ((u / p.TJ) * p.list_pitch + un.J * kTile + c) * p.k;
#pragma unroll
            for (int q = 0; q < KB; ++q)
                if (q < p.k) out[q] = t[q];
        }
    }
}

// fad_nn_test's self pass: nearest_cross_kernel's walk over Z x Z, every pooled row's k nearest OTHER pooled rows.  The
// same keys, list, LDS merge and slots.  On a tile I == J the accumulator of the pair row == column is set to -inf before the keys are
// formed (self_mask; self excluded by index, so a duplicate row is a neighbour at d^2 = 0): its d^2 = max(-2 S', 0) = +inf, the key of
// a padding row, which sorts after every real row's and never reaches an output (k <= N - 1).  Off-diagonal tiles pay nothing.  Masking
// the accumulators in place, ahead of one epilogue for all tiles, keeps KB = 1 at nearest_cross_kernel's 164 VGPRs; a second epilogue
// that replaced the self key itself took 208 (2 waves per SIMD instead of 3).
__device__ __forceinline__ void self_mask(f32x16 (&acc)[2][2], int rbase, int cbase, int lane) {
    int lrow = rbase + 4 * (lane >> 5), lcol = cbase + (lane & 31);
    asm volatile("" : "+v"(lrow), "+v"(lcol));                   // per tile, not hoisted out of the tile loop as lane masks (topk_tile)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int g = 0; g < 16; ++g)
                acc[bi][bj][g] = lcol + bj * 32 == lrow + bi * 32 + (g & 3) + 8 * (g >> 2) ? -INFINITY : acc[bi][bj][g];
}

// a tile's keys into the lane's list: nearest_cross_kernel's epilogue
template <int KB>
__device__ __forceinline__ void keys_tile(const f32x16 (&acc)[2][2], uint32_t i0, uint64_t (&t)[KB]) {
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            // lane half h holds column bj = h at rows r (first) and r + 4 (second)
            const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[bi][0][g]), __float_as_uint(acc[bi][1][g]), false, false);
            const uint32_t r = i0 + bi * 32 + (g & 3) + 8 * (g >> 2);
            const uint64_t k0 = d2_key(__uint_as_float(s[0]), r), k1 = d2_key(__uint_as_float(s[1]), r + 4);
            if constexpr (KB == 1) {
                t[0] = k0 < t[0] ? k0 : t[0];
                t[0] = k1 < t[0] ? k1 : t[0];
            } else {
                if (__ballot(k0 < t[0])) key_insert(t, k0);                          // wave-uniform skip
                if (__ballot(k1 < t[0])) key_insert(t, k1);
            }
        }
}

template <int DT, int KB>
__global__ void __launch_bounds__(kThreads, 2) nearest_self_kernel(PrdcArgs p, uint64_t* __restrict__ lists) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint64_t* lx = reinterpret_cast<uint64_t*>(lds + 2 * kOpBytes + 2 * kTile * 4);     // the wm = 1 waves' lists of a unit [128][KB]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int rbase = wm * 64, c = wn * 64 + (lane >> 5) * 32 + (lane & 31);          // the lane's column of the tile (after the swap)
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);

    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const int64_t u = p.u0 + v;
        const kad::Unit un = kad::cross_unit(u, p.TI, p.TJ, p.rr);
        uint64_t t[KB];
        key_init(t, p.k);

        for (int64_t I = un.I0; I < un.I1; ++I) {
            f32x16 acc[2][2];
            tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, I, un.J, lds, [](int) {}, acc);
            if (I == un.J) self_mask(acc, rbase, wn * 64, lane);                      // uniform over the workgroup
            keys_tile(acc, (uint32_t)(I * kTile + rbase), t);
        }

        if (wm == 1) {
#pragma unroll
            for (int q = 0; q < KB; ++q) lx[c * KB + q] = t[q];
        }
        __syncthreads();
        if (wm == 0) {
#pragma unroll
            for (int q = 0; q < KB; ++q) key_insert(t, q < p.k ? lx[c * KB + q] : ~0ull);
            uint64_t* out = lists + ((u / p.TJ) * p.list_pitch + un.J * kTile + c) * p.k;
#pragma unroll
            for (int q = 0; q < KB; ++q)
                if (q < p.k) out[q] = t[q];
        }
    }
}

template <int KB>
constexpr size_t lds_nearest() { return 2 * kOpBytes + 2 * kTile * 4 + kTile * KB * sizeof(uint64_t); }

// column j < m: the k smallest keys of its NR slots -> index[j * k + q], dist2[j * k + q] in ascending (d^2, i)
__global__ void __launch_bounds__(256) nearest_reduce_kernel(const uint64_t* __restrict__ lists, int64_t nr, int64_t pitch, int k, int64_t m,
                                                             int32_t* __restrict__ index, float* __restrict__ dist2) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    uint64_t t[kMaxK];
    key_init(t, k);
    for (int64_t R = 0; R < nr; ++R) {
        const uint64_t* l = lists + (R * pitch + j) * k;
#pragma unroll
        for (int q = 0; q < kMaxK; ++q) key_insert(t, q < k ? l[q] : ~0ull);
    }
#pragma unroll
    for (int q = 0; q < kMaxK; ++q)
        if (q < k) {
            index[j * k + (k - 1 - q)] = (int32_t)(uint32_t)t[q];
            dist2[j * k + (k - 1 - q)] = __uint_as_float((uint32_t)(t[q] >> 32));
        }
}

// authenticity: nn_r2[j] = r1^2 of y_j's nearest row, and the count of copied rows (d^2 <= r1^2, non-strict) added to *copied
__global__ void __launch_bounds__(256) nearest_copied_kernel(const int32_t* __restrict__ index, const float* __restrict__ dist2, int k,
                                                             int64_t m, const float* __restrict__ r2x, int64_t n,
                                                             float* __restrict__ nn_r2, unsigned long long* __restrict__ copied) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int hit = 0;
    if (j < m) {
        const int32_t i = index[j * k];
        const float r = i >= 0 && i < n ? r2x[i] : NAN;                              // always a row of x when n >= k
        nn_r2[j] = r;
        hit = dist2[j * k] <= r;
    }
    const int n_hit = __syncthreads_count(hit);
    if (threadIdx.x == 0 && n_hit) atomicAdd(copied, (unsigned long long)n_hit);     // integer counts: order does not matter
}

// ---------------------------------------------------------------------------- polynomial-kernel distance, KID
// k(a, b) = (gamma a.b + c0)^p is a function of the dot product, so the row markers take h's place: 0 on a row, -inf on a padding row
// (NaN on a row whose float32 squared norm is not finite, so that such a row can never pass for padding).  The accumulators then start
// at 0 + 0 and end at S = a.b exactly as the MFMAs form it, or at -inf where either row is padding.  Epilogue: u = fma(S, gamma, c0)
// -- the ordinary VALU op that reads the MFMA result, as kernel_value's -- k = u^p by a chain of p - 1 multiplies, and a pair whose
// S is -inf is dropped by a select: it adds exactly nothing.  A real pair's S is finite (|S| <= |a| |b|, both finite), so the marker
// cannot be taken for data.  p is uniform over the launch: one branch per tile, no instantiation per degree.
struct KidArgs {
    PassArgs p;                                // p.ha, p.hb: the row markers; p.c is not read.  Subsets: a = the x images, b = the y images
    float gamma, coef0;
    int degree;                                // 1 .. 4
    double* units;                             // subsets: one float64 per unit of the group
};

template <bool MASK, int P>
__device__ __forceinline__ float kid_tile_sum_p(const f32x16 (&acc)[2][2], float gamma, float coef0, int rbase, int cbase, int lane) {
    int lrow = rbase + 4 * (lane >> 5) - (cbase + (lane & 31));
    if (MASK) asm volatile("" : "+v"(lrow));                                         // as tile_sum: the mask compares stay in the tile
    float s = 0.f;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const float a = acc[bi][bj][g];
                const float u = fmaf(a, gamma, coef0);
                float k = u;
#pragma unroll
                for (int e = 1; e < P; ++e) k *= u;
                bool keep = a != -INFINITY;
                if (MASK) keep = keep && (bj * 32 - bi * 32 - (g & 3) - 8 * (g >> 2)) > lrow;     // column > row
                s += keep ? k : 0.f;
            }
    return s;
}

// (gamma S + c0)^degree summed over the wave's 64 x 64 pairs of a tile; MASK: a diagonal tile of a triangle counts only column > row
template <bool MASK>
__device__ __forceinline__ float kid_tile_sum(const f32x16 (&acc)[2][2], const KidArgs& q, int rbase, int cbase, int lane) {
    switch (q.degree) {
        case 1: return kid_tile_sum_p<MASK, 1>(acc, q.gamma, q.coef0, rbase, cbase, lane);
        case 2: return kid_tile_sum_p<MASK, 2>(acc, q.gamma, q.coef0, rbase, cbase, lane);
        case 3: return kid_tile_sum_p<MASK, 3>(acc, q.gamma, q.coef0, rbase, cbase, lane);
        default: return kid_tile_sum_p<MASK, 4>(acc, q.gamma, q.coef0, rbase, cbase, lane);
    }
}

// fad_kid's sum pass: kad_pass_kernel<DT, MODE_SUM> with the polynomial epilogue -- the same walk, slots and final sum.
template <int DT>
__global__ void __launch_bounds__(kThreads, 2) kid_pass_kernel(KidArgs q) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double* lred = reinterpret_cast<double*>(lds + 2 * kOpBytes + 2 * kTile * 4);
    const PassArgs& p = q.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);
    double dsum = 0.0;
    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const kad::Tile t = p.tri ? kad::tri_tile(p.u0 + v, p.tiles_j) : kad::rect_tile(p.u0 + v, p.tiles_j);
        f32x16 acc[2][2];
        tile_mfma<DT>(p.a, p.b, p.ha, p.hb, p.pitch, p.nchunks, t.I, t.J, lds, [](int) {}, acc);
        const float s = (p.tri && t.I == t.J) ? kid_tile_sum<true>(acc, q, wm * 64, wn * 64, lane) : kid_tile_sum<false>(acc, q, wm * 64, wn * 64, lane);
        dsum += (double)s;
    }
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off, 64);
    if (lane == 0) lred[wave] = dsum;
    __syncthreads();
    if (tid == 0) p.slots[blockIdx.x] = ((lred[0] + lred[1]) + lred[2]) + lred[3];
}

// table[u] = unit u of a group (kid::unit_of, kid_tiles.h) as the pass reads it: the first image row of its subset, its block and its
// tile.  The map's 64-bit divisions and the triangle's root are taken here, once per unit, not in the pass: inlined there they cost the
// pass 6 VGPRs and 88 spilled SGPRs, and with them the third workgroup per CU.
struct KidUnitRow { int64_t row0; int32_t block, I, J, pad; };
__global__ void __launch_bounds__(256) kid_unit_table_kernel(int64_t total, int64_t T, int64_t img_rows, KidUnitRow* __restrict__ table) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= total) return;
    const kid::Unit t = kid::unit_of(u, T);
    table[u] = KidUnitRow{t.q * img_rows, t.block, (int32_t)t.I, (int32_t)t.J, 0};
}

// fad_kid_subsets' pass over a group of subsets: unit p.u0 + v (kid_tiles.h) is one tile of one block of one subset and writes one
// float64, the tile's sum: the lanes' float32 sums in float64 through the wave's butterfly and ((w0 + w1) + w2) + w3.  A value depends
// on its tile alone -- not on the launch cut, the grid or the group.
template <int DT>
__global__ void __launch_bounds__(kThreads, 2) kid_units_kernel(KidArgs q, const KidUnitRow* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double* lred = reinterpret_cast<double*>(lds + 2 * kOpBytes + 2 * kTile * 4);
    const PassArgs& p = q.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int64_t G = gridDim.x, nslots = kad::launch_slots(p.cnt);
    for (int64_t L = blockIdx.x; L < nslots; L += G) {
        bool live;
        const int64_t v = kad::slot_tile(L, p.cnt, &live);
        if (!live) continue;                                                          // uniform over the workgroup
        const KidUnitRow t = table[p.u0 + v];
        const bool ay = t.block == kid::YY, bx = t.block == kid::XX;
        f32x16 acc[2][2];
        tile_mfma<DT>((ay ? p.b : p.a) + t.row0 * p.pitch, (bx ? p.a : p.b) + t.row0 * p.pitch, (ay ? p.hb : p.ha) + t.row0,
                      (bx ? p.ha : p.hb) + t.row0, p.pitch, p.nchunks, t.I, t.J, lds, [](int) {}, acc);
        const float s = (t.block != kid::XY && t.I == t.J) ? kid_tile_sum<true>(acc, q, wm * 64, wn * 64, lane)
                                                           : kid_tile_sum<false>(acc, q, wm * 64, wn * 64, lane);
        double dsum = (double)s;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off, 64);
        if (lane == 0) lred[wave] = dsum;                                             // read before the next tile's first barrier
        __syncthreads();
        if (tid == 0) q.units[p.u0 + v] = ((lred[0] + lred[1]) + lred[2]) + lred[3];
    }
}

// One wave per image row.  Image t (of n_img) holds s rows in img_rows: its row r is x[index[t * s + r]] (index NULL: x[r], a whole
// set), zero-padded to dp columns, the rows past s all zero.  mark: 0 on a row, -inf past s, NaN where the row's float32 squared norm
// is not finite.  The index was checked by kid_index_check_kernel before this kernel reads a row through it.
template <typename T>
__global__ void __launch_bounds__(256) kid_pack_kernel(const T* __restrict__ x, int64_t ld, int64_t d, const int32_t* __restrict__ index,
                                                       int64_t s, int64_t img_rows, int64_t n_img, T* __restrict__ out, int64_t dp,
                                                       float* __restrict__ mark) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n_img * img_rows) return;
    const int64_t t = row / img_rows, r = row % img_rows;
    const bool real = r < s;
    const int64_t src = real ? (index ? (int64_t)index[t * s + r] : r) : 0;
    float sq = 0.f;
    for (int64_t c = lane; c < dp; c += 64) {
        T v = T(0.f);
        if (real && c < d) v = x[src * ld + c];
        out[row * dp + c] = v;
        const float f = (float)v;
        sq = fmaf(f, f, sq);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if (lane == 0) mark[row] = real ? (isfinite(sq) ? 0.f : NAN) : -INFINITY;
}

// bad += the entries of ix outside [0, n) and of iy outside [0, m) (count entries each)
__global__ void __launch_bounds__(256) kid_index_check_kernel(const int32_t* __restrict__ ix, const int32_t* __restrict__ iy, int64_t count,
                                                              int64_t n, int64_t m, unsigned long long* __restrict__ bad) {
    int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const int64_t a = ix[i], b = iy[i];
        mine += (a < 0 || a >= n) + (b < 0 || b >= m);
    }
    __shared__ int red[256];
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicAdd(bad, (unsigned long long)red[0]);      // integer counts: order does not matter
}

// sums[(q0 + q) * 3 + block] = the units of block `block` of the group's subset q, summed in a fixed order (workgroup (q, block)):
// thread t takes the units t, t + 256, ... in unit order, then the tree of kad_slots_sum_kernel.
__global__ void __launch_bounds__(256) kid_subset_sums_kernel(const double* __restrict__ units, int64_t T, int64_t q0, double* __restrict__ sums) {
    __shared__ double red[256];
    const int64_t q = blockIdx.x, tt = kad::tri_tiles(T), U = kid::units_per_subset(T);
    const int block = blockIdx.y;
    const int64_t b = q * U + (block == kid::XX ? 0 : block == kid::YY ? tt : 2 * tt), e = q * U + (block == kid::XX ? tt : block == kid::YY ? 2 * tt : U);
    double s = 0.0;
    for (int64_t i = b + threadIdx.x; i < e; i += 256) s += units[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[(q0 + q) * 3 + block] = red[0];
}

// One workgroup.  Per subset q: the three means (the triangles' sums count every pair i != j twice) and MMD^2, as fad_kid forms them;
// then stats[0] = the mean of MMD^2 over q and stats[1] = its population standard deviation, two passes, each a strided float64 sum
// and the same tree: a fixed order.
__global__ void __launch_bounds__(256) kid_stats_kernel(const double* __restrict__ sums, int64_t nq, int64_t s, double* __restrict__ mmd2,
                                                        double* __restrict__ terms, double* __restrict__ stats) {
    __shared__ double red[256];
    const double pairs = (double)s * (double)(s - 1), square = (double)s * (double)s;
    double acc = 0.0;
    for (int64_t q = threadIdx.x; q < nq; q += 256) {
        const double kxx = 2.0 * sums[3 * q] / pairs, kyy = 2.0 * sums[3 * q + 1] / pairs, kxy = sums[3 * q + 2] / square;
        terms[3 * q] = kxx; terms[3 * q + 1] = kyy; terms[3 * q + 2] = kxy;
        const double v = kxx + kyy - 2.0 * kxy;
        mmd2[q] = v;
        acc += v;
    }
    double mean = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        const double total = red[0];
        __syncthreads();
        if (pass == 0) {
            mean = total / (double)nq;
            acc = 0.0;
            for (int64_t q = threadIdx.x; q < nq; q += 256) acc += (mmd2[q] - mean) * (mmd2[q] - mean);
        } else if (threadIdx.x == 0) {
            stats[0] = mean;
            stats[1] = sqrt(total / (double)nq);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct KadWorkspace {
    DevBuf raw[2], img[2], h[2], slots, small;       // small: info, pass offsets, pass sums, histograms
    DevBuf cross, band, songs;                       // fad_kad_individual: column slots of the two passes, song tables and outputs
    DevBuf lists, prdc;                              // fad_prdc: the radius passes' top-k slots; radii, counts, flags and totals
    DevBuf unc_slots, unc;                           // fad_kad_uncertainty: column slots of the pass; unit tables and per-row outputs
    DevBuf perm_lab, perm_rows, perm_cols, perm;     // fad_kad_permutation_test: labellings, row and column words; slots and tables
    DevBuf near;                                     // fad_nearest: index, dist2, radii, nn radii, copied count; fad_nn_test: index, dist2, counts
    DevBuf kid_index, kid;                           // fad_kid_subsets: the two index lists; the bad-index count, sums and results
    DevBuf sink_slots, sink;                         // fad_sinkhorn: the column states of a half-step; potentials and sums
    DevBuf sliced_theta, sliced;                     // fad_sliced_wasserstein, fad_sliced_individual: the directions' image; projections, sort scratch and sums
    DevBuf kmeans;                                   // fad_kmeans: the centroid operand, labels, dist2, the update's scratch (img[1]: the repeated rows)
    void release_all() {
        for (int i = 0; i < 2; ++i) { raw[i].release(); img[i].release(); h[i].release(); }
        slots.release(); small.release(); cross.release(); band.release(); songs.release(); lists.release(); prdc.release();
        unc_slots.release(); unc.release(); perm_lab.release(); perm_rows.release(); perm_cols.release(); perm.release();
        near.release(); kid_index.release(); kid.release(); sink_slots.release(); sink.release();
        sliced_theta.release(); sliced.release(); kmeans.release();
    }
};

struct Packed {
    const char* img; const float* h; int64_t n, pitch; int nchunks;
    double norm_sum;
};

static KadWorkspace& workspace(int device) {
    static thread_local PerThreadDevice<KadWorkspace> ws;
    return ws.get(device);
}

// What the helpers of one call share: the rows' dtype, the kernel family (FAD_KAD_GAUSSIAN where the entry has none), the device, the
// stream and this thread's workspace on the device.  A local of its entry, opened once the arguments are checked and never copied: it
// owns the guard that gives the caller's device back when the entry returns.
struct Ctx {
    int dtype = FAD_F32, kernel = FAD_KAD_GAUSSIAN, device = -1;
    hipStream_t st = nullptr;
    KadWorkspace* ws = nullptr;
    std::optional<DeviceGuard> guard;
    Ctx() = default;
    Ctx(const Ctx&) = delete;
    Ctx& operator=(const Ctx&) = delete;
    int open(int dtype_, int kernel_, int device_, void* stream) {
        FAD_TRY(check_device(device_));
        guard.emplace(device_);
        if (!guard->ok) return set_error(FAD_ERR_HIP, "hipSetDevice(%d) failed", device_);
        dtype = dtype_; kernel = kernel_; device = device_;
        st = static_cast<hipStream_t>(stream);
        ws = &workspace(device_);
        return FAD_OK;
    }
};

// The start of every public entry that plans passes: the launch budget of this call from FAD_KAD_LAUNCH_BUDGET (unset, empty,
// unparsable or <= 0: kad_tiles.h's 2^30 -- the variable exists for tests, which cut small passes into several launches with it), and
// an empty tally for fad_kad_last_plan.  Read per call, so a process may change the variable between two calls.
static void begin_entry() {
    const char* e = getenv("FAD_KAD_LAUNCH_BUDGET");
    char* end = nullptr;
    const long long v = e && *e ? strtoll(e, &end, 10) : 0;
    kad::set_launch_budget(end && *end == 0 ? (int64_t)v : 0);
    kad::reset_plan_tally();
}

static int64_t depth_elems(int64_t d, int dtype) {
    const int64_t per = kChunk / (int64_t)dtype_size(dtype);
    return cdiv(d, per) * per;
}

static int grid_cap(int device) { return std::max(8, (2 * num_cus(device)) & ~7); }

static int check_rows(const void* x, int64_t n, int64_t ld, int64_t d, int dtype, const char* what) {
    if (!x) return set_error(FAD_ERR_INVALID, "%s: NULL rows", what);
    if (dtype == FAD_F64) return set_error(FAD_ERR_INVALID, "%s: float64 rows are not supported; cast to float32 (or float16 / bfloat16)", what);
    if (dtype != FAD_F16 && dtype != FAD_BF16 && dtype != FAD_F32) return set_error(FAD_ERR_INVALID, "%s: unknown dtype %d", what, dtype);
    if (d < 1 || d > 2048) return set_error(FAD_ERR_INVALID, "%s: D = %lld is outside 1 .. 2048", what, (long long)d);
    if (ld < d) return set_error(FAD_ERR_INVALID, "%s: row pitch %lld < D = %lld", what, (long long)ld, (long long)d);
    if (n < 2) return set_error(FAD_ERR_TOO_FEW_ROWS, "%s: KAD needs at least 2 rows per set, got %lld", what, (long long)n);
    return FAD_OK;
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The regions of one workspace buffer: each starts on a 256-byte boundary, in the order they are added.  add<T>(count) before
// reserve(buffer), ptr(region) after it.
template <typename T> struct Region { size_t at; };
struct Carve {
    size_t size = 0;
    char* base = nullptr;
    template <typename T> Region<T> add(int64_t count) {
        const Region<T> r{size};
        size += align256((size_t)count * sizeof(T));
        return r;
    }
    int reserve(DevBuf& buf) {
        FAD_TRY(buf.reserve(size));
        base = static_cast<char*>(buf.p);
        return FAD_OK;
    }
    template <typename T> T* ptr(Region<T> r) const { return reinterpret_cast<T*>(base + r.at); }
};

// ws.small as every entry reserves it: 4096 doubles of places (info, offsets, sums, per-set info), then the two histograms
static int reserve_small(KadWorkspace& ws) { return ws.small.reserve(4096 * sizeof(double) + 2 * kHistBins * sizeof(unsigned long long)); }

// host rows -> ws.raw[slot] (reserved by the caller) from row `raw_row` on, at a pitch of d; device rows stay where they are
static int stage_rows(const Ctx& cx, int slot, int64_t raw_row, int on_device, const void** src, int64_t rn, int64_t* ld, int64_t d) {
    if (on_device) return FAD_OK;
    const size_t es = dtype_size(cx.dtype);
    char* raw = static_cast<char*>(cx.ws->raw[slot].p) + (size_t)(raw_row * d) * es;
    FAD_HIP_TRY(hipMemcpy2DAsync(raw, (size_t)d * es, *src, (size_t)*ld * es, (size_t)d * es, (size_t)rn, hipMemcpyHostToDevice, cx.st));
    *src = raw;
    *ld = d;
    return FAD_OK;
}

// rn rows of `src` -> r_pad rows of an image at `img` (depth dp, zero padding) and their h: the one launch site of kad_pack_kernel
static int pack_rows(const Ctx& cx, int slot, int64_t raw_row, int on_device, const void* src, int64_t rn, int64_t ld, int64_t d, void* img,
                     int64_t dp, int64_t r_pad, float* h) {
    FAD_TRY(stage_rows(cx, slot, raw_row, on_device, &src, rn, &ld, d));
    const dim3 grid((unsigned)cdiv(r_pad, 4));
    switch (cx.dtype) {
        case FAD_F16: kad_pack_kernel<_Float16><<<grid, 256, 0, cx.st>>>(static_cast<const _Float16*>(src), rn, ld, d, static_cast<_Float16*>(img), dp, r_pad, h); break;
        case FAD_BF16: kad_pack_kernel<__bf16><<<grid, 256, 0, cx.st>>>(static_cast<const __bf16*>(src), rn, ld, d, static_cast<__bf16*>(img), dp, r_pad, h); break;
        default: kad_pack_kernel<float><<<grid, 256, 0, cx.st>>>(static_cast<const float*>(src), rn, ld, d, static_cast<float*>(img), dp, r_pad, h); break;
    }
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// rows -> the set's padded image and h (no check of the norms)
static int pack_image(const Ctx& cx, int slot, const void* x, int64_t n, int64_t ld, int64_t d, int on_device, Packed* out) {
    KadWorkspace& ws = *cx.ws;
    const size_t es = dtype_size(cx.dtype);
    const int64_t dp = depth_elems(d, cx.dtype), n_pad = kad::blocks(n) * kTile;
    if (!on_device) FAD_TRY(ws.raw[slot].reserve((size_t)(n * d) * es));
    FAD_TRY(ws.img[slot].reserve((size_t)(n_pad * dp) * es));
    FAD_TRY(ws.h[slot].reserve((size_t)n_pad * sizeof(float)));
    FAD_TRY(reserve_small(ws));
    float* h = static_cast<float*>(ws.h[slot].p);
    FAD_TRY(pack_rows(cx, slot, 0, on_device, x, n, ld, d, ws.img[slot].p, dp, n_pad, h));
    *out = Packed{static_cast<const char*>(ws.img[slot].p), h, n, dp * (int64_t)es, (int)(dp * (int64_t)es / kChunk), 0.0};
    return FAD_OK;
}

// rows -> the set's padded image and h; reads back the norm sum and checks every norm is finite
static int pack_set(const Ctx& cx, int slot, const void* x, int64_t n, int64_t ld, int64_t d, int on_device, Packed* out) {
    FAD_TRY(pack_image(cx, slot, x, n, ld, d, on_device, out));
    double* info_d = static_cast<double*>(cx.ws->small.p) + 2 * slot;
    kad_norm_info_kernel<<<1, 256, 0, cx.st>>>(out->h, n, info_d);
    FAD_HIP_TRY(hipGetLastError());
    double info[2];
    FAD_HIP_TRY(hipMemcpyAsync(info, info_d, sizeof(info), hipMemcpyDeviceToHost, cx.st));
    FAD_HIP_TRY(hipStreamSynchronize(cx.st));
    if (info[1] != 0.0)
        return set_error(FAD_ERR_NOT_FINITE, "KAD: %lld of %lld rows have a NaN/Inf norm", (long long)info[1], (long long)n);
    out->norm_sum = info[0];
    return FAD_OK;
}

// Several sets in one image, Z (ws.img[0] and ws.h[0], z_pad rows): set i packed from image row r0 on, over r_pad rows (its own rows,
// then zero padding); host rows are staged one set after the other in ws.raw[0].  With set_info, kad_norm_info_kernel of set i follows
// its pack, into the per-set info of ws.small (doubles 1024 + 2 i).  *z: the whole image, n and norm_sum left to the caller.
struct RowSet { const void* src; int64_t rows, ld, r0, r_pad; };
static int pack_sets(const Ctx& cx, const RowSet* sets, int n_sets, int64_t d, int on_device, int64_t z_pad, bool set_info, Packed* z) {
    KadWorkspace& ws = *cx.ws;
    const size_t es = dtype_size(cx.dtype);
    const int64_t dp = depth_elems(d, cx.dtype), pitch = dp * (int64_t)es;
    int64_t total = 0;
    for (int i = 0; i < n_sets; ++i) total += sets[i].rows;
    FAD_TRY(ws.img[0].reserve((size_t)(z_pad * pitch)));
    FAD_TRY(ws.h[0].reserve((size_t)z_pad * sizeof(float)));
    FAD_TRY(reserve_small(ws));
    if (!on_device) FAD_TRY(ws.raw[0].reserve((size_t)(total * d) * es));
    char* zimg = static_cast<char*>(ws.img[0].p);
    float* zh = static_cast<float*>(ws.h[0].p);
    double* info_d = static_cast<double*>(ws.small.p) + 1024;
    int64_t staged = 0;
    for (int i = 0; i < n_sets; ++i) {
        const RowSet& s = sets[i];
        FAD_TRY(pack_rows(cx, 0, staged, on_device, s.src, s.rows, s.ld, d, zimg + s.r0 * pitch, dp, s.r_pad, zh + s.r0));
        staged += s.rows;
        if (set_info) {
            kad_norm_info_kernel<<<1, 256, 0, cx.st>>>(zh + s.r0, s.rows, info_d + 2 * i);
            FAD_HIP_TRY(hipGetLastError());
        }
    }
    *z = Packed{zimg, zh, 0, pitch, (int)(pitch / kChunk), 0.0};
    return FAD_OK;
}

// f(std::integral_constant<int, DT>{}) for the rows' dtype: the one place a pass's kernel instantiation is chosen
template <typename F>
static int with_dtype(int dtype, F&& f) {
    switch (dtype) {
        case FAD_F16: f(std::integral_constant<int, FAD_F16>{}); break;
        case FAD_BF16: f(std::integral_constant<int, FAD_BF16>{}); break;
        default: f(std::integral_constant<int, FAD_F32>{}); break;
    }
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// f(dt, std::integral_constant<int, KF>{}) for the rows' dtype and the kernel (one of FAD_KAD_*, checked by check_kernel)
template <typename F>
static int with_dtype_kernel(int dtype, int kernel, F&& f) {
    switch (kernel) {
        case FAD_KAD_IQ: return with_dtype(dtype, [&](auto dt) { f(dt, std::integral_constant<int, FAD_KAD_IQ>{}); });
        case FAD_KAD_IMQ: return with_dtype(dtype, [&](auto dt) { f(dt, std::integral_constant<int, FAD_KAD_IMQ>{}); });
        default: return with_dtype(dtype, [&](auto dt) { f(dt, std::integral_constant<int, FAD_KAD_GAUSSIAN>{}); });
    }
}

static int check_kernel(int kernel, const char* who) {
    if (kernel != FAD_KAD_GAUSSIAN && kernel != FAD_KAD_IQ && kernel != FAD_KAD_IMQ)
        return set_error(FAD_ERR_INVALID, "%s: unknown kernel %d (FAD_KAD_GAUSSIAN = 0, FAD_KAD_IQ = 1, FAD_KAD_IMQ = 2)", who, kernel);
    return FAD_OK;
}

// the rows of `a` against those of `b`, over the triangle (tri: b is a) or the rectangle; each launch sets u0 and cnt
static PassArgs pass_args(const Packed& a, const Packed& b, bool tri, float c) {
    PassArgs p{};
    p.a = a.img; p.b = b.img; p.ha = a.h; p.hb = b.h; p.pitch = a.pitch; p.n_a = a.n; p.n_b = b.n;
    p.tiles_j = kad::blocks(b.n); p.tri = tri; p.nchunks = a.nchunks; p.c = c;
    return p;
}

static std::vector<kad::Launch> pass_launches(const Ctx& cx, const PassArgs& p, bool hist) {
    const int64_t total = p.tri ? kad::tri_tiles(p.tiles_j) : kad::blocks(p.n_a) * p.tiles_j;
    return kad::launches(total, kad::tiles_per_launch(p.pitch / (int64_t)dtype_size(cx.dtype), cx.dtype == FAD_F32, hist), grid_cap(cx.device));
}

static int median_of_packed(const Ctx& cx, const Packed& x, double* sigma) {
    const hipStream_t st = cx.st;
    const int64_t P = x.n * (x.n - 1) / 2;
    PassArgs p = pass_args(x, x, true, 0.f);
    p.hist = reinterpret_cast<unsigned long long*>(static_cast<double*>(cx.ws->small.p) + 4096);
    const auto launches = pass_launches(cx, p, true);
    static const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
    uint64_t rank[2] = {(uint64_t)((P - 1) / 2), (uint64_t)(P / 2)};
    unsigned int pref[2] = {0, 0};
    std::vector<unsigned long long> hist(2 * kHistBins);
    for (int pass = 0; pass < 3; ++pass) {
        FAD_HIP_TRY(hipMemsetAsync(p.hist, 0, 2 * kHistBins * sizeof(unsigned long long), st));
        p.pref0 = pref[0]; p.pref1 = pref[1]; p.two = pref[0] != pref[1];
        p.lo_shift = shifts[pass]; p.bits = widths[pass]; p.hi_shift = shifts[pass] + widths[pass];
        for (const kad::Launch& l : launches) {
            p.u0 = l.u0; p.cnt = l.cnt;
            FAD_TRY(with_dtype(cx.dtype, [&](auto dt) { kad_pass_kernel<dt, MODE_HIST><<<(unsigned)l.grid, kThreads, kLdsHist, st>>>(p); }));
        }
        FAD_HIP_TRY(hipMemcpyAsync(hist.data(), p.hist, hist.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FAD_HIP_TRY(hipStreamSynchronize(st));
        const bool two = p.two;
        for (int t = 0; t < 2; ++t) {
            const unsigned long long* hh = hist.data() + (two && t == 1 ? kHistBins : 0);
            uint64_t below = 0;
            int bin = -1;
            for (int b = 0; b < (1 << widths[pass]); ++b) {
                if (below + hh[b] > rank[t]) { bin = b; break; }
                below += hh[b];
            }
            if (bin < 0) return set_error(FAD_ERR_HIP, "KAD median: rank %llu not found in pass %d (%llu counted)", (unsigned long long)rank[t], pass,
                                          (unsigned long long)below);
            rank[t] -= below;
            pref[t] = (pref[t] << widths[pass]) | (unsigned int)bin;
        }
    }
    float d2[2];
    memcpy(&d2[0], &pref[0], 4);
    memcpy(&d2[1], &pref[1], 4);
    *sigma = 0.5 * (std::sqrt((double)d2[0]) + std::sqrt((double)d2[1]));
    return FAD_OK;
}

// N sum passes into consecutive slot ranges, then sums_d[q] = pass q's slots summed in a fixed order (enqueued, not read back).
// launch(p, l) enqueues launch l of a pass with p's slots, u0 and cnt set: kad_pass_kernel for the KAD entries (kad_sum_passes),
// kid_pass_kernel for fad_kid, which so has the same launches, slots and sum.
template <int N, typename L>
static int sum_passes(const Ctx& cx, const PassArgs (&passes)[N], double* sums_d, L&& launch) {
    KadWorkspace& ws = *cx.ws;
    std::vector<kad::Launch> launches[N];
    int64_t off[N + 1] = {0};
    for (int q = 0; q < N; ++q) {
        launches[q] = pass_launches(cx, passes[q], false);
        off[q + 1] = off[q];
        for (const kad::Launch& l : launches[q]) off[q + 1] += l.grid;
    }
    FAD_TRY(ws.slots.reserve((size_t)off[N] * sizeof(double)));
    int64_t* off_d = reinterpret_cast<int64_t*>(static_cast<double*>(ws.small.p) + 8);
    FAD_HIP_TRY(hipMemcpyAsync(off_d, off, sizeof(off), hipMemcpyHostToDevice, cx.st));
    for (int q = 0; q < N; ++q) {
        PassArgs p = passes[q];
        p.slots = static_cast<double*>(ws.slots.p) + off[q];
        for (const kad::Launch& l : launches[q]) {
            p.u0 = l.u0; p.cnt = l.cnt;
            FAD_TRY(launch(p, l));
            p.slots += l.grid;
        }
    }
    kad_slots_sum_kernel<<<N, 256, 0, cx.st>>>(static_cast<const double*>(ws.slots.p), off_d, sums_d);
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// fad_kad runs XX, YY and XY; fad_kad_individual XX alone, so its Kxx comes from the same launches, slots and sum as fad_kad's.
template <int N>
static int kad_sum_passes(const Ctx& cx, const PassArgs (&passes)[N], double* sums_d) {
    return sum_passes(cx, passes, sums_d, [&](const PassArgs& p, const kad::Launch& l) {
        return with_dtype_kernel(cx.dtype, cx.kernel, [&](auto dt, auto kf) {
            kad_pass_kernel<dt, MODE_SUM, kf><<<(unsigned)l.grid, kThreads, kLdsSum, cx.st>>>(p);
        });
    });
}

// c = log2(e) / sigma^2 (1 / sigma^2 for iq and imq, whose epilogue takes t = c d^2 / 2 itself) as the kernels' float32: the one place a
// bandwidth becomes a kernel constant, for resolve_sigma and resolve_sigmas alike
enum SigmaCheck { SIGMA_OK = 0, SIGMA_NOT_POSITIVE = 1, SIGMA_OUTSIDE_F32 = 2 };
static SigmaCheck sigma_constant(double sigma, int kernel, float* c) {
    if (!(sigma > 0) || !std::isfinite(sigma)) return SIGMA_NOT_POSITIVE;
    const double cd = (kernel == FAD_KAD_GAUSSIAN ? 1.4426950408889634 : 1.0) / (sigma * sigma);
    if (!(cd > 0) || !std::isfinite(cd) || !std::isfinite((float)cd) || (float)cd == 0.f) return SIGMA_OUTSIDE_F32;
    *c = (float)cd;
    return SIGMA_OK;
}

// sigma = `bandwidth`, or the median pairwise distance of x when it is 0, and its c (sigma_constant)
static int resolve_sigma(const Ctx& cx, const Packed& x, double bandwidth, const char* who, double* sigma, float* c) {
    *sigma = bandwidth;
    if (!(*sigma > 0)) FAD_TRY(median_of_packed(cx, x, sigma));
    switch (sigma_constant(*sigma, cx.kernel, c)) {
        case SIGMA_NOT_POSITIVE:
            return set_error(FAD_ERR_INVALID, "%s: bandwidth %g (the median pairwise distance of the baseline when none is given) must be > 0"
                             " -- are all baseline rows identical?", who, *sigma);
        case SIGMA_OUTSIDE_F32:
            return set_error(FAD_ERR_INVALID, "%s: bandwidth %g is outside the float32 range of the kernel", who, *sigma);
        default: return FAD_OK;
    }
}

// A sweep's list of bandwidths, or of factors of the median (relative): every entry finite and > 0.  Checked before the device is opened.
static int check_bandwidths(const double* bandwidths, int n_bw, int relative, const char* who, bool pooled) {
    for (int b = 0; b < n_bw; ++b)
        if (!(bandwidths[b] > 0) || !std::isfinite(bandwidths[b]))
            return set_error(FAD_ERR_INVALID, "%s: %s %d is %g; every one must be finite and > 0 (the %s is the factor 1)", who,
                             relative ? "factor" : "bandwidth", b, bandwidths[b], pooled ? "pooled median" : "median");
    return FAD_OK;
}

// sigma[b] = bandwidths[b], or bandwidths[b] times the median pairwise distance of x (found once) when relative, and c[b] as
// sigma_constant forms it.  x is the baseline for fad_kad_sweep and the pooled rows for fad_kad_permutation_sweep.
static int resolve_sigmas(const Ctx& cx, const Packed& x, const double* bandwidths, int n_bw, int relative, const char* who, bool pooled,
                          double* sigma, float* c) {
    double median = 1.0;
    if (relative) {
        FAD_TRY(median_of_packed(cx, x, &median));
        if (!(median > 0) || !std::isfinite(median))
            return set_error(FAD_ERR_INVALID, "%s: the median pairwise distance of %s is %g; it must be > 0 -- are all %srows identical?", who,
                             pooled ? "the pooled rows" : "the baseline", median, pooled ? "" : "baseline ");
    }
    for (int b = 0; b < n_bw; ++b) {
        sigma[b] = relative ? bandwidths[b] * median : bandwidths[b];
        if (sigma_constant(sigma[b], cx.kernel, &c[b]) != SIGMA_OK)
            return set_error(FAD_ERR_INVALID, "%s: bandwidth %d (%g) is outside the float32 range of the kernel", who, b, sigma[b]);
    }
    return FAD_OK;
}

// The three sum passes for a group of g <= NB bandwidths (c[0 .. g), padded with c[g - 1]; the padded sums are dropped):
// sums[3 * b + q] = pass q's sum under c[b], read back.  Slots: pass q takes NB * G_q of them, G_q its launches' grids together,
// bandwidth b's at [NB * (G_0 + .. + G_{q-1}) + b * G_q, + G_q) -- within that range in fad_kad_k's order, launch after launch.  A
// launch's epilogue weighs NB single ones (kad_tiles.h), so a launch of 8 bandwidths is no longer than one of fad_kad_k.
template <int NB>
static int sweep_passes(const Ctx& cx, const PassArgs (&passes)[3], const float* c, int g, double* sums) {
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;
    const int dtype = cx.dtype;
    std::vector<kad::Launch> launches[3];
    int64_t G[3], off[3 * NB + 1];
    int64_t base = 0;
    for (int q = 0; q < 3; ++q) {
        const PassArgs& p = passes[q];
        const int64_t total = p.tri ? kad::tri_tiles(p.tiles_j) : kad::blocks(p.n_a) * p.tiles_j;
        const int64_t per = kad::tiles_per_launch_for(p.pitch / (int64_t)dtype_size(dtype), dtype == FAD_F32, kad::kSumEpilogue * NB);
        launches[q] = kad::launches(total, per, grid_cap(cx.device));
        G[q] = 0;
        for (const kad::Launch& l : launches[q]) G[q] += l.grid;
        for (int b = 0; b < NB; ++b) off[q * NB + b] = base + b * G[q];
        base += NB * G[q];
    }
    off[3 * NB] = base;
    FAD_TRY(ws.slots.reserve((size_t)base * sizeof(double)));
    // ws.small: the sweep's offset table [3 * 8 + 1] at double 32 and its sums [3 * 8] at double 64, clear of the single passes' places
    // (info 0 .. 3, offsets 8 .. 11, sums 16 .. 18), of the per-set info at 1024 and of the histograms at 4096
    int64_t* off_d = reinterpret_cast<int64_t*>(static_cast<double*>(ws.small.p) + 32);
    double* sums_d = static_cast<double*>(ws.small.p) + 64;
    static_assert(3 * kSweepGroup + 1 <= 32 && NB <= kSweepGroup, "the sweep's tables in ws.small");
    FAD_HIP_TRY(hipMemcpyAsync(off_d, off, sizeof(off), hipMemcpyHostToDevice, st));
    for (int q = 0; q < 3; ++q) {
        SweepArgs<NB> a;
        a.p = passes[q];
        a.stride = G[q];
        for (int b = 0; b < NB; ++b) a.c[b] = c[b < g ? b : g - 1];
        a.p.slots = static_cast<double*>(ws.slots.p) + off[q * NB];
        for (const kad::Launch& l : launches[q]) {
            a.p.u0 = l.u0; a.p.cnt = l.cnt;
            FAD_TRY(with_dtype_kernel(dtype, cx.kernel, [&](auto dt, auto kf) {
                kad_sweep_kernel<dt, kf, NB><<<(unsigned)l.grid, kThreads, lds_sweep<NB>(), st>>>(a);
            }));
            a.p.slots += l.grid;
        }
    }
    kad_slots_sum_kernel<<<3 * NB, 256, 0, st>>>(static_cast<const double*>(ws.slots.p), off_d, sums_d);
    FAD_HIP_TRY(hipGetLastError());
    double host[3 * NB];
    FAD_HIP_TRY(hipMemcpyAsync(host, sums_d, sizeof(host), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    for (int b = 0; b < g; ++b)
        for (int q = 0; q < 3; ++q) sums[3 * b + q] = host[q * NB + b];
    return FAD_OK;
}

// The three sum passes of KAD for the g <= kSweepGroup bandwidths c[0 .. g), read back: sums[3 * b + q] = pass q's sum under c[b].
// XX and YY over their triangles, XY over the rectangle with the larger set as the row operand.  One bandwidth runs fad_kad's own
// kernel, places and order (so fad_kad_sweep at a single bandwidth is fad_kad_k); 2 .. 4 and 5 .. 8 the sweep kernels of 4 and 8.
static int kad_three_passes(const Ctx& cx, const Packed& px, const Packed& py, const float* c, int g, double* sums) {
    const bool x_rows = px.n != py.n ? px.n > py.n : px.norm_sum >= py.norm_sum;
    const PassArgs passes[3] = {pass_args(px, px, true, c[0]), pass_args(py, py, true, c[0]),
                                pass_args(x_rows ? px : py, x_rows ? py : px, false, c[0])};
    if (g > 4) return sweep_passes<8>(cx, passes, c, g, sums);
    if (g > 1) return sweep_passes<4>(cx, passes, c, g, sums);
    double* sums_d = static_cast<double*>(cx.ws->small.p) + 16;
    FAD_TRY(kad_sum_passes(cx, passes, sums_d));
    FAD_HIP_TRY(hipMemcpyAsync(sums, sums_d, 3 * sizeof(double), hipMemcpyDeviceToHost, cx.st));
    FAD_HIP_TRY(hipStreamSynchronize(cx.st));
    return FAD_OK;
}

// The means and the estimate from the kernel sums over ordered pairs: sxx over the n (n - 1) pairs of x, syy likewise, sxy over n m
static void fill_result(fad_kad_result_t* r, double sxx, double syy, double sxy, int64_t n, int64_t m, double sigma) {
    r->kxx_mean = sxx / ((double)n * (double)(n - 1));
    r->kyy_mean = syy / ((double)m * (double)(m - 1));
    r->kxy_mean = sxy / ((double)n * (double)m);
    r->mmd2 = r->kxx_mean + r->kyy_mean - 2.0 * r->kxy_mean;
    r->bandwidth = sigma;
    r->n = n;
    r->m = m;
}

// A PRDC pass over the rectangle of `rows` x `cols` (fad_prdc): units of rr row blocks, NR row ranges, per-launch units
struct PrdcPlan { int64_t TI, TJ, rr, NR, per_launch; };
static PrdcPlan prdc_plan(const Ctx& cx, const Packed& rows, const Packed& cols, int64_t epilogue) {
    PrdcPlan q;
    const int64_t per = kad::tiles_per_launch_for(rows.pitch / (int64_t)dtype_size(cx.dtype), cx.dtype == FAD_F32, epilogue);
    q.TI = kad::blocks(rows.n); q.TJ = kad::blocks(cols.n);
    q.rr = kad::prdc_rows_per_unit(q.TI, q.TJ, per);
    q.NR = kad::cross_ranges(q.TI, q.rr);
    q.per_launch = kad::prdc_units_per_launch(q.rr, per);
    return q;
}

// r2[j] (TJ * 128 entries, 0 on the padding rows) = the k-th smallest d^2 from row j of x to the other rows of x
static int radius_pass(const Ctx& cx, const Packed& x, int k, float* lists, float* r2) {
    const PrdcPlan q = prdc_plan(cx, x, x, kad::kTopkEpilogue);
    PrdcArgs p{};
    p.a = p.b = x.img; p.ha = p.hb = x.h; p.pitch = x.pitch; p.nchunks = x.nchunks; p.k = k;
    p.TI = q.TI; p.TJ = q.TJ; p.rr = q.rr; p.lists = lists; p.list_pitch = q.TJ * kTile;
    for (const kad::Launch& l : kad::launches(q.NR * q.TJ, q.per_launch, grid_cap(cx.device))) {
        p.u0 = l.u0; p.cnt = l.cnt;
        FAD_TRY(with_dtype(cx.dtype, [&](auto dt) { prdc_radius_kernel<dt><<<(unsigned)l.grid, kThreads, kLdsRadius, cx.st>>>(p); }));
    }
    prdc_radius_reduce_kernel<<<(unsigned)cdiv(p.list_pitch, 256), 256, 0, cx.st>>>(lists, q.NR, p.list_pitch, k, x.n, r2);
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// f(std::integral_constant<int, KB>{}) for the list length the nearest kernels are instantiated at that holds k
template <typename F>
static void with_kb(int k, F&& f) {
    if (k == 1) f(std::integral_constant<int, 1>{});
    else if (k <= 4) f(std::integral_constant<int, 4>{});
    else if (k <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, kMaxK>{});
}

// index / dist2 [y.n x k] (device) = the k nearest rows of x to every row of y, ascending in (d^2, i); `lists` holds NR * TJ * 128 * k
// keys.  self: y is x (fad_nn_test's pooled rows) and the k nearest OTHER rows are wanted -- the same pass with the self pair masked.
static int nearest_pass(const Ctx& cx, const Packed& x, const Packed& y, bool self, int k, uint64_t* lists, int32_t* index, float* dist2) {
    const PrdcPlan q = prdc_plan(cx, x, y, kad::kNearestEpilogue);
    PrdcArgs p{};
    p.a = x.img; p.ha = x.h; p.b = y.img; p.hb = y.h; p.pitch = x.pitch; p.nchunks = x.nchunks; p.k = k;
    p.TI = q.TI; p.TJ = q.TJ; p.rr = q.rr; p.list_pitch = q.TJ * kTile;
    for (const kad::Launch& l : kad::launches(q.NR * q.TJ, q.per_launch, grid_cap(cx.device))) {
        p.u0 = l.u0; p.cnt = l.cnt;
        auto launch = [&](auto self_tag) {
            return with_dtype(cx.dtype, [&](auto dt) {
                with_kb(k, [&](auto kb) {
                    constexpr int DT = decltype(dt)::value, KB = decltype(kb)::value;
                    if constexpr (decltype(self_tag)::value)
                        nearest_self_kernel<DT, KB><<<(unsigned)l.grid, kThreads, lds_nearest<KB>(), cx.st>>>(p, lists);
                    else
                        nearest_cross_kernel<DT, KB><<<(unsigned)l.grid, kThreads, lds_nearest<KB>(), cx.st>>>(p, lists);
                });
            });
        };
        FAD_TRY(self ? launch(std::true_type{}) : launch(std::false_type{}));
    }
    nearest_reduce_kernel<<<(unsigned)cdiv(y.n, 256), 256, 0, cx.st>>>(lists, q.NR, p.list_pitch, k, y.n, index, dist2);
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// The argument checks, the pooled image with its labelling words, and nothing else, of fad_kad_permutation_test_k -- shared with
// fad_kad_permutation_sweep, which takes the same rows and labellings.
static int perm_check_args(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                           const uint32_t* labels, int64_t n_perm) {
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kad_permutation_test (x)"));
    FAD_TRY(check_rows(y, m, ldy, d, dtype, "fad_kad_permutation_test (y)"));
    if (n_perm < 1 || n_perm > kad::kPermMax)
        return set_error(FAD_ERR_INVALID, "fad_kad_permutation_test: %lld permutations (1 .. %lld)", (long long)n_perm, (long long)kad::kPermMax);
    if (!labels) return set_error(FAD_ERR_INVALID, "fad_kad_permutation_test: NULL labels");
    const int64_t N = n + m;
    if (N > INT32_MAX - kTile) return set_error(FAD_ERR_INVALID, "fad_kad_permutation_test: %lld rows in all (at most %d)", (long long)N, INT32_MAX - kTile);
    return FAD_OK;
}

// host labellings: every one with exactly n ones and no bit at or past N (device labellings are counted on the device)
static int perm_check_labels(int64_t n, int64_t m, const uint32_t* labels, int64_t n_perm, int labels_on_device,
                             const char* who = "fad_kad_permutation_test") {
    const int64_t N = n + m;
    const int64_t nwl = cdiv(N, 32);                                                   // words per labelling in the ABI
    if (!labels_on_device) {
        const uint32_t tail = N % 32 ? (1u << (N % 32)) - 1u : 0xffffffffu;
        for (int64_t q = 0; q < n_perm; ++q) {
            const uint32_t* row = labels + q * nwl;
            int64_t ones = 0;
            for (int64_t b = 0; b < nwl; ++b) ones += __builtin_popcount(row[b]);
            if (ones != n || (row[nwl - 1] & ~tail))
                return set_error(FAD_ERR_INVALID, "%s: labelling %lld has %lld ones%s; every labelling needs exactly n = %lld"
                                 " and no bit at or past N = %lld", who, (long long)q, (long long)ones, (row[nwl - 1] & ~tail) ? " and a bit past N" : "",
                                 (long long)n, (long long)N);
        }
    }
    return FAD_OK;
}

// Z's image and h, the labellings (the observed one first) and their row and column words, all on the device.  perm_prepare's two
// refusals name `who` and `family`: the KAD entries' by default, fad_sliced_permutation_test gives its own.
struct PermPrep {
    Packed z;                                                                          // the pooled rows, N of them
    int64_t n, m, N, TZ, z_pad, nwz, dp, NL, W;
    uint32_t* lab; uint32_t* rows_d; uint32_t* cols_d;
};

static int perm_prepare(const Ctx& cx, const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int on_device,
                        const uint32_t* labels, int64_t n_perm, int labels_on_device, PermPrep* out,
                        const char* who = "fad_kad_permutation_test", const char* family = "KAD") {
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;
    const int64_t N = n + m, nwl = cdiv(N, 32);
    const int64_t TZ = kad::blocks(N), z_pad = TZ * kTile, nwz = z_pad / 32;
    const int64_t NL = n_perm + 1, W = kad::perm_words(NL);                            // labellings with the observed one; their words
    // Z = [X; Y] in one image, contiguously: kad_pack_kernel at row 0 (n rows, no padding) and at row n (Y, then Z's padding rows)
    const RowSet sets[2] = {{x, n, ldx, 0, n}, {y, m, ldy, n, z_pad - n}};
    Packed z;
    FAD_TRY(pack_sets(cx, sets, 2, d, on_device, z_pad, false, &z));
    z.n = N;
    double* info_d = static_cast<double*>(ws.small.p) + 1024;                          // norm sum, non-finite rows, bad labellings
    unsigned long long* bad_d = reinterpret_cast<unsigned long long*>(info_d + 2);
    kad_norm_info_kernel<<<1, 256, 0, st>>>(z.h, N, info_d);
    FAD_HIP_TRY(hipGetLastError());

    // the labellings: the observed one (Z's first n rows), then the caller's, at a row pitch of nwz words (Z's padding rows are 0)
    FAD_TRY(ws.perm_lab.reserve((size_t)(NL * nwz) * sizeof(uint32_t)));
    uint32_t* lab = static_cast<uint32_t*>(ws.perm_lab.p);
    std::vector<uint32_t> obs_row((size_t)nwz, 0u);
    for (int64_t b = 0; b < n / 32; ++b) obs_row[(size_t)b] = 0xffffffffu;
    if (n % 32) obs_row[(size_t)(n / 32)] = (1u << (n % 32)) - 1u;
    FAD_HIP_TRY(hipMemsetAsync(lab, 0, (size_t)(NL * nwz) * sizeof(uint32_t), st));
    FAD_HIP_TRY(hipMemcpyAsync(lab, obs_row.data(), (size_t)nwz * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FAD_HIP_TRY(hipMemcpy2DAsync(lab + nwz, (size_t)nwz * sizeof(uint32_t), labels, (size_t)nwl * sizeof(uint32_t), (size_t)nwl * sizeof(uint32_t),
                                 (size_t)n_perm, labels_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    FAD_HIP_TRY(hipMemsetAsync(bad_d, 0, sizeof(unsigned long long), st));
    kad_perm_check_kernel<<<(unsigned)n_perm, 256, 0, st>>>(lab, nwz, N, n, bad_d);
    FAD_HIP_TRY(hipGetLastError());
    double info[2];
    unsigned long long bad = 0;
    FAD_HIP_TRY(hipMemcpyAsync(info, info_d, sizeof(info), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(&bad, bad_d, sizeof(bad), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (bad) return set_error(FAD_ERR_INVALID, "%s: %llu labellings do not have exactly n = %lld ones below N = %lld", who, bad,
                              (long long)n, (long long)N);
    if (info[1] != 0.0)
        return set_error(FAD_ERR_NOT_FINITE, "%s: %lld of %lld rows of x and y have a NaN/Inf norm", family, (long long)info[1], (long long)N);

    // the row and column words of every labelling word
    FAD_TRY(ws.perm_rows.reserve((size_t)(W * z_pad) * sizeof(uint32_t)));
    FAD_TRY(ws.perm_cols.reserve((size_t)(W * z_pad) * sizeof(uint32_t)));
    uint32_t* rows_d = static_cast<uint32_t*>(ws.perm_rows.p);
    uint32_t* cols_d = static_cast<uint32_t*>(ws.perm_cols.p);
    kad_perm_rowbits_kernel<<<(unsigned)cdiv(W * z_pad, 256), 256, 0, st>>>(lab, NL, nwz, W, rows_d);
    FAD_HIP_TRY(hipGetLastError());
    kad_perm_colbits_kernel<<<(unsigned)cdiv(W * cdiv(nwz, 2), 4), 256, 0, st>>>(lab, NL, nwz, W, cols_d);
    FAD_HIP_TRY(hipGetLastError());

    z.norm_sum = info[0];
    *out = PermPrep{z, n, m, N, TZ, z_pad, nwz, depth_elems(d, cx.dtype), NL, W, lab, rows_d, cols_d};
    return FAD_OK;
}

// The Z x Z column pass of the row sums: kad_unc_cols_kernel's walk over one pooled image whose sets start at the row blocks `blk`
// (kad_unc_tiles.h).  The plan adds its two tables to the entry's carve; once the carve is reserved, col_pass_args uploads them and
// gives the pass's arguments but for c, u0 and cnt: column slots in ws.unc_slots (reserved by the entry), one tile wide per unit.
struct ColPlan {
    int64_t rr, U;
    std::vector<kad::Unit> units;
    std::vector<int64_t> seg_start;
    Region<kad::Unit> units_r;
    Region<int64_t> seg_r;
};
static ColPlan col_plan(const Ctx& cx, const std::vector<int64_t>& blk, int64_t dp, Carve* cv) {
    ColPlan q;
    q.rr = kad::unc_rows_per_unit(kad::unc_tiles(blk), kad::tiles_per_launch_for(dp, cx.dtype == FAD_F32, kad::kUncEpilogue));
    kad::unc_units(blk, q.rr, &q.units, &q.seg_start);
    q.U = (int64_t)q.units.size();
    q.units_r = cv->add<kad::Unit>(q.U);
    q.seg_r = cv->add<int64_t>((int64_t)q.seg_start.size());
    return q;
}
static int col_pass_args(const Ctx& cx, const ColPlan& q, const Carve& cv, const Packed& z, ColArgs* p) {
    FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(q.units_r), q.units.data(), (size_t)q.U * sizeof(kad::Unit), hipMemcpyHostToDevice, cx.st));
    FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(q.seg_r), q.seg_start.data(), q.seg_start.size() * sizeof(int64_t), hipMemcpyHostToDevice, cx.st));
    *p = ColArgs{};
    p->a = p->b = z.img; p->ha = p->hb = z.h; p->pitch = z.pitch; p->nchunks = z.nchunks;
    p->units = cv.ptr(q.units_r); p->slots = static_cast<double*>(cx.ws->unc_slots.p); p->slot_pitch = kTile;
    return FAD_OK;
}

// The permutation test of the prepared rows under B bandwidths (sigma_b as c[b]): t [B][NL], labelling 0 the observed one, and the
// observed kernel sums obs [B][3], both read back.  fad_kad_permutation_sweep's body, and with B = 1 fad_kad_permutation_test_k's:
// one bandwidth is one run of kad_perm_kernel over perm_groups(W) word groups, the single test's groups, slots and launches
// (tests/native_cpu/kad_perm_sweep_cover.cpp).  fixed_shift: the shift of every bandwidth, in place of its own T / (N (N - 1)).
static int perm_run(const Ctx& cx, const PermPrep& pp, int B, const float* c, const float* fixed_shift, std::vector<double>* t, double* obs) {
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;
    const int dtype = cx.dtype, kernel = cx.kernel;
    const int64_t N = pp.N, TZ = pp.TZ, z_pad = pp.z_pad, nwz = pp.nwz, dp = pp.dp, NL = pp.NL;
    const bool f32 = dtype == FAD_F32;

    // the r pass's units do not depend on B: a unit's slot is one workgroup's, so r_b has the single call's bits at any size
    Carve cv;
    const ColPlan cp = col_plan(cx, kad::unc_blocks(N, nullptr, 0), dp, &cv);
    const int64_t rr = cp.rr, U = cp.U;

    // the walks of the permutation pass; per bandwidth its word groups as kad_perm_stats_kernel reads them: walk i holds its bandwidths'
    // slots one after the other, [nb][walk slots][32 nw]
    const std::vector<kad::PermSweepWalk> walks = kad::perm_sweep_walks(B, NL);
    std::vector<int64_t> wslots;
    const std::vector<kad::PermSweepLaunch> pl = kad::perm_sweep_launches(TZ, walks, dp, f32, grid_cap(cx.device), &wslots);
    int64_t ngmax = 1, nslot_doubles = 0;
    for (const kad::PermSweepWalk& w : walks) ngmax = std::max(ngmax, w.wgs);
    std::vector<PermGroup> groups((size_t)(B * ngmax));
    std::vector<int> ngs((size_t)B, 0);
    std::vector<int64_t> walk_off(walks.size());
    for (size_t i = 0; i < walks.size(); ++i) {
        const kad::PermSweepWalk& w = walks[i];
        walk_off[i] = nslot_doubles;
        const int64_t per_bw = wslots[i] * 32 * w.nw;
        for (int b = 0; b < w.nb; ++b) {
            groups[(size_t)((w.b0 + b) * ngmax + w.wg)] = PermGroup{w.w0, w.nw, nslot_doubles + b * per_bw, wslots[i]};
            ngs[(size_t)(w.b0 + b)] = (int)w.wgs;
        }
        nslot_doubles += w.nb * per_bw;
    }

    // units | seg_start | r [B][z_pad] | T [B] | groups [B][ngmax] | t [B][NL] | observed sums [B][3] | permutation slots
    const auto r_r = cv.add<double>(B * z_pad), tot_r = cv.add<double>(B);
    const auto groups_r = cv.add<PermGroup>((int64_t)groups.size());
    const auto t_r = cv.add<double>(B * NL), obs_r = cv.add<double>(3 * B), pslots_r = cv.add<double>(nslot_doubles);
    FAD_TRY(cv.reserve(ws.perm));
    const int rg = std::min(B, kad::kPermSweepNB);                                     // bandwidths per r pass at most
    FAD_TRY(ws.unc_slots.reserve((size_t)(rg * U * kTile) * sizeof(double)));
    int64_t* seg_d = cv.ptr(cp.seg_r);
    double* r_d = cv.ptr(r_r);
    double* tot_d = cv.ptr(tot_r);
    PermGroup* groups_d = cv.ptr(groups_r);
    double* t_d = cv.ptr(t_r);
    double* obs_d = cv.ptr(obs_r);
    double* pslots = cv.ptr(pslots_r);
    ColArgs ca;
    FAD_TRY(col_pass_args(cx, cp, cv, pp.z, &ca));
    FAD_HIP_TRY(hipMemcpyAsync(groups_d, groups.data(), groups.size() * sizeof(PermGroup), hipMemcpyHostToDevice, st));

    // r_b = K_b'1 and T_b = 1'r_b, up to kPermSweepNB bandwidths per walk over Z x Z; a launch of NB bandwidths weighs NB epilogues
    for (int b0 = 0; b0 < B; b0 += kad::kPermSweepNB) {
        const int nb = std::min(kad::kPermSweepNB, B - b0), knb = kad::perm_sweep_kernel_nb(nb);
        const int64_t per = std::max<int64_t>(1, kad::tiles_per_launch_for(dp, f32, kad::kUncEpilogue * knb) / rr);
        for (const kad::Launch& l : kad::launches(U, knb == 1 ? kad::unc_units_per_launch(rr, dp, f32) : per, grid_cap(cx.device))) {
            ca.u0 = l.u0; ca.cnt = l.cnt; ca.c = c[b0];
            auto sweep = [&](auto nbc) {
                constexpr int NB = decltype(nbc)::value;
                ColSweepArgs<NB> q;
                q.p = ca; q.nb = nb; q.bstride = U * kTile;
                for (int b = 0; b < NB; ++b) q.c[b] = c[b0 + std::min(b, nb - 1)];
                return with_dtype_kernel(dtype, kernel, [&](auto dt, auto kf) {
                    kad_unc_cols_sweep_kernel<dt, kf, NB><<<(unsigned)l.grid, kThreads, lds_unc_sweep<NB>(), st>>>(q);
                });
            };
            if (knb == 1) {
                FAD_TRY(with_dtype_kernel(dtype, kernel, [&](auto dt, auto kf) {
                    kad_unc_cols_kernel<dt, kf><<<(unsigned)l.grid, kThreads, kLdsUnc, st>>>(ca);
                }));
            } else if (knb == 2) {
                FAD_TRY(sweep(std::integral_constant<int, 2>{}));
            } else {
                FAD_TRY(sweep(std::integral_constant<int, 4>{}));
            }
        }
        for (int b = 0; b < nb; ++b) {
            kad_perm_rows_kernel<<<(unsigned)cdiv(z_pad, 256), 256, 0, st>>>(ca.slots + b * U * kTile, seg_d, N, z_pad, r_d + (b0 + b) * z_pad);
            FAD_HIP_TRY(hipGetLastError());
            kad_perm_total_kernel<<<1, 256, 0, st>>>(r_d + (b0 + b) * z_pad, N, tot_d + b0 + b);
            FAD_HIP_TRY(hipGetLastError());
        }
    }
    double T[FAD_KAD_PERM_MAX_BANDWIDTHS];
    FAD_HIP_TRY(hipMemcpyAsync(T, tot_d, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    // the shift of bandwidth b: the mean off-diagonal kernel value of Z under sigma_b, unless the caller fixes it.  Any constant gives
    // the same t; it sets how much of each kernel value f16 keeps.
    float c0[FAD_KAD_PERM_MAX_BANDWIDTHS];
    for (int b = 0; b < B; ++b) c0[b] = fixed_shift ? *fixed_shift : (float)(T[b] / ((double)N * (double)(N - 1)));

    FAD_HIP_TRY(hipMemsetAsync(pslots, 0, (size_t)nslot_doubles * sizeof(double), st));
    PermArgs pa{};
    pa.z = pp.z.img; pa.h = pp.z.h; pa.pitch = pp.z.pitch; pa.nchunks = pp.z.nchunks; pa.TZ = TZ; pa.nwz = nwz; pa.z_pad = z_pad;
    for (const kad::PermSweepLaunch& l : pl) {
        const kad::PermSweepWalk& w = walks[(size_t)l.walk];
        pa.nw = (int)w.nw; pa.u0 = l.u0; pa.cnt = l.cnt;
        pa.rowbits = pp.rows_d + w.w0 * z_pad;
        pa.colbits = pp.cols_d + w.w0 * z_pad;
        pa.slots = pslots + walk_off[(size_t)l.walk];
        pa.c = c[w.b0]; pa.c0 = c0[w.b0];
        auto sweep = [&](auto nbc) {
            constexpr int NB = decltype(nbc)::value;
            PermSweepArgs<NB> q;
            q.p = pa; q.nb = w.nb; q.bstride = wslots[(size_t)l.walk] * 32 * w.nw;
            for (int b = 0; b < NB; ++b) { q.c[b] = c[w.b0 + std::min(b, w.nb - 1)]; q.c0[b] = c0[w.b0 + std::min(b, w.nb - 1)]; }
            return with_dtype_kernel(dtype, kernel, [&](auto dt, auto kf) {
                kad_perm_sweep_kernel<dt, kf, NB><<<(unsigned)l.grid, kThreads, kLdsPerm, st>>>(q);
            });
        };
        if (w.kernel_nb == 1) {                // one bandwidth: fad_kad_permutation_test_k's own kernel and cut
            FAD_TRY(with_dtype_kernel(dtype, kernel, [&](auto dt, auto kf) {
                kad_perm_kernel<dt, kf><<<(unsigned)l.grid, kThreads, kLdsPerm, st>>>(pa);
            }));
        } else if (w.kernel_nb == 2) {
            FAD_TRY(sweep(std::integral_constant<int, 2>{}));
        } else {
            FAD_TRY(sweep(std::integral_constant<int, 4>{}));
        }
    }
    for (int b = 0; b < B; ++b) {
        kad_perm_stats_kernel<<<(unsigned)NL, 256, 0, st>>>(pslots, groups_d + b * ngmax, ngs[(size_t)b], pp.lab, nwz, r_d + b * z_pad, tot_d + b,
                                                            (double)c0[b], pp.n, pp.m, t_d + b * NL, obs_d + 3 * b);
        FAD_HIP_TRY(hipGetLastError());
    }
    t->resize((size_t)(B * NL));
    FAD_HIP_TRY(hipMemcpyAsync(t->data(), t_d, t->size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(obs, obs_d, (size_t)(3 * B) * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    return FAD_OK;
}

// ---------------------------------------------------------------------------------------- polynomial-kernel distance
struct KidParams { float gamma, coef0; int degree; };

// degree, gamma (<= 0: 1 / d) and coef0 as the kernels take them, in float32
static int kid_params(int degree, double gamma, double coef0, int64_t d, const char* who, KidParams* out) {
    if (degree < 1 || degree > 4) return set_error(FAD_ERR_INVALID, "%s: degree %d is outside 1 .. 4", who, degree);
    if (!std::isfinite(gamma) || !std::isfinite(coef0)) return set_error(FAD_ERR_INVALID, "%s: gamma %g and coef0 %g must be finite", who, gamma, coef0);
    const float g = gamma > 0 ? (float)gamma : (float)(1.0 / (double)d), c = (float)coef0;
    if (!std::isfinite(g) || !(g > 0.f) || !std::isfinite(c))
        return set_error(FAD_ERR_INVALID, "%s: gamma %g or coef0 %g is outside the float32 range", who, gamma, coef0);
    *out = KidParams{g, c, degree};
    return FAD_OK;
}

// n_img images of s rows each (img_rows with the padding) of the rows of x, through `index` (device) or, index NULL, x's own rows:
// slot's image and markers.  Host rows are staged whole, once, in ws.raw[slot] (*staged keeps the device copy for the next group).
static int kid_pack(const Ctx& cx, int slot, const void* x, int64_t n, int64_t ld, int64_t d, int on_device, const int32_t* index, int64_t s,
                    int64_t img_rows, int64_t n_img, const void** staged, Packed* out) {
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;
    const size_t es = dtype_size(cx.dtype);
    const int64_t dp = depth_elems(d, cx.dtype);
    if (!on_device) {
        if (!*staged) {
            FAD_TRY(ws.raw[slot].reserve((size_t)(n * d) * es));
            *staged = x;
            int64_t ld_staged = ld;
            FAD_TRY(stage_rows(cx, slot, 0, on_device, staged, n, &ld_staged, d));
        }
        x = *staged;
        ld = d;
    }
    const int64_t rows = n_img * img_rows;
    FAD_TRY(ws.img[slot].reserve((size_t)(rows * dp) * es));
    FAD_TRY(ws.h[slot].reserve((size_t)rows * sizeof(float)));
    float* h = static_cast<float*>(ws.h[slot].p);
    const dim3 grid((unsigned)cdiv(rows, 4));
    switch (cx.dtype) {
        case FAD_F16: kid_pack_kernel<_Float16><<<grid, 256, 0, st>>>(static_cast<const _Float16*>(x), ld, d, index, s, img_rows, n_img, static_cast<_Float16*>(ws.img[slot].p), dp, h); break;
        case FAD_BF16: kid_pack_kernel<__bf16><<<grid, 256, 0, st>>>(static_cast<const __bf16*>(x), ld, d, index, s, img_rows, n_img, static_cast<__bf16*>(ws.img[slot].p), dp, h); break;
        default: kid_pack_kernel<float><<<grid, 256, 0, st>>>(static_cast<const float*>(x), ld, d, index, s, img_rows, n_img, static_cast<float*>(ws.img[slot].p), dp, h); break;
    }
    FAD_HIP_TRY(hipGetLastError());
    *out = Packed{static_cast<const char*>(ws.img[slot].p), h, s, dp * (int64_t)es, (int)(dp * (int64_t)es / kChunk), 0.0};
    return FAD_OK;
}

static KidArgs kid_args(const PassArgs& p, const KidParams& k) {
    KidArgs q{};
    q.p = p; q.gamma = k.gamma; q.coef0 = k.coef0; q.degree = k.degree;
    return q;
}

// ------------------------------------------------------------------------------------------ Sinkhorn divergence
// One direction of one problem: the rows of `rows` reduced into every column of `cols`.  Planned once (one call of kad::launches, so one
// pass of fad_kad_last_plan's tally) and run at every iteration.
struct SoftminPlan {
    const Packed* rows; const Packed* cols;
    int64_t TI, TJ, rr, NR;
    std::vector<kad::Launch> launches;
};

static SoftminPlan softmin_plan(const Ctx& cx, const Packed& rows, const Packed& cols) {
    SoftminPlan q;
    q.rows = &rows; q.cols = &cols;
    q.TI = kad::blocks(rows.n); q.TJ = kad::blocks(cols.n);
    const int64_t per_launch = kad::tiles_per_launch_for(rows.pitch / (int64_t)dtype_size(cx.dtype), cx.dtype == FAD_F32, kad::kSoftminEpilogue);
    q.rr = kad::cross_rows_per_unit(q.TI, q.TJ, per_launch);
    q.NR = kad::cross_ranges(q.TI, q.rr);
    q.launches = kad::launches(q.NR * q.TJ, std::max<int64_t>(1, per_launch / q.rr), grid_cap(cx.device));
    return q;
}

// One half-step: pot[j] = -eps (LSE_i((p_i - C_ij) / eps) - log rows) for the columns j, hp_rows = h + p of the rows; hp_out (or NULL)
// gets h + pot of the columns.  Enqueued only.
static int softmin_pass(const Ctx& cx, const SoftminPlan& q, const float* hp_rows, float c, double eps, double* pot, float* hp_out) {
    const int64_t cols_pad = q.TJ * kTile;
    SoftminArgs p{};
    p.a = q.rows->img; p.b = q.cols->img; p.ha = hp_rows; p.hb = q.cols->h;
    p.pitch = q.rows->pitch; p.nchunks = q.rows->nchunks; p.c = c;
    p.TI = q.TI; p.TJ = q.TJ; p.rr = q.rr;
    p.slots = static_cast<float2*>(cx.ws->sink_slots.p); p.slot_pitch = cols_pad;
    for (const kad::Launch& l : q.launches) {
        p.u0 = l.u0; p.cnt = l.cnt;
        FAD_TRY(with_dtype(cx.dtype, [&](auto dt) { sinkhorn_cols_kernel<dt><<<(unsigned)l.grid, kThreads, kLdsSoftmin, cx.st>>>(p); }));
    }
    sinkhorn_reduce_kernel<<<(unsigned)cdiv(cols_pad, 256), 256, 0, cx.st>>>(p.slots, q.NR, cols_pad, q.cols->h, q.cols->n, cols_pad, (double)c,
                                                                             eps, eps * std::log((double)q.rows->n), pot, hp_out);
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// ------------------------------------------------------------------------------------- sliced Wasserstein distance
// A float32 direction entry rounded to the rows' dtype, round to nearest even, as the bits the image holds (16-bit dtypes: in the low
// half) and as the value they stand for.  Finite in; a float16 / bfloat16 result may be infinite (the caller refuses it through q).
static uint32_t round_direction(float f, int dtype, double* value) {
    uint32_t x;
    memcpy(&x, &f, 4);
    if (dtype == FAD_F32) { *value = (double)f; return x; }
    if (dtype == FAD_BF16) {
        const uint32_t h = (x + 0x7fffu + ((x >> 16) & 1u)) >> 16, back = h << 16;
        float v;
        memcpy(&v, &back, 4);
        *value = (double)v;
        return h;
    }
    const uint32_t sign = (x >> 16) & 0x8000u, mag = x & 0x7fffffffu;
    uint32_t h;
    if (mag < 0x38800000u) {                               // below 2^-14: a multiple of 2^-24, rounded by the float32 unit itself
        float a;
        memcpy(&a, &mag, 4);
        h = (uint32_t)std::nearbyint(a * 16777216.0f);     // exact product; nearbyint rounds to even; 1024 is the smallest normal
    } else {
        const uint32_t r = (mag + 0xfffu + ((mag >> 13) & 1u)) >> 13;
        h = r - (112u << 10);
        if (h > 0x7c00u) h = 0x7c00u;                      // 65520 and above round to infinity
    }
    const uint32_t e = h >> 10, man = h & 0x3ffu;
    float a;
    if (e == 0) {
        a = (float)man * 5.9604644775390625e-8f;           // 2^-24
    } else {
        const uint32_t back = e == 31 ? 0x7f800000u : ((e + 112u) << 23) | (man << 13);
        memcpy(&a, &back, 4);
    }
    *value = sign ? -(double)a : (double)a;
    return sign | h;
}

constexpr int64_t kSlicedWorkspace = (int64_t)1 << 30;     // bytes of chunked buffers by default (FAD_SLICED_WORKSPACE)
// a call's budget: FAD_SLICED_WORKSPACE where it is a whole number > 0, read per call
static int64_t sliced_budget() {
    const char* env = getenv("FAD_SLICED_WORKSPACE");
    char* end = nullptr;
    const long long v = env && *env ? strtoll(env, &end, 10) : 0;
    return end && *end == 0 && v > 0 ? (int64_t)v : kSlicedWorkspace;
}

struct SlicedPlan { int64_t chunks, lc, passes, share; };
static SlicedPlan& sliced_plan_value() {
    static thread_local SlicedPlan p{0, 0, 0, 0};
    return p;
}

// fad_sliced_individual_last_plan: chunks, directions per chunk, resident units per direction, songs on the long path, most songs in
// one unit, the resident capacity
struct SlicedSongPlan { int64_t v[6]; };
static SlicedSongPlan& sliced_song_plan_value() {
    static thread_local SlicedSongPlan p{{0, 0, 0, 0, 0, 0}};
    return p;
}

// What the three entries check alike, after their NULL rows and before their row counts, in this order.  ldy: the second set's pitch
// where the entry checks it here (NULL: fad_sliced_individual checks its songs' pitch later, with its own text).
static int sliced_check_args(const char* who, const float* directions, int dtype, int64_t d, int64_t ldx, const int64_t* ldy, int projections) {
    if (!directions) return set_error(FAD_ERR_INVALID, "%s: NULL directions", who);
    if (dtype == FAD_F64) return set_error(FAD_ERR_INVALID, "%s: float64 rows are not supported; cast to float32 (or float16 / bfloat16)", who);
    if (dtype != FAD_F16 && dtype != FAD_BF16 && dtype != FAD_F32) return set_error(FAD_ERR_INVALID, "%s: unknown dtype %d", who, dtype);
    if (d < 1 || d > 2048) return set_error(FAD_ERR_INVALID, "%s: D = %lld is outside 1 .. 2048", who, (long long)d);
    if (ldy && (ldx < d || *ldy < d))
        return set_error(FAD_ERR_INVALID, "%s: row pitch %lld / %lld < D = %lld", who, (long long)ldx, (long long)*ldy, (long long)d);
    if (ldx < d) return set_error(FAD_ERR_INVALID, "%s: row pitch %lld < D = %lld", who, (long long)ldx, (long long)d);
    if (projections < 1 || projections > 65536) return set_error(FAD_ERR_INVALID, "%s: %d projections, outside 1 .. 65536", who, projections);
    return FAD_OK;
}

// The directions rounded to the rows' dtype in their zero-padded image (l_img rows of the sets' pitch: kTile rows of zeros follow the
// last direction), and q_l from the rounded values in index order.  build makes no device call.
struct SlicedDirections {
    std::vector<char> timg;
    std::vector<double> q;
    int64_t l_img = 0;

    int build(const float* directions, int64_t L, int64_t d, int dtype, const char* who) {
        const size_t es = dtype_size(dtype);
        const int64_t tpitch = depth_elems(d, dtype) * (int64_t)es;
        l_img = (kad::blocks(L) + 1) * kTile;
        timg.assign((size_t)(l_img * tpitch), 0);
        q.resize((size_t)L);
        for (int64_t l = 0; l < L; ++l) {
            double ql = 0.0;
            for (int64_t c = 0; c < d; ++c) {
                const float f = directions[l * d + c];
                if (!std::isfinite(f)) return set_error(FAD_ERR_INVALID, "%s: direction %lld has an entry that is not finite", who, (long long)l);
                double v;
                const uint32_t bits = round_direction(f, dtype, &v);
                if (es == 2) {
                    const uint16_t h = (uint16_t)bits;
                    memcpy(&timg[(size_t)(l * tpitch + c * 2)], &h, 2);
                } else {
                    memcpy(&timg[(size_t)(l * tpitch + c * 4)], &bits, 4);
                }
                const double sq = v * v;
                ql += sq;
            }
            if (!(ql > 0) || !std::isfinite(ql))
                return set_error(FAD_ERR_INVALID, "%s: direction %lld, rounded to the rows' dtype, has the squared length %g", who, (long long)l, ql);
            q[(size_t)l] = ql;
        }
        return FAD_OK;
    }
    // the image into ws.sliced_theta, enqueued; *theta is its device address
    int upload(const Ctx& cx, const char** theta) const {
        FAD_TRY(cx.ws->sliced_theta.reserve(timg.size()));
        FAD_HIP_TRY(hipMemcpyAsync(cx.ws->sliced_theta.p, timg.data(), timg.size(), hipMemcpyHostToDevice, cx.st));
        *theta = static_cast<const char*>(cx.ws->sliced_theta.p);
        return FAD_OK;
    }
};

// The projections of one set's rows on lc directions from direction l0 on: the one place that fills ProjArgs.  Enqueued only.
static int sliced_project(const Ctx& cx, const Packed& set, const char* theta, const float* zeros, int64_t l0, int64_t lc, float* P,
                          int64_t ppitch, unsigned int* flag) {
    ProjArgs p{};
    p.th = theta + l0 * set.pitch; p.rows = set.img; p.zeros = zeros; p.pitch = set.pitch; p.nchunks = set.nchunks;
    p.TI = kad::blocks(lc); p.TJ = kad::blocks(set.n); p.lc = lc; p.n = set.n; p.P = P; p.ppitch = ppitch; p.flag = flag;
    const unsigned int grid = (unsigned int)std::min<int64_t>(p.TI * p.TJ, grid_cap(cx.device));
    return with_dtype(cx.dtype, [&](auto dt) { sliced_project_kernel<dt><<<grid, kThreads, kLdsProject, cx.st>>>(p); });
}

// the sort's buffers besides the keys: the second key buffer, counts and bases, and for the key-index sort the second
// index buffer
struct SlicedSortScratch { float* tmp; uint32_t* idx_tmp; uint32_t* counts; uint32_t* bases; };

// One set's side of a chunk: sliced_project, then the segmented sort -- keys only, or with `idx` the key-index sort that leaves the row
// of every rank in idx.  Enqueued only.
static int sliced_project_sort(const Ctx& cx, const Packed& set, const char* theta, const float* zeros, int64_t l0, int64_t lc, float* P,
                               int64_t ppitch, uint32_t* idx, const SlicedSortScratch& sc, unsigned int* flag) {
    FAD_TRY(sliced_project(cx, set, theta, zeros, l0, lc, P, ppitch, flag));
    if (idx) FAD_HIP_TRY(ssort::sort_segment_pairs(P, sc.tmp, idx, sc.idx_tmp, ppitch, set.n, lc, sc.counts, sc.bases, cx.st));
    else FAD_HIP_TRY(ssort::sort_segments(P, sc.tmp, ppitch, set.n, lc, sc.counts, sc.bases, cx.st));
    return FAD_OK;
}

// `cur` rows of n 4-byte words, at a pitch of `pad` words on the device, into the host staging array from its row l0 on; nothing where
// the array is empty (not asked for).  The sorted arrays are staged on the host: a refusal after the first chunk must leave the
// caller's arrays as they were.
template <typename T>
static int sliced_stage(std::vector<T>& host, int64_t l0, int64_t n, const void* dev, int64_t pad, int64_t cur, hipStream_t st) {
    static_assert(sizeof(T) == 4, "projections and ranks are 4-byte words");
    if (host.empty()) return FAD_OK;
    FAD_HIP_TRY(hipMemcpy2DAsync(host.data() + l0 * n, (size_t)n * 4, dev, (size_t)pad * 4, (size_t)n * 4, (size_t)cur, hipMemcpyDeviceToHost, st));
    return FAD_OK;
}

// W_l = S[l * stride] / (nm q_l), one division, into W [L]; mean, spread and maximum over l in index order
struct SlicedStats { double mean, std_error, best; int64_t best_l; };
static SlicedStats sliced_stats(const double* S, int64_t stride, double nm, const std::vector<double>& q, double* W) {
    const int64_t L = (int64_t)q.size();
    double sum = 0.0, best = -INFINITY;
    int64_t best_l = 0;
    for (int64_t l = 0; l < L; ++l) {
        const double w = S[l * stride] / (nm * q[(size_t)l]);
        W[l] = w;
        sum += w;
        if (w > best) { best = w; best_l = l; }
    }
    const double mean = sum / (double)L;
    double dev2 = 0.0;
    for (int64_t l = 0; l < L; ++l) {
        const double dv = W[l] - mean;
        const double sq = dv * dv;
        dev2 += sq;
    }
    return SlicedStats{mean, L > 1 ? std::sqrt(dev2 / (double)(L - 1)) / std::sqrt((double)L) : (double)NAN, best, best_l};
}

// What a call over the two whole sets writes besides the result: fad_sliced_wasserstein's detail and, with `shares`,
// fad_sliced_shares' per-row arrays.  All host; every pointer but the two shares may be NULL.
struct SlicedOut {
    double* values; float* sorted_x; float* sorted_y;
    bool shares;
    double* share_x; double* share_y; int32_t* index_x; int32_t* index_y;
};

// fad_sliced_wasserstein and fad_sliced_shares: one body.  Without o.shares the launches are the keys-only sort and
// sliced_match_kernel<false>; with it the key-index sort, sliced_match_kernel<true>, the other side's cost kernel and the per-row sums
// -- and the same slots, S_l and statistics either way.
static int sliced_sets(const char* who, const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                       int on_device, const float* directions, int projections, fad_sliced_result_t* out, const SlicedOut& o, int device,
                       void* stream) {
    if (!x || !y) return set_error(FAD_ERR_INVALID, "%s: NULL rows", who);
    FAD_TRY(sliced_check_args(who, directions, dtype, d, ldx, &ldy, projections));
    if (n < 1 || m < 1) return set_error(FAD_ERR_TOO_FEW_ROWS, "%s: needs at least 1 row per set, got %lld and %lld", who, (long long)n, (long long)m);
    if (n > INT32_MAX - kTile || m > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "%s: %lld and %lld rows (at most %d per set)", who, (long long)n, (long long)m, INT32_MAX - kTile);
    if (n > (((int64_t)1 << 53) - 1) / m)
        return set_error(FAD_ERR_INVALID, "%s: n m = %lld x %lld is 2^53 or more: the integer weights would not be exact in float64", who,
                         (long long)n, (long long)m);
    const int64_t L = projections;
    SlicedDirections dirs;                                     // before any device call
    FAD_TRY(dirs.build(directions, L, d, dtype, who));
    const int64_t budget = sliced_budget();

    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    const hipStream_t st = cx.st;
    Packed px, py;                                             // each set packed once, its norms checked finite
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    FAD_TRY(pack_set(cx, 1, y, m, ldy, d, on_device, &py));
    const char* theta;
    FAD_TRY(dirs.upload(cx, &theta));

    // the chunk: lc directions' projections of both sets, the sort's second buffer, its counts, the match's slots; with shares also
    // the rows at every rank of both sets, the index sort's second buffer and a float64 cost per row of both sets
    const bool x_larger = n >= m, sh = o.shares;
    const int64_t n_pad = kad::blocks(n) * kTile, m_pad = kad::blocks(m) * kTile, t_pad = std::max(n_pad, m_pad);
    const int64_t na = x_larger ? n : m, nb = x_larger ? m : n, nblk = cdiv(na, kMatchBlock), jblk = cdiv(nb, kMatchBlock);
    const int64_t count_words = std::max(ssort::counts_elems(n, 1), ssort::counts_elems(m, 1));
    const int64_t per_dir = 4 * (n_pad + m_pad + t_pad) + 4 * (count_words + ssort::kRadix) + 8 * nblk +
                            (sh ? 4 * (n_pad + m_pad + t_pad) + 8 * (n_pad + m_pad) : 0);
    const int64_t lc = std::max<int64_t>(1, std::min<int64_t>(L, budget / per_dir));
    Carve cv;
    const auto px_r = cv.add<float>(lc * n_pad), py_r = cv.add<float>(lc * m_pad), tmp_r = cv.add<float>(lc * t_pad);
    const auto counts_r = cv.add<uint32_t>(lc * count_words), bases_r = cv.add<uint32_t>(lc * ssort::kRadix);
    const auto slots_r = cv.add<double>(lc * nblk), s_r = cv.add<double>(L);
    const auto zeros_r = cv.add<float>(std::max(t_pad, dirs.l_img));
    const auto flag_r = cv.add<unsigned int>(64);
    const auto ix_r = cv.add<uint32_t>(sh ? lc * n_pad : 0), iy_r = cv.add<uint32_t>(sh ? lc * m_pad : 0);
    const auto itmp_r = cv.add<uint32_t>(sh ? lc * t_pad : 0);
    const auto cx_r = cv.add<double>(sh ? lc * n_pad : 0), cy_r = cv.add<double>(sh ? lc * m_pad : 0);
    const auto den_r = cv.add<double>(sh ? L : 0), acc_r = cv.add<double>(sh ? n + m : 0);
    FAD_TRY(cv.reserve(cx.ws->sliced));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(zeros_r), 0, (size_t)std::max(t_pad, dirs.l_img) * sizeof(float), st));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(flag_r), 0, 64 * sizeof(unsigned int), st));
    const ssort::Plan sp = ssort::plan(n, lc);
    sliced_plan_value() = SlicedPlan{cdiv(L, lc), lc, ssort::kPasses, sp.G > 1 ? -sp.G : sp.W};

    // W_l's denominator (double)(n m) q_l: the per-row costs are divided by it on the device, S_l on the host below
    const double nm = (double)(n * m);
    std::vector<double> den(sh ? (size_t)L : 0);               // lives until the stream is synchronised below
    if (sh) {
        for (int64_t l = 0; l < L; ++l) den[(size_t)l] = nm * dirs.q[(size_t)l];
        FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(den_r), den.data(), (size_t)L * sizeof(double), hipMemcpyHostToDevice, st));
        FAD_HIP_TRY(hipMemsetAsync(cv.ptr(acc_r), 0, (size_t)(n + m) * sizeof(double), st));
    }

    std::vector<float> sx(o.sorted_x ? (size_t)(L * n) : 0), sy(o.sorted_y ? (size_t)(L * m) : 0);
    std::vector<int32_t> hx(o.index_x ? (size_t)(L * n) : 0), hy(o.index_y ? (size_t)(L * m) : 0);
    float* Px = cv.ptr(px_r);
    float* Py = cv.ptr(py_r);
    uint32_t* Ix = cv.ptr(ix_r);
    uint32_t* Iy = cv.ptr(iy_r);
    double* acc_x = cv.ptr(acc_r);
    double* acc_y = acc_x + n;
    const SlicedSortScratch sc{cv.ptr(tmp_r), cv.ptr(itmp_r), cv.ptr(counts_r), cv.ptr(bases_r)};
    const float* A = x_larger ? Px : Py;
    const float* B = x_larger ? Py : Px;
    const int64_t a_pad = x_larger ? n_pad : m_pad, b_pad = x_larger ? m_pad : n_pad;
    for (int64_t l0 = 0; l0 < L; l0 += lc) {
        const int64_t cur = std::min(lc, L - l0);
        FAD_TRY(sliced_project_sort(cx, px, theta, cv.ptr(zeros_r), l0, cur, Px, n_pad, sh ? Ix : nullptr, sc, cv.ptr(flag_r)));
        FAD_TRY(sliced_project_sort(cx, py, theta, cv.ptr(zeros_r), l0, cur, Py, m_pad, sh ? Iy : nullptr, sc, cv.ptr(flag_r)));
        if (sh) {
            sliced_match_kernel<true><<<(unsigned int)(cur * nblk), kMatchBlock, 0, st>>>(A, x_larger ? Ix : Iy, a_pad, na, B, b_pad, nb, nblk,
                                                                                          cv.ptr(den_r) + l0, cv.ptr(slots_r),
                                                                                          cv.ptr(x_larger ? cx_r : cy_r));
            FAD_HIP_TRY(hipGetLastError());
            sliced_other_cost_kernel<<<(unsigned int)(cur * jblk), kMatchBlock, 0, st>>>(A, a_pad, na, B, x_larger ? Iy : Ix, b_pad, nb, jblk,
                                                                                         cv.ptr(den_r) + l0, cv.ptr(x_larger ? cy_r : cx_r));
            FAD_HIP_TRY(hipGetLastError());
            sliced_share_sum_kernel<<<(unsigned int)cdiv(n, 256), 256, 0, st>>>(cv.ptr(cx_r), n_pad, n, cur, acc_x);
            sliced_share_sum_kernel<<<(unsigned int)cdiv(m, 256), 256, 0, st>>>(cv.ptr(cy_r), m_pad, m, cur, acc_y);
        } else {
            sliced_match_kernel<false><<<(unsigned int)(cur * nblk), kMatchBlock, 0, st>>>(A, nullptr, a_pad, na, B, b_pad, nb, nblk, nullptr,
                                                                                           cv.ptr(slots_r), nullptr);
        }
        FAD_HIP_TRY(hipGetLastError());
        sliced_finish_kernel<<<(unsigned int)cdiv(cur, 256), 256, 0, st>>>(cv.ptr(slots_r), nblk, cur, cv.ptr(s_r) + l0);
        FAD_HIP_TRY(hipGetLastError());
        FAD_TRY(sliced_stage(sx, l0, n, Px, n_pad, cur, st));
        FAD_TRY(sliced_stage(sy, l0, m, Py, m_pad, cur, st));
        FAD_TRY(sliced_stage(hx, l0, n, Ix, n_pad, cur, st));
        FAD_TRY(sliced_stage(hy, l0, m, Iy, m_pad, cur, st));
    }
    std::vector<double> S((size_t)L), acc(sh ? (size_t)(n + m) : 0);
    unsigned int flag = 0;
    FAD_HIP_TRY(hipMemcpyAsync(S.data(), cv.ptr(s_r), (size_t)L * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(&flag, cv.ptr(flag_r), sizeof(flag), hipMemcpyDeviceToHost, st));
    if (sh) FAD_HIP_TRY(hipMemcpyAsync(acc.data(), acc_x, (size_t)(n + m) * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (flag) return set_error(FAD_ERR_NOT_FINITE, "%s: a projection is not finite in float32", who);

    std::vector<double> W((size_t)L);
    const SlicedStats t = sliced_stats(S.data(), 1, nm, dirs.q, W.data());
    out->sw2_squared = t.mean; out->std_error = t.std_error;
    out->max_sliced = t.best; out->max_index = t.best_l;
    out->n = n; out->m = m; out->projections = projections;
    if (o.values) memcpy(o.values, W.data(), (size_t)L * sizeof(double));
    if (o.sorted_x) memcpy(o.sorted_x, sx.data(), sx.size() * sizeof(float));
    if (o.sorted_y) memcpy(o.sorted_y, sy.data(), sy.size() * sizeof(float));
    if (o.index_x) memcpy(o.index_x, hx.data(), hx.size() * sizeof(int32_t));
    if (o.index_y) memcpy(o.index_y, hy.data(), hy.size() * sizeof(int32_t));
    if (sh) {                                                  // share = (the running sum over l) / L
        for (int64_t i = 0; i < n; ++i) o.share_x[i] = acc[(size_t)i] / (double)L;
        for (int64_t j = 0; j < m; ++j) o.share_y[j] = acc[(size_t)(n + j)] / (double)L;
    }
    return FAD_OK;
}

// ------------------------------------------------------------------------------- sliced Wasserstein permutation test
// fad_sliced_permutation_last_plan: sort chunks, directions per sort chunk, pair rounds in all, directions per round, labelling words
// per round, the sort's share (as fad_sliced_last_plan reports it, of the pooled rows)
struct SlicedPermPlan { int64_t v[6]; };
static SlicedPermPlan& sliced_perm_plan_value() {
    static thread_local SlicedPermPlan p{{0, 0, 0, 0, 0, 0}};
    return p;
}

// fad_sliced_permutation_test's detail.  All host; every pointer may be NULL.
struct SlicedPermOut { double* values; float* sorted_z; int32_t* index_z; };

// fad_sliced_permutation_test.  The pooled rows are projected and sorted once per direction, with the row at every rank
// (sliced_project_sort's key-index form); the sorted keys and the rows never see a label.  A round takes some directions of the sort
// chunk and some labelling words: ssplit's stable split gives every (direction, labelling) pair of the round its two sorted groups,
// and sliced_match_kernel<false> and sliced_finish_kernel run over the pairs as if they were the directions of a chunk -- the larger
// group leads, the label-1 group at n == m, as x leads in sliced_sets.  S [L][NL] stays on the device until every round has run.
static int sliced_permutation(const char* who, const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d,
                              int dtype, int on_device, const float* directions, int projections, const uint32_t* labels, int64_t n_perm,
                              int labels_on_device, fad_sliced_permutation_result_t* out, double* null_out, double* null_max,
                              const SlicedPermOut& o, int device, void* stream) {
    if (!x || !y) return set_error(FAD_ERR_INVALID, "%s: NULL rows", who);
    FAD_TRY(sliced_check_args(who, directions, dtype, d, ldx, &ldy, projections));
    if (n < 1 || m < 1) return set_error(FAD_ERR_TOO_FEW_ROWS, "%s: needs at least 1 row per set, got %lld and %lld", who, (long long)n, (long long)m);
    const int64_t N = n + m, L = projections, NL = n_perm + 1;
    if (n > INT32_MAX - kTile || m > INT32_MAX - kTile || N > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "%s: %lld rows in all (at most %d)", who, (long long)N, INT32_MAX - kTile);
    if (n > (((int64_t)1 << 53) - 1) / m)
        return set_error(FAD_ERR_INVALID, "%s: n m = %lld x %lld is 2^53 or more: the integer weights would not be exact in float64", who,
                         (long long)n, (long long)m);
    if (n_perm < 1 || n_perm > kad::kPermMax)
        return set_error(FAD_ERR_INVALID, "%s: %lld permutations (1 .. %lld)", who, (long long)n_perm, (long long)kad::kPermMax);
    if (!labels) return set_error(FAD_ERR_INVALID, "%s: NULL labels", who);
    SlicedDirections dirs;                                     // before any device call
    FAD_TRY(dirs.build(directions, L, d, dtype, who));
    FAD_TRY(perm_check_labels(n, m, labels, n_perm, labels_on_device, who));
    const int64_t budget = sliced_budget();

    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    const hipStream_t st = cx.st;
    PermPrep pp;                                               // Z packed once, its norms and the labellings checked; rows_d is not read
    FAD_TRY(perm_prepare(cx, x, n, ldx, y, m, ldy, d, on_device, labels, n_perm, labels_on_device, &pp, who, who));
    const char* theta;
    FAD_TRY(dirs.upload(cx, &theta));

    // the sort chunk: lc directions' pooled keys and rows, their second buffers, the sort's counts -- a quarter of the budget.  The
    // round: dr directions x wr labelling words, 32 pairs a word, each pair its two groups, its match slots and the split's counts.
    const bool one_leads = n >= m;
    const int64_t z_pad = pp.z_pad, W = pp.W, n_pad = kad::blocks(n) * kTile, m_pad = kad::blocks(m) * kTile;
    const int64_t na = one_leads ? n : m, nb = one_leads ? m : n, nblk = cdiv(na, kMatchBlock), G = ssplit::groups(N);
    const int64_t count_words = ssort::counts_elems(N, 1);
    const int64_t per_dir = 16 * z_pad + 4 * (count_words + ssort::kRadix);
    const int64_t lc = std::max<int64_t>(1, std::min<int64_t>(L, budget / 4 / per_dir));
    const int64_t per_word = 32 * (4 * (n_pad + m_pad) + 8 * nblk + 4 * G + 8);
    const int64_t most = (int64_t)INT32_MAX / (32 * std::max(nblk, G));                // words a launch's grid can hold
    const int64_t units = std::max<int64_t>(1, std::min(most, (budget - budget / 4) / per_word));
    const int64_t wr = std::min(W, units), dr = units >= W ? std::min(lc, units / W) : 1;
    Carve cv;
    const auto k_r = cv.add<float>(lc * z_pad), tmp_r = cv.add<float>(lc * z_pad);
    const auto i_r = cv.add<uint32_t>(lc * z_pad), itmp_r = cv.add<uint32_t>(lc * z_pad);
    const auto counts_r = cv.add<uint32_t>(lc * count_words), bases_r = cv.add<uint32_t>(lc * ssort::kRadix);
    const auto one_r = cv.add<float>(dr * wr * 32 * n_pad), zero_r = cv.add<float>(dr * wr * 32 * m_pad);
    const auto slots_r = cv.add<double>(dr * wr * 32 * nblk), sround_r = cv.add<double>(dr * wr * 32);
    const auto scounts_r = cv.add<uint32_t>(ssplit::counts_elems(N, dr, wr));
    const auto s_r = cv.add<double>(L * NL);
    const auto zeros_r = cv.add<float>(std::max(z_pad, dirs.l_img));
    const auto flag_r = cv.add<unsigned int>(64);
    FAD_TRY(cv.reserve(cx.ws->sliced));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(zeros_r), 0, (size_t)std::max(z_pad, dirs.l_img) * sizeof(float), st));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(flag_r), 0, 64 * sizeof(unsigned int), st));
    int64_t rounds = 0;
    for (int64_t l0 = 0; l0 < L; l0 += lc) rounds += cdiv(std::min(lc, L - l0), dr) * cdiv(W, wr);
    const ssort::Plan sp = ssort::plan(N, lc);
    sliced_perm_plan_value() = SlicedPermPlan{{cdiv(L, lc), lc, rounds, dr, wr, sp.G > 1 ? -sp.G : sp.W}};

    std::vector<float> sz(o.sorted_z ? (size_t)(L * N) : 0);
    std::vector<int32_t> hz(o.index_z ? (size_t)(L * N) : 0);
    float* K = cv.ptr(k_r);
    uint32_t* I = cv.ptr(i_r);
    float* one = cv.ptr(one_r);
    float* zero = cv.ptr(zero_r);
    const SlicedSortScratch sc{cv.ptr(tmp_r), cv.ptr(itmp_r), cv.ptr(counts_r), cv.ptr(bases_r)};
    const float* A = one_leads ? one : zero;
    const float* B = one_leads ? zero : one;
    const int64_t a_pad = one_leads ? n_pad : m_pad, b_pad = one_leads ? m_pad : n_pad;
    for (int64_t l0 = 0; l0 < L; l0 += lc) {
        const int64_t cur = std::min(lc, L - l0);
        FAD_TRY(sliced_project_sort(cx, pp.z, theta, cv.ptr(zeros_r), l0, cur, K, z_pad, I, sc, cv.ptr(flag_r)));
        FAD_TRY(sliced_stage(sz, l0, N, K, z_pad, cur, st));
        FAD_TRY(sliced_stage(hz, l0, N, I, z_pad, cur, st));
        for (int64_t d0 = 0; d0 < cur; d0 += dr)
            for (int64_t w0 = 0; w0 < W; w0 += wr) {
                const int64_t dc = std::min(dr, cur - d0), wc = std::min(wr, W - w0), nq = std::min(32 * wc, NL - 32 * w0), pairs = dc * nq;
                const ssplit::Args a{K + d0 * z_pad, I + d0 * z_pad, z_pad, N, pp.cols_d + w0 * z_pad, z_pad, dc, wc, G, nq,
                                     cv.ptr(scounts_r), one, zero, n_pad, m_pad, n, m};
                FAD_HIP_TRY(ssplit::split_segments(a, st));
                sliced_match_kernel<false><<<(unsigned int)(pairs * nblk), kMatchBlock, 0, st>>>(A, nullptr, a_pad, na, B, b_pad, nb, nblk, nullptr,
                                                                                                cv.ptr(slots_r), nullptr);
                FAD_HIP_TRY(hipGetLastError());
                sliced_finish_kernel<<<(unsigned int)cdiv(pairs, 256), 256, 0, st>>>(cv.ptr(slots_r), nblk, pairs, cv.ptr(sround_r));
                FAD_HIP_TRY(hipGetLastError());
                FAD_HIP_TRY(hipMemcpy2DAsync(cv.ptr(s_r) + (l0 + d0) * NL + 32 * w0, (size_t)NL * sizeof(double), cv.ptr(sround_r),
                                             (size_t)nq * sizeof(double), (size_t)nq * sizeof(double), (size_t)dc, hipMemcpyDeviceToDevice, st));
            }
    }
    std::vector<double> S((size_t)(L * NL));
    unsigned int flag = 0;
    FAD_HIP_TRY(hipMemcpyAsync(S.data(), cv.ptr(s_r), S.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(&flag, cv.ptr(flag_r), sizeof(flag), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (flag) return set_error(FAD_ERR_NOT_FINITE, "%s: a projection is not finite in float32", who);

    // per labelling the statistics of fad_sliced_wasserstein over its L values, S at a stride of NL; then the two counts, in float64
    const double nm = (double)(n * m);
    std::vector<double> Wv(o.values ? (size_t)(NL * L) : (size_t)L), T((size_t)NL), M((size_t)NL);
    SlicedStats obs{};
    for (int64_t u = 0; u < NL; ++u) {
        const SlicedStats t = sliced_stats(S.data() + u, NL, nm, dirs.q, Wv.data() + (o.values ? u * L : 0));
        T[(size_t)u] = t.mean; M[(size_t)u] = t.best;
        if (u == 0) obs = t;
    }
    int64_t ge = 0, ge_max = 0;
    for (int64_t p = 0; p < n_perm; ++p) {
        null_out[p] = T[(size_t)(p + 1)];
        null_max[p] = M[(size_t)(p + 1)];
        ge += T[(size_t)(p + 1)] >= T[0];
        ge_max += M[(size_t)(p + 1)] >= M[0];
    }
    out->observed.sw2_squared = obs.mean; out->observed.std_error = obs.std_error;
    out->observed.max_sliced = obs.best; out->observed.max_index = obs.best_l;
    out->observed.n = n; out->observed.m = m; out->observed.projections = projections;
    out->p_value = (double)(1 + ge) / (double)NL;
    out->p_value_max = (double)(1 + ge_max) / (double)NL;
    out->permutations = n_perm;
    if (o.values) memcpy(o.values, Wv.data(), Wv.size() * sizeof(double));
    if (o.sorted_z) memcpy(o.sorted_z, sz.data(), sz.size() * sizeof(float));
    if (o.index_z) memcpy(o.index_z, hz.data(), hz.size() * sizeof(int32_t));
    return FAD_OK;
}

// ------------------------------------------------------------------------------- sliced Wasserstein bootstrap
// fad_sliced_bootstrap_last_plan: sort chunks, directions per sort chunk, rounds in all, directions per round, replicate words per
// round, replicates per word
struct SlicedBootPlan { int64_t v[6]; };
static SlicedBootPlan& sliced_boot_plan_value() {
    static thread_local SlicedBootPlan p{{0, 0, 0, 0, 0, 0}};
    return p;
}

constexpr int64_t kBootMax = 65536;

// fad_sliced_bootstrap's detail.  All host; every pointer may be NULL.
struct SlicedBootOut { double* values; float* sorted_x; int32_t* index_x; float* sorted_y; int32_t* index_y; int64_t* totals; };

// One side's replicates on the host: the all-ones replicate in front of the caller's n_boot, every replicate's total, and the count
// words as sexpand takes them (cols [W x pad], byte b of word w of a row = its count in replicate 4 w + b; 0 past the last replicate).
struct BootSide {
    std::vector<int64_t> total;
    std::vector<uint32_t> cols;
    int64_t most = 0;

    int sum(const uint8_t* counts, int64_t rows, int64_t n_boot, const char* side, const char* who) {
        total.assign((size_t)(n_boot + 1), 0);
        total[0] = most = rows;
        for (int64_t b = 0; b < n_boot; ++b) {
            int64_t t = 0;
            for (int64_t i = 0; i < rows; ++i) t += counts[b * rows + i];
            if (t < 1) return set_error(FAD_ERR_INVALID, "%s: replicate %lld takes no row of %s", who, (long long)b, side);
            if (t > INT32_MAX - kTile)
                return set_error(FAD_ERR_INVALID, "%s: replicate %lld takes %lld rows of %s (at most %d)", who, (long long)b, (long long)t, side,
                                 INT32_MAX - kTile);
            total[(size_t)(b + 1)] = t;
            most = std::max(most, t);
        }
        return FAD_OK;
    }
    void pack(const uint8_t* counts, int64_t rows, int64_t pad) {
        const int64_t NB = (int64_t)total.size(), W = sexpand::words(NB);
        cols.assign((size_t)(W * pad), 0u);
        for (int64_t q = 0; q < NB; ++q) {
            uint32_t* w = cols.data() + (q / sexpand::kPerWord) * pad;
            const int shift = 8 * (int)(q % sexpand::kPerWord);
            if (q == 0) for (int64_t i = 0; i < rows; ++i) w[i] |= 1u << shift;
            else for (int64_t i = 0; i < rows; ++i) w[i] |= (uint32_t)counts[(q - 1) * rows + i] << shift;
        }
    }
};

// fad_sliced_bootstrap.  x and y are each projected and sorted once per direction, with the row at every rank (sliced_project_sort's
// key-index form).  A round takes some directions of the sort chunk and some replicate words: sexpand's stable expansion gives every
// (direction, replicate) pair of the round its two sorted resamples, and sliced_match_sized_kernel and sliced_finish_sized_kernel run
// over the pairs with every replicate's own sizes.  S [L][NB] stays on the device until every round has run.
static int sliced_bootstrap(const char* who, const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                            int on_device, const float* directions, int projections, const uint8_t* counts_x, const uint8_t* counts_y,
                            int64_t n_boot, fad_sliced_bootstrap_result_t* out, double* boot, double* boot_max, const SlicedBootOut& o,
                            int device, void* stream) {
    if (!x || !y) return set_error(FAD_ERR_INVALID, "%s: NULL rows", who);
    FAD_TRY(sliced_check_args(who, directions, dtype, d, ldx, &ldy, projections));
    if (n < 1 || m < 1) return set_error(FAD_ERR_TOO_FEW_ROWS, "%s: needs at least 1 row per set, got %lld and %lld", who, (long long)n, (long long)m);
    if (n > INT32_MAX - kTile || m > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "%s: %lld and %lld rows (at most %d per set)", who, (long long)n, (long long)m, INT32_MAX - kTile);
    if (n > (((int64_t)1 << 53) - 1) / m)
        return set_error(FAD_ERR_INVALID, "%s: n m = %lld x %lld is 2^53 or more: the integer weights would not be exact in float64", who,
                         (long long)n, (long long)m);
    if (n_boot < 1 || n_boot > kBootMax)
        return set_error(FAD_ERR_INVALID, "%s: %lld replicates (1 .. %lld)", who, (long long)n_boot, (long long)kBootMax);
    if (!counts_x || !counts_y) return set_error(FAD_ERR_INVALID, "%s: NULL counts", who);
    const int64_t L = projections, NB = n_boot + 1, W = sexpand::words(NB);
    SlicedDirections dirs;                                     // before any device call
    FAD_TRY(dirs.build(directions, L, d, dtype, who));
    BootSide bx, by;
    FAD_TRY(bx.sum(counts_x, n, n_boot, "x", who));
    FAD_TRY(by.sum(counts_y, m, n_boot, "y", who));
    for (int64_t u = 0; u < NB; ++u)
        if (bx.total[(size_t)u] > (((int64_t)1 << 53) - 1) / by.total[(size_t)u])
            return set_error(FAD_ERR_INVALID, "%s: replicate %lld has n m = %lld x %lld, 2^53 or more: the integer weights would not be exact "
                             "in float64", who, (long long)(u - 1), (long long)bx.total[(size_t)u], (long long)by.total[(size_t)u]);
    const int64_t budget = sliced_budget();
    const int64_t n_pad = kad::blocks(n) * kTile, m_pad = kad::blocks(m) * kTile, t_pad = std::max(n_pad, m_pad);
    bx.pack(counts_x, n, n_pad);
    by.pack(counts_y, m, m_pad);
    std::vector<int32_t> sizes((size_t)(2 * NB));              // every replicate's total of x, then of y
    for (int64_t u = 0; u < NB; ++u) { sizes[(size_t)u] = (int32_t)bx.total[(size_t)u]; sizes[(size_t)(NB + u)] = (int32_t)by.total[(size_t)u]; }

    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    const hipStream_t st = cx.st;
    Packed px, py;                                             // each set packed once, its norms checked finite
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    FAD_TRY(pack_set(cx, 1, y, m, ldy, d, on_device, &py));
    const char* theta;
    FAD_TRY(dirs.upload(cx, &theta));

    // the sort chunk: lc directions' keys and rows of both sets, the sort's second buffers and counts -- a quarter of the budget.  The
    // round: dr directions x wr replicate words, 4 pairs a word, each pair its two expanded sets at the pitch of the largest replicate,
    // its match slots and the expansion's counts (x's, then y's in the same words).
    const int64_t xp = kad::blocks(bx.most) * kTile, yp = kad::blocks(by.most) * kTile;
    const int64_t nblk = cdiv(std::max(bx.most, by.most), kMatchBlock), G = std::max(sexpand::groups(n), sexpand::groups(m));
    const int64_t count_words = std::max(ssort::counts_elems(n, 1), ssort::counts_elems(m, 1));
    const int64_t per_dir = 8 * (n_pad + m_pad + t_pad) + 4 * (count_words + ssort::kRadix);
    const int64_t lc = std::max<int64_t>(1, std::min<int64_t>(L, budget / 4 / per_dir));
    const int64_t per_word = sexpand::kPerWord * (4 * (xp + yp) + 8 * nblk + 4 * G + 8);
    const int64_t most = (int64_t)INT32_MAX / (sexpand::kPerWord * std::max(nblk, G)); // words a launch's grid can hold
    const int64_t units = std::max<int64_t>(1, std::min(most, (budget - budget / 4) / per_word));
    const int64_t wr = std::min(W, units), dr = units >= W ? std::min(lc, units / W) : 1;
    Carve cv;
    const auto kx_r = cv.add<float>(lc * n_pad), ky_r = cv.add<float>(lc * m_pad), tmp_r = cv.add<float>(lc * t_pad);
    const auto ix_r = cv.add<uint32_t>(lc * n_pad), iy_r = cv.add<uint32_t>(lc * m_pad), itmp_r = cv.add<uint32_t>(lc * t_pad);
    const auto counts_r = cv.add<uint32_t>(lc * count_words), bases_r = cv.add<uint32_t>(lc * ssort::kRadix);
    const auto ex_r = cv.add<float>(dr * wr * sexpand::kPerWord * xp), ey_r = cv.add<float>(dr * wr * sexpand::kPerWord * yp);
    const auto slots_r = cv.add<double>(dr * wr * sexpand::kPerWord * nblk), sround_r = cv.add<double>(dr * wr * sexpand::kPerWord);
    const auto ecounts_r = cv.add<uint32_t>(dr * wr * G * sexpand::kPerWord);
    const auto colsx_r = cv.add<uint32_t>(W * n_pad), colsy_r = cv.add<uint32_t>(W * m_pad);
    const auto sizes_r = cv.add<int32_t>(2 * NB);
    const auto s_r = cv.add<double>(L * NB);
    const auto zeros_r = cv.add<float>(std::max(t_pad, dirs.l_img));
    const auto flag_r = cv.add<unsigned int>(64);
    FAD_TRY(cv.reserve(cx.ws->sliced));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(zeros_r), 0, (size_t)std::max(t_pad, dirs.l_img) * sizeof(float), st));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(flag_r), 0, 64 * sizeof(unsigned int), st));
    FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(colsx_r), bx.cols.data(), bx.cols.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(colsy_r), by.cols.data(), by.cols.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(sizes_r), sizes.data(), sizes.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    int64_t rounds = 0;
    for (int64_t l0 = 0; l0 < L; l0 += lc) rounds += cdiv(std::min(lc, L - l0), dr) * cdiv(W, wr);
    sliced_boot_plan_value() = SlicedBootPlan{{cdiv(L, lc), lc, rounds, dr, wr, sexpand::kPerWord}};

    std::vector<float> sx(o.sorted_x ? (size_t)(L * n) : 0), sy(o.sorted_y ? (size_t)(L * m) : 0);
    std::vector<int32_t> hx(o.index_x ? (size_t)(L * n) : 0), hy(o.index_y ? (size_t)(L * m) : 0);
    float* Kx = cv.ptr(kx_r);
    float* Ky = cv.ptr(ky_r);
    uint32_t* Ix = cv.ptr(ix_r);
    uint32_t* Iy = cv.ptr(iy_r);
    float* Ex = cv.ptr(ex_r);
    float* Ey = cv.ptr(ey_r);
    const int32_t* tx = cv.ptr(sizes_r);
    const int32_t* ty = tx + NB;
    const SlicedSortScratch sc{cv.ptr(tmp_r), cv.ptr(itmp_r), cv.ptr(counts_r), cv.ptr(bases_r)};
    for (int64_t l0 = 0; l0 < L; l0 += lc) {
        const int64_t cur = std::min(lc, L - l0);
        FAD_TRY(sliced_project_sort(cx, px, theta, cv.ptr(zeros_r), l0, cur, Kx, n_pad, Ix, sc, cv.ptr(flag_r)));
        FAD_TRY(sliced_project_sort(cx, py, theta, cv.ptr(zeros_r), l0, cur, Ky, m_pad, Iy, sc, cv.ptr(flag_r)));
        FAD_TRY(sliced_stage(sx, l0, n, Kx, n_pad, cur, st));
        FAD_TRY(sliced_stage(sy, l0, m, Ky, m_pad, cur, st));
        FAD_TRY(sliced_stage(hx, l0, n, Ix, n_pad, cur, st));
        FAD_TRY(sliced_stage(hy, l0, m, Iy, m_pad, cur, st));
        for (int64_t d0 = 0; d0 < cur; d0 += dr)
            for (int64_t w0 = 0; w0 < W; w0 += wr) {
                const int64_t dc = std::min(dr, cur - d0), wc = std::min(wr, W - w0), q0 = sexpand::kPerWord * w0;
                const int64_t nq = std::min(sexpand::kPerWord * wc, NB - q0), pairs = dc * nq;
                const sexpand::Args ax{Kx + d0 * n_pad, Ix + d0 * n_pad, n_pad, n, cv.ptr(colsx_r) + w0 * n_pad, n_pad, dc, wc,
                                       sexpand::groups(n), nq, cv.ptr(ecounts_r), Ex, xp, tx + q0};
                const sexpand::Args ay{Ky + d0 * m_pad, Iy + d0 * m_pad, m_pad, m, cv.ptr(colsy_r) + w0 * m_pad, m_pad, dc, wc,
                                       sexpand::groups(m), nq, cv.ptr(ecounts_r), Ey, yp, ty + q0};
                FAD_HIP_TRY(sexpand::expand_segments(ax, st));
                FAD_HIP_TRY(sexpand::expand_segments(ay, st));
                sliced_match_sized_kernel<<<(unsigned int)(pairs * nblk), kMatchBlock, 0, st>>>(Ex, xp, Ey, yp, tx + q0, ty + q0, nq, nblk,
                                                                                              cv.ptr(slots_r));
                FAD_HIP_TRY(hipGetLastError());
                sliced_finish_sized_kernel<<<(unsigned int)cdiv(pairs, 256), 256, 0, st>>>(cv.ptr(slots_r), nblk, tx + q0, ty + q0, nq, pairs,
                                                                                         cv.ptr(sround_r));
                FAD_HIP_TRY(hipGetLastError());
                FAD_HIP_TRY(hipMemcpy2DAsync(cv.ptr(s_r) + (l0 + d0) * NB + q0, (size_t)NB * sizeof(double), cv.ptr(sround_r),
                                             (size_t)nq * sizeof(double), (size_t)nq * sizeof(double), (size_t)dc, hipMemcpyDeviceToDevice, st));
            }
    }
    std::vector<double> S((size_t)(L * NB));
    unsigned int flag = 0;
    FAD_HIP_TRY(hipMemcpyAsync(S.data(), cv.ptr(s_r), S.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(&flag, cv.ptr(flag_r), sizeof(flag), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (flag) return set_error(FAD_ERR_NOT_FINITE, "%s: a projection is not finite in float32", who);

    // per replicate the statistics of fad_sliced_wasserstein over its L values, S at a stride of NB, with the replicate's own n m
    std::vector<double> Wv(o.values ? (size_t)(NB * L) : (size_t)L);
    SlicedStats obs{};
    for (int64_t u = 0; u < NB; ++u) {
        const double nm = (double)(bx.total[(size_t)u] * by.total[(size_t)u]);
        const SlicedStats t = sliced_stats(S.data() + u, NB, nm, dirs.q, Wv.data() + (o.values ? u * L : 0));
        if (u == 0) obs = t;
        else { boot[u - 1] = t.mean; boot_max[u - 1] = t.best; }
    }
    out->observed.sw2_squared = obs.mean; out->observed.std_error = obs.std_error;
    out->observed.max_sliced = obs.best; out->observed.max_index = obs.best_l;
    out->observed.n = n; out->observed.m = m; out->observed.projections = projections;
    out->replicates = n_boot;
    if (o.values) memcpy(o.values, Wv.data(), Wv.size() * sizeof(double));
    if (o.sorted_x) memcpy(o.sorted_x, sx.data(), sx.size() * sizeof(float));
    if (o.sorted_y) memcpy(o.sorted_y, sy.data(), sy.size() * sizeof(float));
    if (o.index_x) memcpy(o.index_x, hx.data(), hx.size() * sizeof(int32_t));
    if (o.index_y) memcpy(o.index_y, hy.data(), hy.size() * sizeof(int32_t));
    if (o.totals)
        for (int64_t u = 0; u < NB; ++u) { o.totals[2 * u] = bx.total[(size_t)u]; o.totals[2 * u + 1] = by.total[(size_t)u]; }
    return FAD_OK;
}

// What fad_sliced_individual writes: five values per song and, where not NULL, its detail's arrays.  All host.
struct SlicedSongOut {
    double* sw2; double* std_error; double* max_sliced; int64_t* max_index; int32_t* status;
    double* values; float* sorted_x; float* sorted_rows;
};

// fad_sliced_individual: the baseline's side of a chunk as sliced_sets has it; the song rows projected in one launch, every song's
// range sorted on its own (resident units, the long songs by the global sort), one match workgroup per (direction, song).
static int sliced_songs(const char* who, const void* x, int64_t n, int64_t ldx, const void* rows, int64_t n_rows, int64_t ldy,
                        const int64_t* offsets, int64_t n_songs, int64_t d, int dtype, int on_device, const float* directions,
                        int projections, const SlicedSongOut& o, int device, void* stream) {
    if (!x) return set_error(FAD_ERR_INVALID, "%s: NULL rows", who);
    if (!offsets) return set_error(FAD_ERR_INVALID, "%s: NULL offsets", who);
    FAD_TRY(sliced_check_args(who, directions, dtype, d, ldx, nullptr, projections));
    if (n < 1) return set_error(FAD_ERR_TOO_FEW_ROWS, "%s: needs at least 1 baseline row, got %lld", who, (long long)n);
    if (n > INT32_MAX - kTile) return set_error(FAD_ERR_INVALID, "%s: %lld baseline rows (at most %d)", who, (long long)n, INT32_MAX - kTile);
    if (n_songs < 1 || n_songs > INT32_MAX) return set_error(FAD_ERR_INVALID, "%s: %lld songs", who, (long long)n_songs);
    if (n_rows < 0 || n_rows > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "%s: %lld song rows (at most %d)", who, (long long)n_rows, INT32_MAX - kTile);
    if (n_rows > 0 && !rows) return set_error(FAD_ERR_INVALID, "%s: NULL song rows", who);
    if (n_rows > 0 && ldy < d) return set_error(FAD_ERR_INVALID, "%s: song row pitch %lld < D = %lld", who, (long long)ldy, (long long)d);
    if (offsets[0] != 0 || offsets[n_songs] != n_rows)
        return set_error(FAD_ERR_INVALID, "%s: offsets run from %lld to %lld, not 0 to %lld", who, (long long)offsets[0],
                         (long long)offsets[n_songs], (long long)n_rows);
    int64_t longest = 0;
    for (int64_t s = 0; s < n_songs; ++s) {
        const int64_t m = offsets[s + 1] - offsets[s];
        if (m < 0) return set_error(FAD_ERR_INVALID, "%s: offsets decrease at song %lld", who, (long long)s);
        if (m > 0 && n > (((int64_t)1 << 53) - 1) / m)
            return set_error(FAD_ERR_INVALID, "%s: n m = %lld x %lld (song %lld) is 2^53 or more: the integer weights would not be exact in "
                             "float64", who, (long long)n, (long long)m, (long long)s);
        longest = std::max(longest, m);
    }
    const int64_t L = projections;
    SlicedDirections dirs;                                     // before any device call
    FAD_TRY(dirs.build(directions, L, d, dtype, who));
    const int64_t budget = sliced_budget();
    const songsort::Table table = songsort::build_units(offsets, n_songs);
    const int64_t n_units = (int64_t)table.units.size(), n_long = (int64_t)table.long_songs.size();

    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    const hipStream_t st = cx.st;
    Packed px, pr{};                                           // the baseline's norms are checked finite; the songs' per song, below
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    if (n_rows > 0) FAD_TRY(pack_image(cx, 1, rows, n_rows, ldy, d, on_device, &pr));
    const char* theta;
    FAD_TRY(dirs.upload(cx, &theta));

    // the chunk: lc directions' projections of the baseline and of all song rows, the global sort's second buffer (as wide as the song
    // rows only when a song takes the long path) and counts, one sum per song
    const int64_t n_pad = kad::blocks(n) * kTile, r_pad = kad::blocks(n_rows) * kTile, t_pad = std::max(n_pad, n_long ? r_pad : 0);
    const int64_t count_words = std::max(ssort::counts_elems(n, 1), ssort::counts_elems(longest > songsort::kCapacity ? longest : 1, 1));
    const int64_t per_dir = 4 * (n_pad + r_pad + t_pad) + 4 * (count_words + ssort::kRadix) + 8 * n_songs;
    const int64_t lc = std::max<int64_t>(1, std::min<int64_t>(L, budget / per_dir));
    const int64_t n_zeros = std::max(std::max(n_pad, r_pad), dirs.l_img);
    Carve cv;
    const auto px_r = cv.add<float>(lc * n_pad), pr_r = cv.add<float>(lc * r_pad), tmp_r = cv.add<float>(lc * t_pad);
    const auto counts_r = cv.add<uint32_t>(lc * count_words), bases_r = cv.add<uint32_t>(lc * ssort::kRadix);
    const auto s_r = cv.add<double>(lc * n_songs);
    const auto zeros_r = cv.add<float>(n_zeros);
    const auto off_r = cv.add<int64_t>(n_songs + 1);
    const auto units_r = cv.add<songsort::Unit>(n_units);
    const auto ends_r = cv.add<int32_t>((int64_t)table.ends.size());
    const auto bad_r = cv.add<unsigned int>(n_songs);
    const auto flag_r = cv.add<unsigned int>(128);             // word 0: the baseline's projections; word 64: the song rows', never read
    FAD_TRY(cv.reserve(cx.ws->sliced));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(zeros_r), 0, (size_t)n_zeros * sizeof(float), st));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(flag_r), 0, 128 * sizeof(unsigned int), st));
    FAD_HIP_TRY(hipMemsetAsync(cv.ptr(bad_r), 0, (size_t)n_songs * sizeof(unsigned int), st));
    FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(off_r), offsets, (size_t)(n_songs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (n_units) {
        FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(units_r), table.units.data(), (size_t)n_units * sizeof(songsort::Unit), hipMemcpyHostToDevice, st));
        FAD_HIP_TRY(hipMemcpyAsync(cv.ptr(ends_r), table.ends.data(), table.ends.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    sliced_song_plan_value() = SlicedSongPlan{{cdiv(L, lc), lc, n_units, n_long, table.most_songs, songsort::kCapacity}};

    if (n_rows > 0) {
        sliced_song_norm_kernel<<<(unsigned int)cdiv(n_rows, 256), 256, 0, st>>>(pr.h, n_rows, cv.ptr(off_r), n_songs, cv.ptr(bad_r));
        FAD_HIP_TRY(hipGetLastError());
    }
    std::vector<double> S((size_t)(L * n_songs), 0.0);
    std::vector<float> sx(o.sorted_x ? (size_t)(L * n) : 0), sr(o.sorted_rows ? (size_t)(L * n_rows) : 0);
    float* Px = cv.ptr(px_r);
    float* Pr = cv.ptr(pr_r);
    unsigned int* flags = cv.ptr(flag_r);
    const SlicedSortScratch sc{cv.ptr(tmp_r), nullptr, cv.ptr(counts_r), cv.ptr(bases_r)};
    for (int64_t l0 = 0; l0 < L; l0 += lc) {
        const int64_t cur = std::min(lc, L - l0);
        FAD_TRY(sliced_project_sort(cx, px, theta, cv.ptr(zeros_r), l0, cur, Px, n_pad, nullptr, sc, flags));
        if (n_rows > 0) {
            FAD_TRY(sliced_project(cx, pr, theta, cv.ptr(zeros_r), l0, cur, Pr, r_pad, flags + 64));
            FAD_HIP_TRY(songsort::sort_units(Pr, r_pad, cur, cv.ptr(units_r), cv.ptr(ends_r), n_units, st));
            for (const int64_t s : table.long_songs)           // the rare path: the global sort, song by song
                FAD_HIP_TRY(ssort::sort_segments(Pr + offsets[s], sc.tmp + offsets[s], r_pad, offsets[s + 1] - offsets[s], cur, sc.counts,
                                                 sc.bases, st));
            SongMatchArgs ma{Px, n_pad, n, Pr, r_pad, cv.ptr(off_r), n_songs, cv.ptr(s_r), cv.ptr(bad_r)};
            const int64_t per = std::max<int64_t>(1, (int64_t)INT32_MAX / n_songs);    // directions per launch: the grid's x extent
            for (int64_t c0 = 0; c0 < cur; c0 += per) {
                const int64_t cc = std::min(per, cur - c0);
                ma.px = Px + c0 * n_pad; ma.pr = Pr + c0 * r_pad; ma.S = cv.ptr(s_r) + c0 * n_songs;
                sliced_song_match_kernel<<<(unsigned int)(cc * n_songs), kMatchBlock, 0, st>>>(ma);
                FAD_HIP_TRY(hipGetLastError());
            }
            FAD_HIP_TRY(hipMemcpyAsync(S.data() + l0 * n_songs, cv.ptr(s_r), (size_t)(cur * n_songs) * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        FAD_TRY(sliced_stage(sx, l0, n, Px, n_pad, cur, st));
        FAD_TRY(sliced_stage(sr, l0, n_rows, Pr, r_pad, cur, st));
    }
    std::vector<unsigned int> bad((size_t)n_songs);
    unsigned int flag = 0;
    FAD_HIP_TRY(hipMemcpyAsync(bad.data(), cv.ptr(bad_r), (size_t)n_songs * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(&flag, flags, sizeof(flag), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (flag) return set_error(FAD_ERR_NOT_FINITE, "%s: a projection of the baseline is not finite in float32", who);

    // per song, the statistics of fad_sliced_wasserstein over the pair (x, song)
    std::vector<double> W((size_t)L);
    for (int64_t s = 0; s < n_songs; ++s) {
        const int64_t m = offsets[s + 1] - offsets[s];
        double* vals = o.values ? o.values + s * L : nullptr;
        if (m == 0 || bad[(size_t)s]) {
            o.status[s] = m == 0 ? FAD_ERR_TOO_FEW_ROWS : FAD_ERR_NOT_FINITE;
            o.sw2[s] = o.std_error[s] = o.max_sliced[s] = NAN;
            o.max_index[s] = -1;
            for (int64_t l = 0; vals && l < L; ++l) vals[l] = NAN;
            continue;
        }
        const SlicedStats t = sliced_stats(S.data() + s, n_songs, (double)(n * m), dirs.q, W.data());
        o.status[s] = FAD_OK;
        o.sw2[s] = t.mean; o.std_error[s] = t.std_error;
        o.max_sliced[s] = t.best; o.max_index[s] = t.best_l;
        if (vals) memcpy(vals, W.data(), (size_t)L * sizeof(double));
    }
    if (o.sorted_x) memcpy(o.sorted_x, sx.data(), sx.size() * sizeof(float));
    if (o.sorted_rows && !sr.empty()) memcpy(o.sorted_rows, sr.data(), sr.size() * sizeof(float));
    return FAD_OK;
}

// ------------------------------------------------------------------------------------------- Lloyd's k-means
// fad_kmeans_last_plan: planes, launches of the last assignment, update chunk rows, most chunks of one cluster in the last update,
// iterations, assignments made
struct KmeansPlan { int64_t v[6]; };
static KmeansPlan& kmeans_plan_value() {
    static thread_local KmeansPlan p{{0, 0, 0, 0, 0, 0}};
    return p;
}

template <int DT> struct KmeansRow { using type = float; };
template <> struct KmeansRow<FAD_F16> { using type = _Float16; };
template <> struct KmeansRow<FAD_BF16> { using type = __bf16; };

static int kmeans_planes(int dtype) { return dtype == FAD_F16 ? 2 : dtype == FAD_BF16 ? 3 : 1; }

// fad_kmeans once its arguments are checked: the pooled rows packed once (and repeated once per plane), then the loop of DESIGN 4.22 --
// an assignment is nearest_pass with the centroids as the row operand and k = 1, an update is kmeans::update.  The host reads one
// integer per iteration (the changed labels); everything else stays on the device until the end.
static int kmeans_run(const Ctx& cx, const RowSet* sets, int n_sets, int64_t N, int64_t d, int on_device, int64_t K, const float* init,
                      int max_iter, float* centroids, int32_t* labels, int64_t* counts, float* dist2, double* inertia_trace,
                      fad_kmeans_result_t* out) {
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;
    const size_t es = dtype_size(cx.dtype);
    const int P = kmeans_planes(cx.dtype);
    const int64_t z_pad = kad::blocks(N) * kTile, k_pad = kad::blocks(K) * kTile, dp = depth_elems(d, cx.dtype);

    Packed pz;
    FAD_TRY(pack_sets(cx, sets, n_sets, d, on_device, z_pad, true, &pz));
    pz.n = N;
    std::vector<double> info((size_t)(2 * n_sets));
    FAD_HIP_TRY(hipMemcpyAsync(info.data(), static_cast<double*>(ws.small.p) + 1024, info.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    double bad_rows = 0.0;
    for (int i = 0; i < n_sets; ++i) bad_rows += info[(size_t)(2 * i + 1)];
    if (bad_rows != 0.0)
        return set_error(FAD_ERR_NOT_FINITE, "fad_kmeans: %lld of %lld rows have a NaN/Inf norm", (long long)bad_rows, (long long)N);

    // float16 rows: the power of two g that the operands are scaled by (kmeans::f16_scale), from the largest row magnitude
    float g = 1.f;
    if (cx.dtype == FAD_F16) {
        unsigned int* max_d = reinterpret_cast<unsigned int*>(static_cast<double*>(ws.small.p) + 1024 + 2 * kmeans::kMaxSets);
        unsigned int max_bits = 0;
        FAD_HIP_TRY(hipMemsetAsync(max_d, 0, sizeof(unsigned int), st));
        const int64_t count = z_pad * dp;
        kmeans::absmax_f16_kernel<<<(unsigned)std::min<int64_t>(cdiv(count, 256), 4096), 256, 0, st>>>(reinterpret_cast<const uint16_t*>(pz.img),
                                                                                                     count, max_d);
        FAD_HIP_TRY(hipGetLastError());
        FAD_HIP_TRY(hipMemcpyAsync(&max_bits, max_d, sizeof(max_bits), hipMemcpyDeviceToHost, st));
        FAD_HIP_TRY(hipStreamSynchronize(st));
        g = kmeans::f16_scale(max_bits);
    }

    // the column operand: every row (times g) P times side by side, against the P planes of g c; h of the rows times g^2
    Packed rows = pz;
    if (P > 1) {
        FAD_TRY(ws.img[1].reserve((size_t)(z_pad * pz.pitch * P)));
        FAD_TRY(ws.h[1].reserve((size_t)z_pad * sizeof(float)));
        FAD_TRY(with_dtype(cx.dtype, [&](auto dt) {
            using T = typename KmeansRow<decltype(dt)::value>::type;
            if constexpr (kmeans::Planes<T>::value > 1) {
                const int64_t vecs = z_pad * (dp / (16 / (int64_t)sizeof(T)));
                kmeans::replicate_kernel<T><<<(unsigned)cdiv(vecs, 256), 256, 0, st>>>(reinterpret_cast<const T*>(pz.img), z_pad, dp, g,
                                                                                     static_cast<T*>(ws.img[1].p));
            }
        }));
        float* hs = static_cast<float*>(ws.h[1].p);
        kmeans::scale_kernel<<<(unsigned)cdiv(z_pad, 256), 256, 0, st>>>(pz.h, g * g, z_pad, hs);
        FAD_HIP_TRY(hipGetLastError());
        rows = Packed{static_cast<const char*>(ws.img[1].p), hs, N, pz.pitch * P, pz.nchunks * P, 0.0};
    }

    const int64_t chunks = kmeans::chunks_bound(N, K), T1 = (int64_t)max_iter + 1;
    Carve cv;
    const auto cent_r = cv.add<float>(K * d);
    const auto cimg_r = cv.add<char>(k_pad * rows.pitch);
    const auto ch_r = cv.add<float>(k_pad);
    const auto lab_r = cv.add<int32_t>(2 * N);
    const auto dist2_r = cv.add<float>(N);
    const auto keys_r = cv.add<uint32_t>(4 * N);
    const auto scount_r = cv.add<uint32_t>(kmeans::sort_counts_elems(N));
    const auto sbase_r = cv.add<uint32_t>(ssort::bases_elems(1));
    const auto counts_r = cv.add<uint32_t>(K), starts_r = cv.add<uint32_t>(K + 1), chunk0_r = cv.add<uint32_t>(K + 1), stats_r = cv.add<uint32_t>(2);
    const auto partial_r = cv.add<double>(chunks * d);
    const auto trace_r = cv.add<double>(T1);
    const auto flag_r = cv.add<unsigned long long>(2);
    FAD_TRY(cv.reserve(ws.kmeans));
    float* cent = cv.ptr(cent_r);
    char* cimg = cv.ptr(cimg_r);
    float* ch = cv.ptr(ch_r);
    int32_t* lab[2] = {cv.ptr(lab_r), cv.ptr(lab_r) + N};
    float* dist2_d = cv.ptr(dist2_r);
    kmeans::UpdateScratch w{};
    w.keys = cv.ptr(keys_r); w.keys_tmp = w.keys + N; w.idx = w.keys + 2 * N; w.idx_tmp = w.keys + 3 * N;
    w.sort_counts = cv.ptr(scount_r); w.sort_bases = cv.ptr(sbase_r);
    w.counts = cv.ptr(counts_r); w.starts = cv.ptr(starts_r); w.chunk0 = cv.ptr(chunk0_r); w.stats = cv.ptr(stats_r);
    w.partial = cv.ptr(partial_r);
    double* trace_d = cv.ptr(trace_r);
    unsigned long long* bad_d = cv.ptr(flag_r);
    unsigned long long* changed_d = bad_d + 1;
    const PrdcPlan q = prdc_plan(cx, Packed{cimg, ch, K, rows.pitch, rows.nchunks, 0.0}, rows, kad::kNearestEpilogue);
    FAD_TRY(ws.lists.reserve((size_t)(q.NR * z_pad) * sizeof(uint64_t)));
    const Packed pc{cimg, ch, K, rows.pitch, rows.nchunks, 0.0};

    // C_0: the given centroids, their planes and h
    FAD_HIP_TRY(hipMemcpyAsync(cent, init, (size_t)(K * d) * sizeof(float), hipMemcpyHostToDevice, st));
    FAD_HIP_TRY(hipMemsetAsync(bad_d, 0, 2 * sizeof(unsigned long long), st));
    FAD_HIP_TRY(hipMemsetAsync(w.stats, 0, 2 * sizeof(uint32_t), st));
    FAD_TRY(with_dtype(cx.dtype, [&](auto dt) {
        using T = typename KmeansRow<decltype(dt)::value>::type;
        kmeans::centroid_finish_kernel<T><<<(unsigned)cdiv(k_pad, 4), 256, 0, st>>>(nullptr, nullptr, nullptr, K, k_pad, d, dp, cent,
                                                                                 reinterpret_cast<T*>(cimg), ch, g, bad_d);
    }));
    unsigned long long bad_cent = 0;
    FAD_HIP_TRY(hipMemcpyAsync(&bad_cent, bad_d, sizeof(bad_cent), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (bad_cent)
        return set_error(FAD_ERR_NOT_FINITE, "fad_kmeans: %llu of %lld init centroids are not finite in the rows' dtype (float16 rows: an entry "
                         "must stay below 32x the largest row entry)", bad_cent, (long long)K);

    int64_t assignments = 0, last_launches = 0;
    auto assign = [&](int32_t* into) -> int {
        const int64_t before = kad::plan_tally().launches;
        FAD_TRY(nearest_pass(cx, pc, rows, false, 1, static_cast<uint64_t*>(ws.lists.p), into, dist2_d));
        last_launches = kad::plan_tally().launches - before;
        if (g != 1.f) kmeans::scale_kernel<<<(unsigned)cdiv(N, 256), 256, 0, st>>>(dist2_d, 1.f / (g * g), N, dist2_d);   // d^2 of g x, g c
        kmeans::inertia_kernel<<<1, 256, 0, st>>>(dist2_d, N, trace_d + assignments);
        FAD_HIP_TRY(hipGetLastError());
        ++assignments;
        return FAD_OK;
    };
    // the labels of `now` that differ from `then`: the one integer the host reads per iteration
    auto changed = [&](const int32_t* now, const int32_t* then, unsigned long long* count) -> int {
        FAD_HIP_TRY(hipMemsetAsync(changed_d, 0, sizeof(unsigned long long), st));
        kmeans::labels_changed_kernel<<<(unsigned)cdiv(N, 256), 256, 0, st>>>(now, then, N, changed_d);
        FAD_HIP_TRY(hipGetLastError());
        FAD_HIP_TRY(hipMemcpyAsync(count, changed_d, sizeof(*count), hipMemcpyDeviceToHost, st));
        FAD_HIP_TRY(hipStreamSynchronize(st));
        return FAD_OK;
    };
    auto update = [&](const int32_t* from) -> int {
        hipError_t e = hipSuccess;
        FAD_TRY(with_dtype(cx.dtype, [&](auto dt) {
            using T = typename KmeansRow<decltype(dt)::value>::type;
            e = kmeans::update<T>(from, N, K, k_pad, d, dp, reinterpret_cast<const T*>(pz.img), pz.pitch / (int64_t)es, w, cent,
                                  reinterpret_cast<T*>(cimg), ch, g, st);
        }));
        FAD_HIP_TRY(e);
        return FAD_OK;
    };

    int cur = 0, converged = 0, iterations = 0;
    long long changed_last = -1;
    bool updated = false;
    for (int t = 1; t <= max_iter; ++t) {
        FAD_TRY(assign(lab[cur]));
        iterations = t;
        if (t > 1) {
            unsigned long long c = 0;
            FAD_TRY(changed(lab[cur], lab[cur ^ 1], &c));
            changed_last = (long long)c;
            if (c == 0) { converged = 1; break; }
        }
        FAD_TRY(update(lab[cur]));
        updated = true;
        cur ^= 1;
    }
    if (!converged) {                                                                 // labels that belong to the returned centroids
        FAD_TRY(assign(lab[cur]));
        if (max_iter > 0) {
            unsigned long long c = 0;
            FAD_TRY(changed(lab[cur], lab[cur ^ 1], &c));
            changed_last = (long long)c;
        }
    }

    // counts of the returned labels
    FAD_HIP_TRY(hipMemsetAsync(w.counts, 0, (size_t)K * sizeof(uint32_t), st));
    kmeans::label_count_kernel<<<(unsigned)cdiv(N, 256), 256, 0, st>>>(lab[cur], N, K, w.keys, w.counts);
    FAD_HIP_TRY(hipGetLastError());
    std::vector<uint32_t> counts_h((size_t)K);
    std::vector<double> trace((size_t)assignments);
    uint32_t stats[2] = {0, 0};
    FAD_HIP_TRY(hipMemcpyAsync(counts_h.data(), w.counts, (size_t)K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(trace.data(), trace_d, trace.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(stats, w.stats, sizeof(stats), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(centroids, cent, (size_t)(K * d) * sizeof(float), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(labels, lab[cur], (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (dist2) FAD_HIP_TRY(hipMemcpyAsync(dist2, dist2_d, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));

    int64_t empty = 0;
    for (int64_t c = 0; c < K; ++c) {
        counts[c] = (int64_t)counts_h[(size_t)c];
        empty += counts_h[(size_t)c] == 0;
    }
    if (inertia_trace) memcpy(inertia_trace, trace.data(), trace.size() * sizeof(double));
    out->inertia = trace.back();
    out->n = N; out->k = K; out->iterations = iterations; out->converged = converged; out->changed_last = changed_last;
    out->empty_clusters = empty; out->assignments = assignments;
    kmeans_plan_value() = KmeansPlan{{P, last_launches, kmeans::kChunkRows, updated ? (int64_t)stats[0] : 0, iterations, assignments}};
    return FAD_OK;
}

}  // namespace

}  // namespace fad

extern "C" {

int fad_kad_median_distance(const void* x, int64_t n, int64_t ld, int64_t d, int dtype, int on_device, double* sigma, int device,
                            void* stream) {
    using namespace fad;
    begin_entry();
    if (!sigma) return set_error(FAD_ERR_INVALID, "fad_kad_median_distance: NULL output");
    FAD_TRY(check_rows(x, n, ld, d, dtype, "fad_kad_median_distance"));
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    Packed px;
    FAD_TRY(pack_set(cx, 0, x, n, ld, d, on_device, &px));
    return median_of_packed(cx, px, sigma);
}

int fad_kad(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
            double bandwidth, fad_kad_result_t* out, int device, void* stream) {
    return fad_kad_k(x, n, ldx, y, m, ldy, d, dtype, on_device, bandwidth, FAD_KAD_GAUSSIAN, out, device, stream);
}

int fad_kad_k(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
              double bandwidth, int kernel, fad_kad_result_t* out, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!out) return set_error(FAD_ERR_INVALID, "fad_kad: NULL output");
    FAD_TRY(check_kernel(kernel, "fad_kad"));
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kad (x)"));
    FAD_TRY(check_rows(y, m, ldy, d, dtype, "fad_kad (y)"));
    if (std::isnan(bandwidth) || std::isinf(bandwidth))
        return set_error(FAD_ERR_INVALID, "fad_kad: bandwidth %g is not finite", bandwidth);
    Ctx cx;
    FAD_TRY(cx.open(dtype, kernel, device, stream));

    Packed px, py;
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    FAD_TRY(pack_set(cx, 1, y, m, ldy, d, on_device, &py));
    double sigma, sums[3];
    float c;
    FAD_TRY(resolve_sigma(cx, px, bandwidth, "fad_kad", &sigma, &c));
    FAD_TRY(kad_three_passes(cx, px, py, &c, 1, sums));
    fill_result(out, 2.0 * sums[0], 2.0 * sums[1], sums[2], n, m, sigma);
    return FAD_OK;
}


int fad_kad_sweep(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                  const double* bandwidths, int n_bw, int relative, int kernel, fad_kad_result_t* out, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!out) return set_error(FAD_ERR_INVALID, "fad_kad_sweep: NULL output");
    if (!bandwidths) return set_error(FAD_ERR_INVALID, "fad_kad_sweep: NULL bandwidths");
    if (n_bw < 1 || n_bw > FAD_KAD_MAX_BANDWIDTHS)
        return set_error(FAD_ERR_INVALID, "fad_kad_sweep: %d bandwidths, outside 1 .. %d", n_bw, FAD_KAD_MAX_BANDWIDTHS);
    FAD_TRY(check_kernel(kernel, "fad_kad_sweep"));
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kad_sweep (x)"));
    FAD_TRY(check_rows(y, m, ldy, d, dtype, "fad_kad_sweep (y)"));
    FAD_TRY(check_bandwidths(bandwidths, n_bw, relative, "fad_kad_sweep", false));
    Ctx cx;
    FAD_TRY(cx.open(dtype, kernel, device, stream));

    Packed px, py;
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    FAD_TRY(pack_set(cx, 1, y, m, ldy, d, on_device, &py));
    double sigma[FAD_KAD_MAX_BANDWIDTHS], sums[3 * FAD_KAD_MAX_BANDWIDTHS];
    float c[FAD_KAD_MAX_BANDWIDTHS];
    FAD_TRY(resolve_sigmas(cx, px, bandwidths, n_bw, relative, "fad_kad_sweep", false, sigma, c));
    for (int b0 = 0; b0 < n_bw; b0 += kSweepGroup)
        FAD_TRY(kad_three_passes(cx, px, py, c + b0, std::min(kSweepGroup, n_bw - b0), sums + 3 * b0));
    for (int b = 0; b < n_bw; ++b)             // only now: a refusal above leaves `out` as it was
        fill_result(&out[b], 2.0 * sums[3 * b], 2.0 * sums[3 * b + 1], sums[3 * b + 2], n, m, sigma[b]);
    return FAD_OK;
}


int fad_kad_individual(const void* x, int64_t n, int64_t ldx, const void* rows, int64_t n_rows, int64_t ldy, const int64_t* offsets,
                       int64_t n_songs, int64_t d, int dtype, int on_device, double bandwidth, fad_kad_result_t* base, double* out_mmd2,
                       double* out_kyy_mean, double* out_kxy_mean, int32_t* out_status, int device, void* stream) {
    return fad_kad_individual_k(x, n, ldx, rows, n_rows, ldy, offsets, n_songs, d, dtype, on_device, bandwidth, FAD_KAD_GAUSSIAN, base,
                                out_mmd2, out_kyy_mean, out_kxy_mean, out_status, device, stream);
}

int fad_kad_individual_k(const void* x, int64_t n, int64_t ldx, const void* rows, int64_t n_rows, int64_t ldy, const int64_t* offsets,
                         int64_t n_songs, int64_t d, int dtype, int on_device, double bandwidth, int kernel, fad_kad_result_t* base,
                         double* out_mmd2, double* out_kyy_mean, double* out_kxy_mean, int32_t* out_status, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!base) return set_error(FAD_ERR_INVALID, "fad_kad_individual: NULL output");
    FAD_TRY(check_kernel(kernel, "fad_kad_individual"));
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kad_individual (x)"));
    if (n_songs < 0 || n_songs > INT32_MAX) return set_error(FAD_ERR_INVALID, "fad_kad_individual: %lld songs", (long long)n_songs);
    if (!offsets || (n_songs > 0 && (!out_mmd2 || !out_kyy_mean || !out_kxy_mean || !out_status)))
        return set_error(FAD_ERR_INVALID, "fad_kad_individual: NULL offsets or per-song output");
    if (n_rows < 0 || n_rows > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "fad_kad_individual: %lld song rows (at most %d)", (long long)n_rows, INT32_MAX - kTile);
    if (n_rows > 0 && !rows) return set_error(FAD_ERR_INVALID, "fad_kad_individual: NULL song rows");
    if (n_rows > 0 && ldy < d) return set_error(FAD_ERR_INVALID, "fad_kad_individual: song row pitch %lld < D = %lld", (long long)ldy, (long long)d);
    if (offsets[0] != 0 || offsets[n_songs] != n_rows)
        return set_error(FAD_ERR_INVALID, "fad_kad_individual: offsets run from %lld to %lld, not 0 to %lld", (long long)offsets[0],
                         (long long)offsets[n_songs], (long long)n_rows);
    for (int64_t s = 0; s < n_songs; ++s)
        if (offsets[s + 1] < offsets[s]) return set_error(FAD_ERR_INVALID, "fad_kad_individual: offsets decrease at song %lld", (long long)s);
    if (std::isnan(bandwidth) || std::isinf(bandwidth))
        return set_error(FAD_ERR_INVALID, "fad_kad_individual: bandwidth %g is not finite", bandwidth);
    Ctx cx;
    FAD_TRY(cx.open(dtype, kernel, device, stream));
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;

    // the baseline: sigma and Kxx exactly as fad_kad finds them (the same launches, slots and fixed-order sum)
    Packed px;
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    double sigma;
    float c;
    FAD_TRY(resolve_sigma(cx, px, bandwidth, "fad_kad_individual", &sigma, &c));
    const PassArgs xx[1] = {pass_args(px, px, true, c)};
    double* sxx_d = static_cast<double*>(ws.small.p) + 16;
    FAD_TRY(kad_sum_passes(cx, xx, sxx_d));

    // the songs: cross pass (X x Y) and band pass (pairs inside each song), per-column slots, one reduction per song
    if (n_rows > 0 && n_songs > 0) {
        Packed py;
        FAD_TRY(pack_image(cx, 1, rows, n_rows, ldy, d, on_device, &py));
        const bool f32 = dtype == FAD_F32;
        const int64_t depth = px.pitch / (int64_t)dtype_size(dtype), TI = kad::blocks(n), TJ = kad::blocks(n_rows), m_pad = TJ * kTile;
        const int64_t rr = kad::cross_rows_per_unit(TI, TJ, kad::tiles_per_launch(depth, f32)), NR = kad::cross_ranges(TI, rr);
        std::vector<kad::Unit> bunits;
        std::vector<int64_t> bstart;
        kad::band_units(offsets, n_songs, &bunits, &bstart);
        const int64_t U = (int64_t)bunits.size();

        // song tables and outputs, one buffer: offsets | band_start | band units | row_end | kyy | kxy | status
        Carve cv;
        const auto off_r = cv.add<int64_t>(n_songs + 1), bstart_r = cv.add<int64_t>(TJ + 1);
        const auto bunits_r = cv.add<kad::Unit>(U);
        const auto row_end_r = cv.add<int>(m_pad);
        const auto kyy_r = cv.add<double>(n_songs), kxy_r = cv.add<double>(n_songs);
        const auto status_r = cv.add<int>(n_songs);
        FAD_TRY(cv.reserve(ws.songs));
        FAD_TRY(ws.cross.reserve((size_t)(NR * m_pad) * sizeof(double)));
        FAD_TRY(ws.band.reserve((size_t)(U * kTile) * sizeof(double)));
        int64_t* off_d = cv.ptr(off_r);
        int64_t* bstart_d = cv.ptr(bstart_r);
        kad::Unit* bunits_d = cv.ptr(bunits_r);
        int* row_end_d = cv.ptr(row_end_r);
        double* kyy_d = cv.ptr(kyy_r);
        double* kxy_d = cv.ptr(kxy_r);
        int* status_d = cv.ptr(status_r);
        FAD_HIP_TRY(hipMemcpyAsync(off_d, offsets, (size_t)(n_songs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        FAD_HIP_TRY(hipMemcpyAsync(bstart_d, bstart.data(), bstart.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        FAD_HIP_TRY(hipMemcpyAsync(bunits_d, bunits.data(), bunits.size() * sizeof(kad::Unit), hipMemcpyHostToDevice, st));
        kad_row_end_kernel<<<(unsigned)cdiv(m_pad, 256), 256, 0, st>>>(off_d, n_songs, n_rows, m_pad, row_end_d);
        FAD_HIP_TRY(hipGetLastError());

        ColArgs p{};
        p.b = py.img; p.hb = py.h; p.pitch = px.pitch; p.nchunks = px.nchunks; p.c = c;
        p.a = px.img; p.ha = px.h; p.TI = TI; p.TJ = TJ; p.rr = rr;
        p.slots = static_cast<double*>(ws.cross.p); p.slot_pitch = m_pad;
        for (const kad::Launch& l : kad::launches(NR * TJ, kad::units_per_launch(rr, depth, f32), grid_cap(device))) {
            p.u0 = l.u0; p.cnt = l.cnt;
            FAD_TRY(with_dtype_kernel(dtype, kernel, [&](auto dt, auto kf) {
                kad_cols_kernel<dt, false, kf><<<(unsigned)l.grid, kThreads, kLdsCols, st>>>(p);
            }));
        }
        p.a = py.img; p.ha = py.h; p.units = bunits_d; p.row_end = row_end_d;
        p.slots = static_cast<double*>(ws.band.p); p.slot_pitch = kTile;
        for (const kad::Launch& l : kad::launches(U, kad::units_per_launch(kad::kBandPiece, depth, f32), grid_cap(device))) {
            p.u0 = l.u0; p.cnt = l.cnt;
            FAD_TRY(with_dtype_kernel(dtype, kernel, [&](auto dt, auto kf) {
                kad_cols_kernel<dt, true, kf><<<(unsigned)l.grid, kThreads, kLdsCols, st>>>(p);
            }));
        }
        kad_song_reduce_kernel<<<(unsigned)n_songs, 256, 0, st>>>(static_cast<const double*>(ws.cross.p), NR, m_pad,
                                                                  static_cast<const double*>(ws.band.p), bstart_d, py.h, off_d, (double)n,
                                                                  kyy_d, kxy_d, status_d);
        FAD_HIP_TRY(hipGetLastError());
        FAD_HIP_TRY(hipMemcpyAsync(out_kyy_mean, kyy_d, (size_t)n_songs * sizeof(double), hipMemcpyDeviceToHost, st));
        FAD_HIP_TRY(hipMemcpyAsync(out_kxy_mean, kxy_d, (size_t)n_songs * sizeof(double), hipMemcpyDeviceToHost, st));
        FAD_HIP_TRY(hipMemcpyAsync(out_status, status_d, (size_t)n_songs * sizeof(int), hipMemcpyDeviceToHost, st));
    } else {
        for (int64_t s = 0; s < n_songs; ++s) {                  // no song rows at all: every song is empty
            out_kyy_mean[s] = out_kxy_mean[s] = NAN;
            out_status[s] = FAD_ERR_TOO_FEW_ROWS;
        }
    }
    double sxx;
    FAD_HIP_TRY(hipMemcpyAsync(&sxx, sxx_d, sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));

    base->kxx_mean = 2.0 * sxx / ((double)n * (double)(n - 1));
    base->kyy_mean = base->kxy_mean = base->mmd2 = NAN;
    base->bandwidth = sigma;
    base->n = n;
    base->m = n_rows;
    for (int64_t s = 0; s < n_songs; ++s)
        out_mmd2[s] = out_status[s] == FAD_OK ? base->kxx_mean + out_kyy_mean[s] - 2.0 * out_kxy_mean[s] : NAN;
    return FAD_OK;
}

int fad_kad_uncertainty(const void* x, int64_t n, int64_t ldx, const void* const* ys, const int64_t* ms, const int64_t* ldys, int n_sets,
                        int64_t d, int dtype, int on_device, double bandwidth, fad_kad_result_t* out, double* cov, double* proj_x,
                        double* proj_y, int device, void* stream) {
    return fad_kad_uncertainty_k(x, n, ldx, ys, ms, ldys, n_sets, d, dtype, on_device, bandwidth, FAD_KAD_GAUSSIAN, out, cov, proj_x, proj_y,
                                 device, stream);
}

int fad_kad_uncertainty_k(const void* x, int64_t n, int64_t ldx, const void* const* ys, const int64_t* ms, const int64_t* ldys, int n_sets,
                          int64_t d, int dtype, int on_device, double bandwidth, int kernel, fad_kad_result_t* out, double* cov,
                          double* proj_x, double* proj_y, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!out || !cov) return set_error(FAD_ERR_INVALID, "fad_kad_uncertainty: NULL output");
    FAD_TRY(check_kernel(kernel, "fad_kad_uncertainty"));
    if (n_sets < 1 || n_sets > kad::kUncMaxSets)
        return set_error(FAD_ERR_INVALID, "fad_kad_uncertainty: %d evaluation sets (1 .. %d)", n_sets, kad::kUncMaxSets);
    if (!ys || !ms || !ldys) return set_error(FAD_ERR_INVALID, "fad_kad_uncertainty: NULL set table");
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kad_uncertainty (x)"));
    for (int s = 0; s < n_sets; ++s) FAD_TRY(check_rows(ys[s], ms[s], ldys[s], d, dtype, "fad_kad_uncertainty (a set)"));
    if (std::isnan(bandwidth) || std::isinf(bandwidth))
        return set_error(FAD_ERR_INVALID, "fad_kad_uncertainty: bandwidth %g is not finite", bandwidth);
    Ctx cx;
    FAD_TRY(cx.open(dtype, kernel, device, stream));
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;
    const int S = n_sets;

    // Z: X, then every set from a tile boundary, in one image (kad_unc_tiles.h)
    UncSets q{};
    q.n = n; q.S = S;
    const std::vector<int64_t> blk = kad::unc_blocks(n, ms, S);
    q.TX = blk[0];
    q.yoff[0] = 0;
    for (int s = 0; s < S; ++s) { q.blk[s] = blk[(size_t)s]; q.m[s] = ms[s]; q.yoff[s + 1] = q.yoff[s] + ms[s]; }
    q.blk[S] = blk[(size_t)S];
    const int64_t TZ = q.blk[S], z_pad = TZ * kTile, M = q.yoff[S];
    std::vector<RowSet> sets;
    sets.push_back(RowSet{x, n, ldx, 0, kad::blocks(n) * kTile});
    for (int s = 0; s < S; ++s) sets.push_back(RowSet{ys[s], ms[s], ldys[s], q.blk[s] * kTile, kad::blocks(ms[s]) * kTile});
    Packed px;
    FAD_TRY(pack_sets(cx, sets.data(), S + 1, d, on_device, z_pad, true, &px));
    double* info_d = static_cast<double*>(ws.small.p) + 1024;                          // [2 (S + 1)]: norm sum, non-finite rows
    std::vector<double> info((size_t)(2 * (S + 1)));
    FAD_HIP_TRY(hipMemcpyAsync(info.data(), info_d, info.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    for (int s = -1; s < S; ++s)
        if (info[(size_t)(2 * (s + 1) + 1)] != 0.0)
            return set_error(FAD_ERR_NOT_FINITE, "KAD: %lld of %lld rows of %s have a NaN/Inf norm", (long long)info[(size_t)(2 * (s + 1) + 1)],
                             (long long)(s < 0 ? n : ms[s]), s < 0 ? "the baseline" : "an evaluation set");

    px.n = n;                                  // the baseline is the image's first rows
    px.norm_sum = info[0];
    double sigma;
    float c;
    FAD_TRY(resolve_sigma(cx, px, bandwidth, "fad_kad_uncertainty", &sigma, &c));

    // the pass: units, slots and per-row tables
    const bool f32 = dtype == FAD_F32;
    const int64_t dp = depth_elems(d, dtype);
    Carve cv;
    const ColPlan cp = col_plan(cx, blk, dp, &cv);
    const int64_t W = std::min<int64_t>(256, cdiv(n, kUncCovRows)), P = (int64_t)S * S;

    // units | seg_start | a [S n] | b [M] | rxx [n] | ryy [M] | ryx [M] | stats [5 S + 1] | cov partials [W P] | cov sums [P]
    const auto a_r = cv.add<double>(S * n), b_r = cv.add<double>(M), rxx_r = cv.add<double>(n), ryy_r = cv.add<double>(M);
    const auto ryx_r = cv.add<double>(M), stats_r = cv.add<double>(5 * S + 1), part_r = cv.add<double>(W * P), covs_r = cv.add<double>(P);
    FAD_TRY(cv.reserve(ws.unc));
    FAD_TRY(ws.unc_slots.reserve((size_t)(cp.U * kTile) * sizeof(double)));
    int64_t* seg_d = cv.ptr(cp.seg_r);
    double* a_d = cv.ptr(a_r);
    double* b_d = cv.ptr(b_r);
    double* rxx_d = cv.ptr(rxx_r);
    double* ryy_d = cv.ptr(ryy_r);
    double* ryx_d = cv.ptr(ryx_r);
    double* stats_d = cv.ptr(stats_r);
    double* part_d = cv.ptr(part_r);
    double* covs_d = cv.ptr(covs_r);

    ColArgs p;
    FAD_TRY(col_pass_args(cx, cp, cv, px, &p));
    p.c = c;
    for (const kad::Launch& l : kad::launches(cp.U, kad::unc_units_per_launch(cp.rr, dp, f32), grid_cap(device))) {
        p.u0 = l.u0; p.cnt = l.cnt;
        FAD_TRY(with_dtype_kernel(dtype, kernel, [&](auto dt, auto kf) {
            kad_unc_cols_kernel<dt, kf><<<(unsigned)l.grid, kThreads, kLdsUnc, st>>>(p);
        }));
    }
    kad_unc_rows_kernel<<<(unsigned)cdiv(z_pad, 256), 256, 0, st>>>(p.slots, seg_d, q, a_d, b_d, rxx_d, ryy_d, ryx_d);
    FAD_HIP_TRY(hipGetLastError());
    kad_unc_sets_kernel<<<(unsigned)(S + 1), 256, 0, st>>>(a_d, b_d, rxx_d, ryy_d, ryx_d, q, stats_d);
    FAD_HIP_TRY(hipGetLastError());
    kad_unc_cov_kernel<<<dim3((unsigned)W, (unsigned)cdiv(P, 256)), 256, 0, st>>>(a_d, stats_d, q, part_d);
    FAD_HIP_TRY(hipGetLastError());
    kad_unc_cov_sum_kernel<<<(unsigned)cdiv(P, 256), 256, 0, st>>>(part_d, W, (int)P, covs_d);
    FAD_HIP_TRY(hipGetLastError());

    std::vector<double> stats((size_t)(5 * S + 1)), covs((size_t)P);
    FAD_HIP_TRY(hipMemcpyAsync(stats.data(), stats_d, stats.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(covs.data(), covs_d, covs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (proj_x) FAD_HIP_TRY(hipMemcpyAsync(proj_x, a_d, (size_t)(S * n) * sizeof(double), hipMemcpyDeviceToHost, st));
    if (proj_y) FAD_HIP_TRY(hipMemcpyAsync(proj_y, b_d, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));

    const double nd = (double)n, cov_x = 4.0 / (nd * (nd - 1.0));
    for (int s = 0; s < S; ++s) {
        const double* t = stats.data() + 5 * s;
        const double md = (double)ms[s];
        fill_result(&out[s], stats[(size_t)(5 * S)], t[3], t[4], n, ms[s], sigma);
        out[s].mmd2 = t[0] + t[1];             // as kad_unc_sets_kernel forms it, not from the means
        for (int u = 0; u < S; ++u) cov[s * S + u] = cov_x * covs[(size_t)(s * S + u)];
        cov[s * S + s] += 4.0 / (md * (md - 1.0)) * t[2];
    }
    return FAD_OK;
}

int fad_prdc(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device, int k,
             fad_prdc_result_t* out, fad_prdc_detail_t* detail, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!out) return set_error(FAD_ERR_INVALID, "fad_prdc: NULL output");
    if (k < 1 || k > kMaxK) return set_error(FAD_ERR_INVALID, "fad_prdc: k = %d is outside 1 .. %d", k, kMaxK);
    if (!x || !y) return set_error(FAD_ERR_INVALID, "fad_prdc: NULL rows");
    // dtype, d and ld as fad_kad checks them; the row counts are checked against k below
    FAD_TRY(check_rows(x, std::max<int64_t>(n, 2), ldx, d, dtype, "fad_prdc (x)"));
    FAD_TRY(check_rows(y, std::max<int64_t>(m, 2), ldy, d, dtype, "fad_prdc (y)"));
    if (n <= k || m <= k)
        return set_error(FAD_ERR_TOO_FEW_ROWS, "fad_prdc: k = %d needs more than k rows per set, got %lld and %lld", k, (long long)n,
                         (long long)m);
    if (n > INT32_MAX - kTile || m > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "fad_prdc: %lld and %lld rows (at most %d per set)", (long long)n, (long long)m, INT32_MAX - kTile);
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;

    Packed px, py;
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    FAD_TRY(pack_set(cx, 1, y, m, ldy, d, on_device, &py));
    const PrdcPlan qx = prdc_plan(cx, px, px, kad::kTopkEpilogue), qy = prdc_plan(cx, py, py, kad::kTopkEpilogue);
    const PrdcPlan qc = prdc_plan(cx, px, py, kad::kFlagEpilogue);
    const int64_t n_pad = qx.TJ * kTile, m_pad = qy.TJ * kTile;

    // radii x | radii y | flags | balls | totals | count slots
    Carve cv;
    const auto r2x_r = cv.add<float>(n_pad), r2y_r = cv.add<float>(m_pad);
    const auto flags_r = cv.add<int>(n_pad), balls_r = cv.add<int>(m_pad);
    const auto totals_r = cv.add<unsigned long long>(4);
    const auto counts_r = cv.add<int>(qc.NR * m_pad);
    FAD_TRY(cv.reserve(ws.prdc));
    FAD_TRY(ws.lists.reserve((size_t)std::max(qx.NR * n_pad, qy.NR * m_pad) * (size_t)k * sizeof(float)));
    float* r2x = cv.ptr(r2x_r);
    float* r2y = cv.ptr(r2y_r);
    int* flags = cv.ptr(flags_r);
    int* balls = cv.ptr(balls_r);
    unsigned long long* totals = cv.ptr(totals_r);
    float* lists = static_cast<float*>(ws.lists.p);

    FAD_TRY(radius_pass(cx, px, k, lists, r2x));
    FAD_TRY(radius_pass(cx, py, k, lists, r2y));
    FAD_HIP_TRY(hipMemsetAsync(flags, 0, (size_t)n_pad * sizeof(int), st));

    PrdcArgs p{};
    p.a = px.img; p.ha = px.h; p.b = py.img; p.hb = py.h; p.pitch = px.pitch; p.nchunks = px.nchunks; p.k = k;
    p.TI = qc.TI; p.TJ = qc.TJ; p.rr = qc.rr; p.ra = r2x; p.rb = r2y;
    p.counts = cv.ptr(counts_r); p.count_pitch = m_pad; p.flags = flags;
    for (const kad::Launch& l : kad::launches(qc.NR * qc.TJ, qc.per_launch, grid_cap(device))) {
        p.u0 = l.u0; p.cnt = l.cnt;
        FAD_TRY(with_dtype(dtype, [&](auto dt) { prdc_cross_kernel<dt><<<(unsigned)l.grid, kThreads, kLdsCross, st>>>(p); }));
    }
    prdc_balls_kernel<<<(unsigned)cdiv(m, 256), 256, 0, st>>>(p.counts, qc.NR, m_pad, m, balls);
    FAD_HIP_TRY(hipGetLastError());
    prdc_stats_kernel<<<1, 1024, 0, st>>>(balls, m, flags, n, totals);
    FAD_HIP_TRY(hipGetLastError());

    unsigned long long tot[4];
    FAD_HIP_TRY(hipMemcpyAsync(tot, totals, sizeof(tot), hipMemcpyDeviceToHost, st));
    if (detail) {
        if (detail->radius2_x) FAD_HIP_TRY(hipMemcpyAsync(detail->radius2_x, r2x, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
        if (detail->radius2_y) FAD_HIP_TRY(hipMemcpyAsync(detail->radius2_y, r2y, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, st));
        if (detail->balls_y) FAD_HIP_TRY(hipMemcpyAsync(detail->balls_y, balls, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
        if (detail->flags_x) FAD_HIP_TRY(hipMemcpyAsync(detail->flags_x, flags, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    FAD_HIP_TRY(hipStreamSynchronize(st));

    out->precision = (double)tot[0] / (double)m;
    out->density = (double)tot[1] / ((double)k * (double)m);
    out->recall = (double)tot[2] / (double)n;
    out->coverage = (double)tot[3] / (double)n;
    out->n = n;
    out->m = m;
    out->k = k;
    return FAD_OK;
}

int fad_nearest(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device, int k,
                int authenticity, int32_t* index, float* dist2, float* nn_radius2, fad_nearest_result_t* out, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!out || !index || !dist2) return set_error(FAD_ERR_INVALID, "fad_nearest: NULL output");
    if (k < 1 || k > kMaxK) return set_error(FAD_ERR_INVALID, "fad_nearest: k = %d is outside 1 .. %d", k, kMaxK);
    if (!x || !y) return set_error(FAD_ERR_INVALID, "fad_nearest: NULL rows");
    // dtype, d and ld as fad_kad checks them; the row counts are checked below
    FAD_TRY(check_rows(x, std::max<int64_t>(n, 2), ldx, d, dtype, "fad_nearest (x)"));
    FAD_TRY(check_rows(y, std::max<int64_t>(m, 2), ldy, d, dtype, "fad_nearest (y)"));
    if (n < k || m < 1 || (authenticity && n < 2))
        return set_error(FAD_ERR_TOO_FEW_ROWS, "fad_nearest: k = %d%s needs n >= %d and m >= 1, got n = %lld, m = %lld", k,
                         authenticity ? " with authenticity" : "", authenticity ? std::max(k, 2) : k, (long long)n, (long long)m);
    if (n > INT32_MAX - kTile || m > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "fad_nearest: %lld and %lld rows (at most %d per set)", (long long)n, (long long)m, INT32_MAX - kTile);
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;

    Packed px, py;
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    FAD_TRY(pack_set(cx, 1, y, m, ldy, d, on_device, &py));
    const PrdcPlan qc = prdc_plan(cx, px, py, kad::kNearestEpilogue), qx = prdc_plan(cx, px, px, kad::kTopkEpilogue);
    const int64_t n_pad = qx.TJ * kTile, m_pad = qc.TJ * kTile;

    // index | dist2 | radii x | nn radii | copied
    Carve cv;
    const auto index_r = cv.add<int32_t>(m * k);
    const auto dist2_r = cv.add<float>(m * k), r2x_r = cv.add<float>(n_pad), nn_r2_r = cv.add<float>(m);
    const auto copied_r = cv.add<unsigned long long>(1);
    FAD_TRY(cv.reserve(ws.near));
    // the radius pass's float lists, then (stream-ordered) the cross pass's keys in the same buffer
    FAD_TRY(ws.lists.reserve(std::max((size_t)(qc.NR * m_pad * k) * sizeof(uint64_t),
                                      authenticity ? (size_t)(qx.NR * n_pad) * sizeof(float) : (size_t)0)));
    int32_t* index_d = cv.ptr(index_r);
    float* dist2_d = cv.ptr(dist2_r);
    float* r2x = cv.ptr(r2x_r);
    float* nn_r2 = cv.ptr(nn_r2_r);
    unsigned long long* copied_d = cv.ptr(copied_r);

    if (authenticity) FAD_TRY(radius_pass(cx, px, 1, static_cast<float*>(ws.lists.p), r2x));
    FAD_TRY(nearest_pass(cx, px, py, false, k, static_cast<uint64_t*>(ws.lists.p), index_d, dist2_d));
    unsigned long long copied = 0;
    if (authenticity) {
        FAD_HIP_TRY(hipMemsetAsync(copied_d, 0, sizeof(unsigned long long), st));
        nearest_copied_kernel<<<(unsigned)cdiv(m, 256), 256, 0, st>>>(index_d, dist2_d, k, m, r2x, n, nn_r2, copied_d);
        FAD_HIP_TRY(hipGetLastError());
        FAD_HIP_TRY(hipMemcpyAsync(&copied, copied_d, sizeof(copied), hipMemcpyDeviceToHost, st));
        if (nn_radius2) FAD_HIP_TRY(hipMemcpyAsync(nn_radius2, nn_r2, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    FAD_HIP_TRY(hipMemcpyAsync(index, index_d, (size_t)(m * k) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipMemcpyAsync(dist2, dist2_d, (size_t)(m * k) * sizeof(float), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));

    out->authenticity = authenticity ? 1.0 - (double)copied / (double)m : NAN;
    out->copied = authenticity ? (int64_t)copied : -1;
    out->n = n;
    out->m = m;
    out->k = k;
    return FAD_OK;
}

int fad_nn_test(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device, int k,
                const uint32_t* labels, int64_t n_perm, int labels_on_device, fad_nn_test_result_t* out, int64_t* null_correct_x,
                int64_t* null_correct_y, int32_t* index, float* dist2, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!out || !null_correct_x || !null_correct_y) return set_error(FAD_ERR_INVALID, "fad_nn_test: NULL output");
    if (k < 1 || k > nnv::kMaxVotes || k % 2 == 0)
        return set_error(FAD_ERR_INVALID, "fad_nn_test: k = %d must be odd and in 1 .. %d", k, nnv::kMaxVotes);
    FAD_TRY(perm_check_args(x, n, ldx, y, m, ldy, d, dtype, labels, n_perm));
    if (k > n + m - 1)
        return set_error(FAD_ERR_INVALID, "fad_nn_test: k = %d needs at least k + 1 pooled rows, got %lld", k, (long long)(n + m));
    FAD_TRY(perm_check_labels(n, m, labels, n_perm, labels_on_device));
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;

    PermPrep pp;
    FAD_TRY(perm_prepare(cx, x, n, ldx, y, m, ldy, d, on_device, labels, n_perm, labels_on_device, &pp));
    const int64_t N = pp.N, z_pad = pp.z_pad, NL = pp.NL, W = pp.W;
    const Packed& pz = pp.z;
    const PrdcPlan q = prdc_plan(cx, pz, pz, kad::kNearestEpilogue);

    // index | dist2 | counts [32 W][2]
    Carve cv;
    const auto index_r = cv.add<int32_t>(N * k);
    const auto dist2_r = cv.add<float>(N * k);
    const auto counts_r = cv.add<unsigned long long>(64 * W);
    FAD_TRY(cv.reserve(ws.near));
    FAD_TRY(ws.lists.reserve((size_t)(q.NR * z_pad * k) * sizeof(uint64_t)));
    int32_t* index_d = cv.ptr(index_r);
    float* dist2_d = cv.ptr(dist2_r);
    unsigned long long* counts_d = cv.ptr(counts_r);

    // the graph (it never sees a label), then every labelling's votes on it
    FAD_TRY(nearest_pass(cx, pz, pz, true, k, static_cast<uint64_t*>(ws.lists.p), index_d, dist2_d));
    FAD_HIP_TRY(hipMemsetAsync(counts_d, 0, (size_t)(64 * W) * sizeof(unsigned long long), st));
    nnv::nn_vote_kernel<<<dim3((unsigned)cdiv(N, nnv::kVoteRows), (unsigned)W), 256, 0, st>>>(pp.cols_d, z_pad, index_d, k, N, counts_d);
    FAD_HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> counts((size_t)(2 * NL));
    FAD_HIP_TRY(hipMemcpyAsync(counts.data(), counts_d, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (index) FAD_HIP_TRY(hipMemcpyAsync(index, index_d, (size_t)(N * k) * sizeof(int32_t), back, st));
    if (dist2) FAD_HIP_TRY(hipMemcpyAsync(dist2, dist2_d, (size_t)(N * k) * sizeof(float), back, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));

    const int64_t cx0 = (int64_t)counts[0], cy0 = (int64_t)counts[1], c0 = cx0 + cy0;
    int64_t ge = 0, le = 0;
    for (int64_t p = 0; p < n_perm; ++p) {
        const int64_t cx = (int64_t)counts[(size_t)(2 * (p + 1))], cy = (int64_t)counts[(size_t)(2 * (p + 1) + 1)];
        null_correct_x[p] = cx;
        null_correct_y[p] = cy;
        ge += cx + cy >= c0;
        le += cx + cy <= c0;
    }
    out->accuracy = (double)c0 / (double)N;
    out->accuracy_x = (double)cx0 / (double)n;
    out->accuracy_y = (double)cy0 / (double)m;
    out->p_value = (double)(1 + ge) / (double)(n_perm + 1);
    out->p_value_low = (double)(1 + le) / (double)(n_perm + 1);
    out->correct_x = cx0;
    out->correct_y = cy0;
    out->n = n;
    out->m = m;
    out->k = k;
    return FAD_OK;
}

int fad_kad_permutation_test(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                             int on_device, double bandwidth, const uint32_t* labels, int64_t n_perm, int labels_on_device,
                             fad_kad_result_t* observed, double* null_out, double* p_value, int device, void* stream) {
    return fad_kad_permutation_test_k(x, n, ldx, y, m, ldy, d, dtype, on_device, bandwidth, FAD_KAD_GAUSSIAN, labels, n_perm,
                                      labels_on_device, observed, null_out, p_value, device, stream);
}

int fad_kad_permutation_test_k(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                               int on_device, double bandwidth, int kernel, const uint32_t* labels, int64_t n_perm, int labels_on_device,
                               fad_kad_result_t* observed, double* null_out, double* p_value, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!observed || !null_out || !p_value) return set_error(FAD_ERR_INVALID, "fad_kad_permutation_test: NULL output");
    FAD_TRY(check_kernel(kernel, "fad_kad_permutation_test"));
    FAD_TRY(perm_check_args(x, n, ldx, y, m, ldy, d, dtype, labels, n_perm));
    if (std::isnan(bandwidth) || std::isinf(bandwidth))
        return set_error(FAD_ERR_INVALID, "fad_kad_permutation_test: bandwidth %g is not finite", bandwidth);
    FAD_TRY(perm_check_labels(n, m, labels, n_perm, labels_on_device));
    Ctx cx;
    FAD_TRY(cx.open(dtype, kernel, device, stream));

    PermPrep pp;
    FAD_TRY(perm_prepare(cx, x, n, ldx, y, m, ldy, d, on_device, labels, n_perm, labels_on_device, &pp));
    // sigma: the given one, or the median pairwise distance of Z (fad_kad_median_distance on the pooled rows, bit for bit)
    double sigma;
    float c;
    FAD_TRY(resolve_sigma(cx, pp.z, bandwidth, "fad_kad_permutation_test", &sigma, &c));

    // the shift: the kernel value at the median distance (t = 1/2: e^-1/2, 2/3 for iq, 1 / sqrt(1.5) for imq) under the default sigma;
    // the mean off-diagonal kernel value of Z, perm_run's own, under a given one
    const float at_median = kernel == FAD_KAD_IQ ? 0.66666666666666663f : kernel == FAD_KAD_IMQ ? 0.81649658092772603f : 0.60653065971263342f;
    std::vector<double> t;
    double obs[3];
    FAD_TRY(perm_run(cx, pp, 1, &c, bandwidth > 0 ? nullptr : &at_median, &t, obs));

    fill_result(observed, obs[0], obs[1], obs[2], n, m, sigma);
    observed->mmd2 = t[0];                     // as kad_perm_stats_kernel forms it, not from the means
    int64_t ge = 0;
    for (int64_t q = 0; q < n_perm; ++q) {
        null_out[q] = t[(size_t)q + 1];
        ge += t[(size_t)q + 1] >= t[0];
    }
    *p_value = (double)(1 + ge) / (double)(n_perm + 1);
    return FAD_OK;
}

int fad_kad_last_plan(int64_t out[5]) {
    using namespace fad;
    if (!out) return set_error(FAD_ERR_INVALID, "fad_kad_last_plan: NULL output");
    const kad::PlanTally& t = kad::plan_tally();
    out[0] = t.passes; out[1] = t.launches; out[2] = t.min_launches; out[3] = t.max_launches; out[4] = t.max_walk;
    return FAD_OK;
}

int fad_kad_aggregate(const double* t, int n_bw, int64_t n_lab, double* p_values, double* p_aggregated) {
    using namespace fad;
    if (!t || !p_values || !p_aggregated) return set_error(FAD_ERR_INVALID, "fad_kad_aggregate: NULL argument");
    if (n_bw < 1) return set_error(FAD_ERR_INVALID, "fad_kad_aggregate: %d bandwidths; at least 1", n_bw);
    if (n_lab < 2 || n_lab > kad::kPermMax + 1)
        return set_error(FAD_ERR_INVALID, "fad_kad_aggregate: %lld labellings (the observed one and 1 .. %lld more)", (long long)n_lab,
                         (long long)kad::kPermMax);
    kad::perm_aggregate(t, n_bw, n_lab, p_values, p_aggregated);
    return FAD_OK;
}

int fad_kad_permutation_sweep(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                              int on_device, const double* bandwidths, int n_bw, int relative, int kernel, const uint32_t* labels,
                              int64_t n_perm, int labels_on_device, fad_kad_result_t* observed, double* null_out, double* p_values,
                              double* p_aggregated, int device, void* stream) {
    using namespace fad;
    begin_entry();
    const char* who = "fad_kad_permutation_sweep";
    if (!observed || !null_out || !p_values || !p_aggregated) return set_error(FAD_ERR_INVALID, "%s: NULL output", who);
    if (!bandwidths) return set_error(FAD_ERR_INVALID, "%s: NULL bandwidths", who);
    if (n_bw < 1 || n_bw > FAD_KAD_PERM_MAX_BANDWIDTHS)
        return set_error(FAD_ERR_INVALID, "%s: %d bandwidths, outside 1 .. %d", who, n_bw, FAD_KAD_PERM_MAX_BANDWIDTHS);
    FAD_TRY(check_kernel(kernel, who));
    FAD_TRY(perm_check_args(x, n, ldx, y, m, ldy, d, dtype, labels, n_perm));
    FAD_TRY(check_bandwidths(bandwidths, n_bw, relative, who, true));
    FAD_TRY(perm_check_labels(n, m, labels, n_perm, labels_on_device));
    Ctx cx;
    FAD_TRY(cx.open(dtype, kernel, device, stream));

    PermPrep pp;
    FAD_TRY(perm_prepare(cx, x, n, ldx, y, m, ldy, d, on_device, labels, n_perm, labels_on_device, &pp));
    // sigma_b: the given ones, or factors of the median pairwise distance of Z (found once); c_b as fad_kad_sweep forms it
    const int B = n_bw;
    const int64_t NL = pp.NL;
    double sigma[FAD_KAD_PERM_MAX_BANDWIDTHS], obs[3 * FAD_KAD_PERM_MAX_BANDWIDTHS];
    float c[FAD_KAD_PERM_MAX_BANDWIDTHS];
    FAD_TRY(resolve_sigmas(cx, pp.z, bandwidths, B, relative, who, true, sigma, c));
    std::vector<double> t;
    FAD_TRY(perm_run(cx, pp, B, c, nullptr, &t, obs));

    for (int b = 0; b < B; ++b) {              // only now: a refusal above leaves the outputs as they were
        fill_result(&observed[b], obs[3 * b], obs[3 * b + 1], obs[3 * b + 2], n, m, sigma[b]);
        observed[b].mmd2 = t[(size_t)(b * NL)];                                        // as kad_perm_stats_kernel forms it
        for (int64_t q = 0; q < n_perm; ++q) null_out[b * n_perm + q] = t[(size_t)(b * NL + q + 1)];
    }
    kad::perm_aggregate(t.data(), B, NL, p_values, p_aggregated);
    return FAD_OK;
}

int fad_kid(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
            int degree, double gamma, double coef0, fad_kid_result_t* out, int device, void* stream) {
    using namespace fad;
    begin_entry();
    if (!out) return set_error(FAD_ERR_INVALID, "fad_kid: NULL output");
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kid (x)"));
    FAD_TRY(check_rows(y, m, ldy, d, dtype, "fad_kid (y)"));
    KidParams k;
    FAD_TRY(kid_params(degree, gamma, coef0, d, "fad_kid", &k));
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    FAD_TRY(reserve_small(*cx.ws));

    Packed px, py;
    const void* staged[2] = {nullptr, nullptr};
    FAD_TRY(kid_pack(cx, 0, x, n, ldx, d, on_device, nullptr, n, kad::blocks(n) * kTile, 1, &staged[0], &px));
    FAD_TRY(kid_pack(cx, 1, y, m, ldy, d, on_device, nullptr, m, kad::blocks(m) * kTile, 1, &staged[1], &py));

    // passes as fad_kad's: XX and YY over their triangles, XY over the rectangle with the larger set as the row operand; launches, slots
    // and sum are sum_passes' own, with kid_pass_kernel in kad_pass_kernel's place
    const bool x_rows = n >= m;
    const PassArgs passes[3] = {pass_args(px, px, true, 0.f), pass_args(py, py, true, 0.f), pass_args(x_rows ? px : py, x_rows ? py : px, false, 0.f)};
    double* sums_d = static_cast<double*>(cx.ws->small.p) + 16;
    FAD_TRY(sum_passes(cx, passes, sums_d, [&](const PassArgs& p, const kad::Launch& l) {
        const KidArgs a = kid_args(p, k);
        return with_dtype(dtype, [&](auto dt) { kid_pass_kernel<dt><<<(unsigned)l.grid, kThreads, kLdsSum, cx.st>>>(a); });
    }));
    double sums[3];
    FAD_HIP_TRY(hipMemcpyAsync(sums, sums_d, sizeof(sums), hipMemcpyDeviceToHost, cx.st));
    FAD_HIP_TRY(hipStreamSynchronize(cx.st));
    for (int q = 0; q < 3; ++q)
        if (!std::isfinite(sums[q]))
            return set_error(FAD_ERR_NOT_FINITE, "fad_kid: the kernel sum of %s is not finite (NaN/Inf rows, or (gamma a.b + coef0)^%d beyond float32)",
                             q == 0 ? "x-x" : q == 1 ? "y-y" : "x-y", degree);

    out->kxx_mean = 2.0 * sums[0] / ((double)n * (double)(n - 1));
    out->kyy_mean = 2.0 * sums[1] / ((double)m * (double)(m - 1));
    out->kxy_mean = sums[2] / ((double)n * (double)m);
    out->mmd2 = out->kxx_mean + out->kyy_mean - 2.0 * out->kxy_mean;
    out->gamma = (double)k.gamma;
    out->coef0 = (double)k.coef0;
    out->degree = degree;
    out->n = n;
    out->m = m;
    return FAD_OK;
}

int fad_kid_subsets(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                    int degree, double gamma, double coef0, const int32_t* index_x, const int32_t* index_y, int64_t n_subsets,
                    int64_t subset_size, int index_on_device, double* mmd2, double* terms, double* mean, double* std_out, int device,
                    void* stream) {
    using namespace fad;
    begin_entry();
    if (!mmd2 || !mean || !std_out) return set_error(FAD_ERR_INVALID, "fad_kid_subsets: NULL output");
    if (!index_x || !index_y) return set_error(FAD_ERR_INVALID, "fad_kid_subsets: NULL index");
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kid_subsets (x)"));
    FAD_TRY(check_rows(y, m, ldy, d, dtype, "fad_kid_subsets (y)"));
    KidParams k;
    FAD_TRY(kid_params(degree, gamma, coef0, d, "fad_kid_subsets", &k));
    const int64_t s = subset_size;
    if (s < 2) return set_error(FAD_ERR_TOO_FEW_ROWS, "fad_kid_subsets: a subset needs at least 2 rows, got %lld", (long long)s);
    if (s > std::min(n, m))
        return set_error(FAD_ERR_INVALID, "fad_kid_subsets: subset size %lld is larger than the smaller set (%lld rows)", (long long)s,
                         (long long)std::min(n, m));
    if (n_subsets < 1) return set_error(FAD_ERR_INVALID, "fad_kid_subsets: %lld subsets (at least 1)", (long long)n_subsets);
    if (n > INT32_MAX || m > INT32_MAX) return set_error(FAD_ERR_INVALID, "fad_kid_subsets: the index is 32-bit, at most %d rows per set", INT32_MAX);
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;

    // the index lists on the device, checked there before any row is read through them
    const int64_t count = n_subsets * s;
    const int32_t* ix = index_x;
    const int32_t* iy = index_y;
    if (!index_on_device) {
        FAD_TRY(ws.kid_index.reserve((size_t)(2 * count) * sizeof(int32_t)));
        int32_t* both = static_cast<int32_t*>(ws.kid_index.p);
        FAD_HIP_TRY(hipMemcpyAsync(both, index_x, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st));
        FAD_HIP_TRY(hipMemcpyAsync(both + count, index_y, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st));
        ix = both;
        iy = both + count;
    }
    // ws.kid: the bad-index count (32 doubles' room), then sums [3 S], mmd2 [S], terms [3 S], stats [2]
    FAD_TRY(ws.kid.reserve((size_t)(32 + 7 * n_subsets + 2) * sizeof(double)));
    unsigned long long* bad_d = static_cast<unsigned long long*>(ws.kid.p);
    double* sums_d = static_cast<double*>(ws.kid.p) + 32;
    double* mmd2_d = sums_d + 3 * n_subsets;
    double* terms_d = mmd2_d + n_subsets;
    double* stats_d = terms_d + 3 * n_subsets;
    FAD_HIP_TRY(hipMemsetAsync(bad_d, 0, sizeof(unsigned long long), st));
    kid_index_check_kernel<<<(unsigned)std::min<int64_t>(cdiv(count, 256), 1024), 256, 0, st>>>(ix, iy, count, n, m, bad_d);
    FAD_HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    FAD_HIP_TRY(hipMemcpyAsync(&bad, bad_d, sizeof(bad), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (bad) return set_error(FAD_ERR_INVALID, "fad_kid_subsets: %llu index entries are outside [0, %lld) of x or [0, %lld) of y", bad, (long long)n,
                              (long long)m);

    // the subsets in groups whose two images stay under kid::kImageBudget: gather-pack, one pass over the group's units, the units
    // of every (subset, block) summed in unit order
    const int64_t T = kad::blocks(s), img_rows = T * kTile, U = kid::units_per_subset(T);
    const int64_t row_bytes = depth_elems(d, dtype) * (int64_t)dtype_size(dtype);
    const int64_t per_launch = kad::tiles_per_launch(row_bytes / (int64_t)dtype_size(dtype), dtype == FAD_F32);
    const void* staged[2] = {nullptr, nullptr};
    for (const kid::Group& grp : kid::plan(n_subsets, s, row_bytes, kid::kImageBudget)) {
        Packed px, py;
        FAD_TRY(kid_pack(cx, 0, x, n, ldx, d, on_device, ix + grp.q0 * s, s, img_rows, grp.count, &staged[0], &px));
        FAD_TRY(kid_pack(cx, 1, y, m, ldy, d, on_device, iy + grp.q0 * s, s, img_rows, grp.count, &staged[1], &py));
        // ws.slots: the group's units, one float64 each, then the unit table the pass reads
        const int64_t total = grp.count * U;
        FAD_TRY(ws.slots.reserve((size_t)total * (sizeof(double) + sizeof(KidUnitRow))));
        KidArgs a = kid_args(pass_args(px, py, false, 0.f), k);
        a.units = static_cast<double*>(ws.slots.p);
        KidUnitRow* table = reinterpret_cast<KidUnitRow*>(a.units + total);
        kid_unit_table_kernel<<<(unsigned)cdiv(total, 256), 256, 0, st>>>(total, T, img_rows, table);
        FAD_HIP_TRY(hipGetLastError());
        for (const kad::Launch& l : kad::launches(total, per_launch, grid_cap(device))) {
            a.p.u0 = l.u0; a.p.cnt = l.cnt;
            FAD_TRY(with_dtype(dtype, [&](auto dt) { kid_units_kernel<dt><<<(unsigned)l.grid, kThreads, kLdsSum, st>>>(a, table); }));
        }
        kid_subset_sums_kernel<<<dim3((unsigned)grp.count, 3), 256, 0, st>>>(a.units, T, grp.q0, sums_d);
        FAD_HIP_TRY(hipGetLastError());
    }
    kid_stats_kernel<<<1, 256, 0, st>>>(sums_d, n_subsets, s, mmd2_d, terms_d, stats_d);
    FAD_HIP_TRY(hipGetLastError());
    std::vector<double> host((size_t)(7 * n_subsets + 2));
    FAD_HIP_TRY(hipMemcpyAsync(host.data(), sums_d, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    for (int64_t q = 0; q < n_subsets; ++q)
        for (int b = 0; b < 3; ++b)
            if (!std::isfinite(host[(size_t)(3 * q + b)]))
                return set_error(FAD_ERR_NOT_FINITE, "fad_kid_subsets: the kernel sum of %s of subset %lld is not finite (NaN/Inf rows, or "
                                 "(gamma a.b + coef0)^%d beyond float32)", b == 0 ? "x-x" : b == 1 ? "y-y" : "x-y", (long long)q, degree);

    const double* r = host.data() + 3 * n_subsets;            // only now: a refusal above leaves the outputs as they were
    for (int64_t q = 0; q < n_subsets; ++q) mmd2[q] = r[q];
    if (terms)
        for (int64_t q = 0; q < 3 * n_subsets; ++q) terms[q] = r[n_subsets + q];
    *mean = r[4 * n_subsets];
    *std_out = r[4 * n_subsets + 1];
    return FAD_OK;
}

int fad_sinkhorn(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                 double epsilon, int iterations, fad_sinkhorn_result_t* out, fad_sinkhorn_detail_t* detail, int device, void* stream) {
    using namespace fad;
    begin_entry();
    const char* who = "fad_sinkhorn";
    if (!out) return set_error(FAD_ERR_INVALID, "%s: NULL output", who);
    if (!x || !y) return set_error(FAD_ERR_INVALID, "%s: NULL rows", who);
    if (dtype == FAD_F64) return set_error(FAD_ERR_INVALID, "%s: float64 rows are not supported; cast to float32 (or float16 / bfloat16)", who);
    if (dtype != FAD_F16 && dtype != FAD_BF16 && dtype != FAD_F32) return set_error(FAD_ERR_INVALID, "%s: unknown dtype %d", who, dtype);
    if (d < 1 || d > 2048) return set_error(FAD_ERR_INVALID, "%s: D = %lld is outside 1 .. 2048", who, (long long)d);
    if (ldx < d || ldy < d) return set_error(FAD_ERR_INVALID, "%s: row pitch %lld / %lld < D = %lld", who, (long long)ldx, (long long)ldy, (long long)d);
    if (n < 1 || m < 1) return set_error(FAD_ERR_TOO_FEW_ROWS, "%s: needs at least 1 row per set, got %lld and %lld", who, (long long)n, (long long)m);
    if (n > INT32_MAX - kTile || m > INT32_MAX - kTile)
        return set_error(FAD_ERR_INVALID, "%s: %lld and %lld rows (at most %d per set)", who, (long long)n, (long long)m, INT32_MAX - kTile);
    if (iterations < 1 || iterations > 100000) return set_error(FAD_ERR_INVALID, "%s: %d iterations, outside 1 .. 100000", who, iterations);
    if (std::isnan(epsilon) || std::isinf(epsilon)) return set_error(FAD_ERR_INVALID, "%s: epsilon %g is not finite", who, epsilon);
    const bool by_median = !(epsilon > 0);
    if (by_median && n < 2)
        return set_error(FAD_ERR_TOO_FEW_ROWS, "%s: the default epsilon is taken from the median pairwise distance of x, which needs 2 rows", who);
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    KadWorkspace& ws = *cx.ws;
    const hipStream_t st = cx.st;

    // each set packed once: the two images serve every iteration of all three problems
    Packed px, py;
    FAD_TRY(pack_set(cx, 0, x, n, ldx, d, on_device, &px));
    FAD_TRY(pack_set(cx, 1, y, m, ldy, d, on_device, &py));
    double eps = epsilon;
    if (by_median) {
        double median;
        FAD_TRY(median_of_packed(cx, px, &median));
        if (!(median > 0))
            return set_error(FAD_ERR_INVALID, "%s: the median pairwise distance of x is %g, so there is no default epsilon -- are all rows of x "
                             "identical?", who, median);
        eps = (FAD_SINKHORN_BLUR_FACTOR * median) * (FAD_SINKHORN_BLUR_FACTOR * median);
    }
    const double cd = 1.4426950408889634 / eps;
    const float c = (float)cd;
    if (!(eps > 0) || !std::isfinite(eps) || !std::isfinite(c) || c == 0.f)
        return set_error(FAD_ERR_INVALID, "%s: epsilon %g is outside the float32 range of the kernel", who, eps);

    // problems: (x, y), (x, x), (y, y).  Per problem f, g and f' in float64 and h + f, h + g in float32; then 9 sums.
    const Packed* A[3] = {&px, &px, &py};
    const Packed* B[3] = {&py, &px, &py};
    Carve cv;
    Region<double> f_r[3], g_r[3], f2_r[3];
    Region<float> hpf_r[3], hpg_r[3];
    int64_t slots = 0;
    for (int q = 0; q < 3; ++q) {
        const int64_t a_pad = kad::blocks(A[q]->n) * kTile, b_pad = kad::blocks(B[q]->n) * kTile;
        f_r[q] = cv.add<double>(a_pad); g_r[q] = cv.add<double>(b_pad); f2_r[q] = cv.add<double>(a_pad);
        hpf_r[q] = cv.add<float>(a_pad); hpg_r[q] = cv.add<float>(b_pad);
    }
    const auto sums_r = cv.add<double>(9);
    FAD_TRY(cv.reserve(ws.sink));
    SoftminPlan plan_f[3], plan_g[3];
    for (int q = 0; q < 3; ++q) {
        plan_f[q] = softmin_plan(cx, *B[q], *A[q]);            // f: over the rows of B, for every row of A
        plan_g[q] = softmin_plan(cx, *A[q], *B[q]);
        slots = std::max({slots, plan_f[q].NR * plan_f[q].TJ * kTile, plan_g[q].NR * plan_g[q].TJ * kTile});
    }
    FAD_TRY(ws.sink_slots.reserve((size_t)slots * sizeof(float2)));

    double* sums_d = cv.ptr(sums_r);
    for (int q = 0; q < 3; ++q) {
        double* f = cv.ptr(f_r[q]);
        double* g = cv.ptr(g_r[q]);
        double* f2 = cv.ptr(f2_r[q]);
        float* hpf = cv.ptr(hpf_r[q]);
        float* hpg = cv.ptr(hpg_r[q]);
        for (int it = 0; it < iterations; ++it) {              // Gauss-Seidel from f = g = 0: g takes the new f
            FAD_TRY(softmin_pass(cx, plan_f[q], it == 0 ? B[q]->h : hpg, c, eps, f, hpf));
            FAD_TRY(softmin_pass(cx, plan_g[q], hpf, c, eps, g, hpg));
        }
        FAD_TRY(softmin_pass(cx, plan_f[q], hpg, c, eps, f2, nullptr));               // f', for the marginal error only
        sinkhorn_finish_kernel<<<1, 256, 0, st>>>(f, g, f2, A[q]->n, B[q]->n, 1.0 / eps, sums_d + 3 * q);
        FAD_HIP_TRY(hipGetLastError());
    }
    double sums[9];
    FAD_HIP_TRY(hipMemcpyAsync(sums, sums_d, sizeof(sums), hipMemcpyDeviceToHost, st));
    std::vector<double> fx, gx, fy, gy, fv, gv;
    auto fetch = [&](std::vector<double>* v, Region<double> r, int64_t count) {
        v->resize((size_t)count);
        return hipMemcpyAsync(v->data(), cv.ptr(r), (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st);
    };
    if (detail && (detail->f || detail->pot_x)) FAD_HIP_TRY(fetch(&fv, f_r[0], n));
    if (detail && (detail->g || detail->pot_y)) FAD_HIP_TRY(fetch(&gv, g_r[0], m));
    if (detail && detail->pot_x) { FAD_HIP_TRY(fetch(&fx, f_r[1], n)); FAD_HIP_TRY(fetch(&gx, g_r[1], n)); }
    if (detail && detail->pot_y) { FAD_HIP_TRY(fetch(&fy, f_r[2], m)); FAD_HIP_TRY(fetch(&gy, g_r[2], m)); }
    FAD_HIP_TRY(hipStreamSynchronize(st));
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(sums[q])) return set_error(FAD_ERR_NOT_FINITE, "%s: a potential is not finite (epsilon %g)", who, eps);

    double ot[3], err[3];                                      // only now: a refusal above leaves the outputs as they were
    for (int q = 0; q < 3; ++q) {
        ot[q] = sums[3 * q] / (double)A[q]->n + sums[3 * q + 1] / (double)B[q]->n;
        err[q] = sums[3 * q + 2] / (double)A[q]->n;
    }
    out->ot_xy = ot[0]; out->ot_xx = ot[1]; out->ot_yy = ot[2];
    out->divergence = ot[0] - 0.5 * ot[1] - 0.5 * ot[2];
    out->epsilon = eps;
    out->marginal_error = err[0]; out->marginal_error_xx = err[1]; out->marginal_error_yy = err[2];
    out->n = n; out->m = m; out->iterations = iterations;
    if (detail) {
        for (int64_t i = 0; detail->f && i < n; ++i) detail->f[i] = fv[(size_t)i];
        for (int64_t j = 0; detail->g && j < m; ++j) detail->g[j] = gv[(size_t)j];
        for (int64_t i = 0; detail->pot_x && i < n; ++i) detail->pot_x[i] = fv[(size_t)i] - 0.5 * (fx[(size_t)i] + gx[(size_t)i]);
        for (int64_t j = 0; detail->pot_y && j < m; ++j) detail->pot_y[j] = gv[(size_t)j] - 0.5 * (fy[(size_t)j] + gy[(size_t)j]);
    }
    return FAD_OK;
}

int fad_sliced_wasserstein(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                           const float* directions, int projections, fad_sliced_result_t* out, fad_sliced_detail_t* detail, int device,
                           void* stream) {
    using namespace fad;
    begin_entry();
    sliced_plan_value() = SlicedPlan{0, 0, 0, 0};
    const char* who = "fad_sliced_wasserstein";
    if (!out) return set_error(FAD_ERR_INVALID, "%s: NULL output", who);
    SlicedOut o{};
    if (detail) { o.values = detail->values; o.sorted_x = detail->sorted_x; o.sorted_y = detail->sorted_y; }
    return sliced_sets(who, x, n, ldx, y, m, ldy, d, dtype, on_device, directions, projections, out, o, device, stream);
}

int fad_sliced_shares(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                      const float* directions, int projections, fad_sliced_result_t* out, double* share_x, double* share_y,
                      fad_sliced_shares_detail_t* detail, int device, void* stream) {
    using namespace fad;
    begin_entry();
    sliced_plan_value() = SlicedPlan{0, 0, 0, 0};
    const char* who = "fad_sliced_shares";
    if (!out || !share_x || !share_y) return set_error(FAD_ERR_INVALID, "%s: NULL output", who);
    SlicedOut o{};
    o.shares = true; o.share_x = share_x; o.share_y = share_y;
    if (detail) {
        o.values = detail->values; o.sorted_x = detail->sorted_x; o.sorted_y = detail->sorted_y;
        o.index_x = detail->index_x; o.index_y = detail->index_y;
    }
    return sliced_sets(who, x, n, ldx, y, m, ldy, d, dtype, on_device, directions, projections, out, o, device, stream);
}

int fad_sliced_last_plan(int64_t out[4]) {
    using namespace fad;
    if (!out) return set_error(FAD_ERR_INVALID, "fad_sliced_last_plan: NULL output");
    const SlicedPlan& p = sliced_plan_value();
    out[0] = p.chunks; out[1] = p.lc; out[2] = p.passes; out[3] = p.share;
    return FAD_OK;
}

int fad_sliced_permutation_test(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                                int on_device, const float* directions, int projections, const uint32_t* labels, int64_t n_perm,
                                int labels_on_device, fad_sliced_permutation_result_t* out, double* null_out, double* null_max,
                                fad_sliced_permutation_detail_t* detail, int device, void* stream) {
    using namespace fad;
    begin_entry();
    sliced_perm_plan_value() = SlicedPermPlan{{0, 0, 0, 0, 0, 0}};
    const char* who = "fad_sliced_permutation_test";
    if (!out || !null_out || !null_max) return set_error(FAD_ERR_INVALID, "%s: NULL output", who);
    SlicedPermOut o{};
    if (detail) { o.values = detail->values; o.sorted_z = detail->sorted_z; o.index_z = detail->index_z; }
    return sliced_permutation(who, x, n, ldx, y, m, ldy, d, dtype, on_device, directions, projections, labels, n_perm, labels_on_device, out,
                              null_out, null_max, o, device, stream);
}

int fad_sliced_permutation_last_plan(int64_t out[6]) {
    using namespace fad;
    if (!out) return set_error(FAD_ERR_INVALID, "fad_sliced_permutation_last_plan: NULL output");
    const SlicedPermPlan& p = sliced_perm_plan_value();
    for (int i = 0; i < 6; ++i) out[i] = p.v[i];
    return FAD_OK;
}

int fad_sliced_bootstrap(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                         const float* directions, int projections, const uint8_t* counts_x, const uint8_t* counts_y, int64_t n_boot,
                         fad_sliced_bootstrap_result_t* out, double* boot, double* boot_max, fad_sliced_bootstrap_detail_t* detail,
                         int device, void* stream) {
    using namespace fad;
    begin_entry();
    sliced_boot_plan_value() = SlicedBootPlan{{0, 0, 0, 0, 0, 0}};
    const char* who = "fad_sliced_bootstrap";
    if (!out || !boot || !boot_max) return set_error(FAD_ERR_INVALID, "%s: NULL output", who);
    SlicedBootOut o{};
    if (detail) {
        o.values = detail->values; o.sorted_x = detail->sorted_x; o.index_x = detail->index_x;
        o.sorted_y = detail->sorted_y; o.index_y = detail->index_y; o.totals = detail->totals;
    }
    return sliced_bootstrap(who, x, n, ldx, y, m, ldy, d, dtype, on_device, directions, projections, counts_x, counts_y, n_boot, out, boot,
                            boot_max, o, device, stream);
}

int fad_sliced_bootstrap_last_plan(int64_t out[6]) {
    using namespace fad;
    if (!out) return set_error(FAD_ERR_INVALID, "fad_sliced_bootstrap_last_plan: NULL output");
    const SlicedBootPlan& p = sliced_boot_plan_value();
    for (int i = 0; i < 6; ++i) out[i] = p.v[i];
    return FAD_OK;
}

int fad_sliced_individual(const void* x, int64_t n, int64_t ldx, const void* rows, int64_t n_rows, int64_t ldy, const int64_t* offsets,
                          int64_t n_songs, int64_t d, int dtype, int on_device, const float* directions, int projections, double* out_sw2,
                          double* out_std_error, double* out_max_sliced, int64_t* out_max_index, int32_t* out_status,
                          fad_sliced_individual_detail_t* detail, int device, void* stream) {
    using namespace fad;
    begin_entry();
    sliced_song_plan_value() = SlicedSongPlan{{0, 0, 0, 0, 0, 0}};
    const char* who = "fad_sliced_individual";
    if (!out_sw2 || !out_std_error || !out_max_sliced || !out_max_index || !out_status)
        return set_error(FAD_ERR_INVALID, "%s: NULL per-song output", who);
    SlicedSongOut o{out_sw2, out_std_error, out_max_sliced, out_max_index, out_status, nullptr, nullptr, nullptr};
    if (detail) { o.values = detail->values; o.sorted_x = detail->sorted_x; o.sorted_rows = detail->sorted_rows; }
    return sliced_songs(who, x, n, ldx, rows, n_rows, ldy, offsets, n_songs, d, dtype, on_device, directions, projections, o, device, stream);
}

int fad_sliced_individual_last_plan(int64_t out[6]) {
    using namespace fad;
    if (!out) return set_error(FAD_ERR_INVALID, "fad_sliced_individual_last_plan: NULL output");
    const SlicedSongPlan& p = sliced_song_plan_value();
    for (int i = 0; i < 6; ++i) out[i] = p.v[i];
    return FAD_OK;
}

int fad_kmeans(const void* const* xs, const int64_t* ns, const int64_t* lds, int n_sets, int64_t d, int dtype, int on_device, int64_t k,
               const float* init, int max_iter, float* centroids, int32_t* labels, int64_t* counts, float* dist2, double* inertia_trace,
               fad_kmeans_result_t* out, int device, void* stream) {
    using namespace fad;
    begin_entry();
    kmeans_plan_value() = KmeansPlan{{0, 0, 0, 0, 0, 0}};
    if (!out || !centroids || !labels || !counts) return set_error(FAD_ERR_INVALID, "fad_kmeans: NULL output");
    if (!xs || !ns || !lds || !init) return set_error(FAD_ERR_INVALID, "fad_kmeans: NULL argument");
    if (n_sets < 1 || n_sets > kmeans::kMaxSets)
        return set_error(FAD_ERR_INVALID, "fad_kmeans: %d row sets (1 .. %d)", n_sets, kmeans::kMaxSets);
    if (max_iter < 0) return set_error(FAD_ERR_INVALID, "fad_kmeans: max_iter = %d is negative", max_iter);
    int64_t N = 0;
    RowSet sets[kmeans::kMaxSets];
    for (int i = 0; i < n_sets; ++i) {
        if (ns[i] < 1) return set_error(FAD_ERR_TOO_FEW_ROWS, "fad_kmeans: set %d has %lld rows", i, (long long)ns[i]);
        FAD_TRY(check_rows(xs[i], std::max<int64_t>(ns[i], 2), lds[i], d, dtype, "fad_kmeans"));
        if (ns[i] > INT32_MAX - kTile - N)
            return set_error(FAD_ERR_INVALID, "fad_kmeans: more than %d pooled rows", INT32_MAX - kTile);
        sets[i] = RowSet{xs[i], ns[i], lds[i], N, ns[i]};
        N += ns[i];
    }
    if (k < 1 || k > N || k > kmeans::kMaxClusters)
        return set_error(FAD_ERR_INVALID, "fad_kmeans: K = %lld is outside 1 .. min(N = %lld, %d)", (long long)k, (long long)N,
                         kmeans::kMaxClusters);
    for (int64_t i = 0; i < k * d; ++i)
        if (!std::isfinite(init[i]))
            return set_error(FAD_ERR_NOT_FINITE, "fad_kmeans: init centroid %lld has a NaN/Inf entry", (long long)(i / d));
    sets[n_sets - 1].r_pad = kad::blocks(N) * kTile - sets[n_sets - 1].r0;
    Ctx cx;
    FAD_TRY(cx.open(dtype, FAD_KAD_GAUSSIAN, device, stream));
    return kmeans_run(cx, sets, n_sets, N, d, on_device, k, init, max_iter, centroids, labels, counts, dist2, inertia_trace, out);
}

int fad_kmeans_last_plan(int64_t out[6]) {
    using namespace fad;
    if (!out) return set_error(FAD_ERR_INVALID, "fad_kmeans_last_plan: NULL output");
    const KmeansPlan& p = kmeans_plan_value();
    for (int i = 0; i < 6; ++i) out[i] = p.v[i];
    return FAD_OK;
}

}  // extern "C"
