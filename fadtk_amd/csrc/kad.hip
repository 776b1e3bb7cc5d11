// Kernel Audio Distance: the unbiased Gaussian-kernel MMD^2 between two sets of embedding rows, and the median pairwise distance
// of one set (the default bandwidth).  DESIGN.md 4.6.
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
// The cross pass always runs with the larger set (by rows, then by sum of row norms) as the row operand, so that swapping the
// arguments adds exactly the same tile sums.  KAD's code object is loaded at its first call, not by check_device's warm-up.
#include "fad_common.h"
#include "kad_tiles.h"

#include <algorithm>
#include <cmath>
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
    float c;                                   // log2(e) / sigma^2 (MODE_SUM)
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

// k(S') summed over the wave's 64 x 64 pairs of a tile; MASK: a diagonal tile of a triangle counts only column > row
template <bool MASK>
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
                // c > 0, so min(S', 0) * c == min(S' * c, 0).  The multiply is an ordinary VALU op that reads the MFMA result, so the
                // compiler places the MFMA -> VALU wait states before it; the clamp then reads only that VALU result.  (An inline-asm read
                // of the accumulator itself would get no wait states: the hazard recognizer does not look inside asm.)  The clamp is asm so
                // that no canonicalising v_max comes with it.
                float v = acc[bi][bj][g] * c, w;
                asm("v_min_f32 %0, 0, %1" : "=v"(w) : "v"(v));
                float e = __builtin_amdgcn_exp2f(w);
                if (MASK) e = (bj * 32 - bi * 32 - (g & 3) - 8 * (g >> 2)) > lrow ? e : 0.f;     // column > row
                s += e;
            }
    return s;
}

template <int DT, int MODE>
__global__ void __launch_bounds__(kThreads, 2) kad_pass_kernel(PassArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* la = lds;
    char* lb = lds + kOpBytes;
    float* lh = reinterpret_cast<float*>(lds + 2 * kOpBytes);                          // [0, 128): rows, [128, 256): columns
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
        const char* ga = p.a + t.I * kTile * p.pitch;
        const char* gb = p.b + t.J * kTile * p.pitch;

        __syncthreads();                                                              // the previous tile is done with LDS
        if (tid < kTile) lh[tid] = p.ha[t.I * kTile + tid];
        else lh[tid] = p.hb[t.J * kTile + tid - kTile];

        // global -> registers: 128 rows x 128 bytes per operand = 1024 pieces of 16 B, 4 per thread
        u32x4 ra[4], rb[4];
        auto load = [&](int ch) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = (tid >> 3) + 32 * q, col = (tid & 7) * 16;
                ra[q] = *reinterpret_cast<const u32x4*>(ga + row * p.pitch + ch * kChunk + col);
                rb[q] = *reinterpret_cast<const u32x4*>(gb + row * p.pitch + ch * kChunk + col);
            }
        };
        load(0);
        __syncthreads();

        f32x16 acc[2][2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                const float hc = lh[kTile + wn * 64 + bj * 32 + (lane & 31)];
#pragma unroll
                for (int g = 0; g < 16; ++g)
                    acc[bi][bj][g] = lh[wm * 64 + bi * 32 + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5)] + hc;
            }

        for (int ch = 0; ch < p.nchunks; ++ch) {
            if (ch) __syncthreads();                                                  // everybody is through the last chunk
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = (tid >> 3) + 32 * q, col = (tid & 7) * 16;
                *reinterpret_cast<u32x4*>(la + row * kLdsRow + col) = ra[q];
                *reinterpret_cast<u32x4*>(lb + row * kLdsRow + col) = rb[q];
            }
            __syncthreads();
            if (ch + 1 < p.nchunks) load(ch + 1);                                     // in flight under this chunk's MFMAs
            chunk_mfma<DT>(la + wm * 64 * kLdsRow, lb + wn * 64 * kLdsRow, lane, acc);
        }

        const int rbase = wm * 64, cbase = wn * 64;
        if (MODE == MODE_SUM) {
            const float s = (p.tri && t.I == t.J) ? tile_sum<true>(acc, p.c, rbase, cbase, lane) : tile_sum<false>(acc, p.c, rbase, cbase, lane);
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

// ------------------------------------------------------------------------------------------------------------------ host side
struct KadWorkspace {
    DevBuf raw[2], img[2], h[2], slots, small;       // small: info, pass offsets, pass sums, histograms
    void release_all() {
        for (int i = 0; i < 2; ++i) { raw[i].release(); img[i].release(); h[i].release(); }
        slots.release(); small.release();
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

// rows -> the set's padded image and h; reads back the norm sum and checks every norm is finite
static int pack_set(int slot, const void* x, int64_t n, int64_t ld, int64_t d, int dtype, int on_device, int device, hipStream_t st,
                    KadWorkspace& ws, Packed* out) {
    const size_t es = dtype_size(dtype);
    const int64_t dp = depth_elems(d, dtype), n_pad = kad::blocks(n) * kTile;
    if (!on_device) {
        FAD_TRY(ws.raw[slot].reserve((size_t)(n * d) * es));
        FAD_TRY(host_to_device_2d(ws.raw[slot].p, (size_t)d * es, x, (size_t)ld * es, (size_t)d * es, (size_t)n, device, st));
        x = ws.raw[slot].p;
        ld = d;
    }
    FAD_TRY(ws.img[slot].reserve((size_t)(n_pad * dp) * es));
    FAD_TRY(ws.h[slot].reserve((size_t)n_pad * sizeof(float)));
    FAD_TRY(ws.small.reserve(4096 * sizeof(double) + 2 * kHistBins * sizeof(unsigned long long)));
    float* h = static_cast<float*>(ws.h[slot].p);
    const dim3 grid((unsigned)cdiv(n_pad, 4));
    switch (dtype) {
        case FAD_F16: kad_pack_kernel<_Float16><<<grid, 256, 0, st>>>(static_cast<const _Float16*>(x), n, ld, d, static_cast<_Float16*>(ws.img[slot].p), dp, n_pad, h); break;
        case FAD_BF16: kad_pack_kernel<__bf16><<<grid, 256, 0, st>>>(static_cast<const __bf16*>(x), n, ld, d, static_cast<__bf16*>(ws.img[slot].p), dp, n_pad, h); break;
        default: kad_pack_kernel<float><<<grid, 256, 0, st>>>(static_cast<const float*>(x), n, ld, d, static_cast<float*>(ws.img[slot].p), dp, n_pad, h); break;
    }
    FAD_HIP_TRY(hipGetLastError());
    double* info_d = static_cast<double*>(ws.small.p) + 2 * slot;
    kad_norm_info_kernel<<<1, 256, 0, st>>>(h, n, info_d);
    FAD_HIP_TRY(hipGetLastError());
    double info[2];
    FAD_HIP_TRY(hipMemcpyAsync(info, info_d, sizeof(info), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    if (info[1] != 0.0)
        return set_error(FAD_ERR_NOT_FINITE, "KAD: %lld of %lld rows have a NaN/Inf norm", (long long)info[1], (long long)n);
    *out = Packed{static_cast<const char*>(ws.img[slot].p), h, n, dp * (int64_t)es, (int)(dp * (int64_t)es / kChunk), info[0]};
    return FAD_OK;
}

template <int MODE>
static int launch_pass(int dtype, PassArgs p, int64_t grid, hipStream_t st) {
    const size_t lds = MODE == MODE_SUM ? kLdsSum : kLdsHist;
    switch (dtype) {
        case FAD_F16: kad_pass_kernel<FAD_F16, MODE><<<(unsigned)grid, kThreads, lds, st>>>(p); break;
        case FAD_BF16: kad_pass_kernel<FAD_BF16, MODE><<<(unsigned)grid, kThreads, lds, st>>>(p); break;
        default: kad_pass_kernel<FAD_F32, MODE><<<(unsigned)grid, kThreads, lds, st>>>(p); break;
    }
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// Launch plan of one pass: (u0, cnt, grid) per launch.
struct Launch { int64_t u0, cnt, grid; };
static std::vector<Launch> plan(int64_t total, int64_t depth, bool f32, bool hist, int device) {
    std::vector<Launch> out;
    const int64_t per = kad::tiles_per_launch(depth, f32, hist);
    for (int64_t u0 = 0; u0 < total; u0 += per) {
        const int64_t cnt = std::min(per, total - u0);
        out.push_back(Launch{u0, cnt, kad::launch_grid(cnt, grid_cap(device))});
    }
    return out;
}

static int median_of_packed(const Packed& x, int dtype, int device, hipStream_t st, KadWorkspace& ws, double* sigma) {
    const int64_t T = kad::blocks(x.n), P = x.n * (x.n - 1) / 2;
    unsigned long long* hist_d = reinterpret_cast<unsigned long long*>(static_cast<double*>(ws.small.p) + 4096);
    const auto launches = plan(kad::tri_tiles(T), x.pitch / (int64_t)dtype_size(dtype), dtype == FAD_F32, true, device);
    static const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
    uint64_t rank[2] = {(uint64_t)((P - 1) / 2), (uint64_t)(P / 2)};
    unsigned int pref[2] = {0, 0};
    std::vector<unsigned long long> hist(2 * kHistBins);
    for (int pass = 0; pass < 3; ++pass) {
        FAD_HIP_TRY(hipMemsetAsync(hist_d, 0, 2 * kHistBins * sizeof(unsigned long long), st));
        PassArgs p{};
        p.a = p.b = x.img; p.ha = p.hb = x.h; p.pitch = x.pitch; p.n_a = p.n_b = x.n; p.tiles_j = T; p.tri = 1;
        p.nchunks = x.nchunks; p.hist = hist_d;
        p.pref0 = pref[0]; p.pref1 = pref[1]; p.two = pref[0] != pref[1];
        p.lo_shift = shifts[pass]; p.bits = widths[pass]; p.hi_shift = shifts[pass] + widths[pass];
        for (const Launch& l : launches) {
            p.u0 = l.u0; p.cnt = l.cnt;
            FAD_TRY(launch_pass<MODE_HIST>(dtype, p, l.grid, st));
        }
        FAD_HIP_TRY(hipMemcpyAsync(hist.data(), hist_d, hist.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
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

}  // namespace

}  // namespace fad

extern "C" {

int fad_kad_median_distance(const void* x, int64_t n, int64_t ld, int64_t d, int dtype, int on_device, double* sigma, int device,
                            void* stream) {
    using namespace fad;
    if (!sigma) return set_error(FAD_ERR_INVALID, "fad_kad_median_distance: NULL output");
    FAD_TRY(check_rows(x, n, ld, d, dtype, "fad_kad_median_distance"));
    FAD_TRY(check_device(device));
    DeviceGuard g(device);
    if (!g.ok) return set_error(FAD_ERR_HIP, "hipSetDevice(%d) failed", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    KadWorkspace& ws = workspace(device);
    Packed px;
    FAD_TRY(pack_set(0, x, n, ld, d, dtype, on_device, device, st, ws, &px));
    return median_of_packed(px, dtype, device, st, ws, sigma);
}

int fad_kad(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
            double bandwidth, fad_kad_result_t* out, int device, void* stream) {
    using namespace fad;
    if (!out) return set_error(FAD_ERR_INVALID, "fad_kad: NULL output");
    FAD_TRY(check_rows(x, n, ldx, d, dtype, "fad_kad (x)"));
    FAD_TRY(check_rows(y, m, ldy, d, dtype, "fad_kad (y)"));
    if (std::isnan(bandwidth) || std::isinf(bandwidth))
        return set_error(FAD_ERR_INVALID, "fad_kad: bandwidth %g is not finite", bandwidth);
    FAD_TRY(check_device(device));
    DeviceGuard g(device);
    if (!g.ok) return set_error(FAD_ERR_HIP, "hipSetDevice(%d) failed", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    KadWorkspace& ws = workspace(device);

    Packed px, py;
    FAD_TRY(pack_set(0, x, n, ldx, d, dtype, on_device, device, st, ws, &px));
    FAD_TRY(pack_set(1, y, m, ldy, d, dtype, on_device, device, st, ws, &py));
    double sigma = bandwidth;
    if (!(sigma > 0)) FAD_TRY(median_of_packed(px, dtype, device, st, ws, &sigma));
    if (!(sigma > 0) || !std::isfinite(sigma))
        return set_error(FAD_ERR_INVALID, "fad_kad: bandwidth %g (the median pairwise distance of the baseline when none is given) must be > 0"
                         " -- are all baseline rows identical?", sigma);
    const double cd = 1.4426950408889634 / (sigma * sigma);
    if (!(cd > 0) || !std::isfinite(cd) || !std::isfinite((float)cd) || (float)cd == 0.f)
        return set_error(FAD_ERR_INVALID, "fad_kad: bandwidth %g is outside the float32 range of the kernel", sigma);

    // passes: XX and YY over their triangles, XY over the rectangle with the larger set as the row operand
    const bool x_rows = n != m ? n > m : px.norm_sum >= py.norm_sum;
    const Packed& ra = x_rows ? px : py;
    const Packed& rb = x_rows ? py : px;
    const int64_t depth = px.pitch / (int64_t)dtype_size(dtype);
    struct PassDef { const Packed* a; const Packed* b; bool tri; int64_t total, tj; };
    const PassDef defs[3] = {{&px, &px, true, kad::tri_tiles(kad::blocks(n)), kad::blocks(n)},
                             {&py, &py, true, kad::tri_tiles(kad::blocks(m)), kad::blocks(m)},
                             {&ra, &rb, false, kad::blocks(ra.n) * kad::blocks(rb.n), kad::blocks(rb.n)}};
    std::vector<Launch> launches[3];
    int64_t off[4] = {0, 0, 0, 0};
    for (int q = 0; q < 3; ++q) {
        launches[q] = plan(defs[q].total, depth, dtype == FAD_F32, false, device);
        off[q + 1] = off[q];
        for (const Launch& l : launches[q]) off[q + 1] += l.grid;
    }
    FAD_TRY(ws.slots.reserve((size_t)off[3] * sizeof(double)));
    double* small = static_cast<double*>(ws.small.p);
    int64_t* off_d = reinterpret_cast<int64_t*>(small + 8);
    double* sums_d = small + 16;
    FAD_HIP_TRY(hipMemcpyAsync(off_d, off, sizeof(off), hipMemcpyHostToDevice, st));
    for (int q = 0; q < 3; ++q) {
        PassArgs p{};
        p.a = defs[q].a->img; p.b = defs[q].b->img; p.ha = defs[q].a->h; p.hb = defs[q].b->h; p.pitch = px.pitch;
        p.n_a = defs[q].a->n; p.n_b = defs[q].b->n; p.tiles_j = defs[q].tj; p.tri = defs[q].tri; p.nchunks = px.nchunks;
        p.c = (float)cd;
        double* slots = static_cast<double*>(ws.slots.p) + off[q];
        for (const Launch& l : launches[q]) {
            p.u0 = l.u0; p.cnt = l.cnt; p.slots = slots;
            FAD_TRY(launch_pass<MODE_SUM>(dtype, p, l.grid, st));
            slots += l.grid;
        }
    }
    kad_slots_sum_kernel<<<3, 256, 0, st>>>(static_cast<const double*>(ws.slots.p), off_d, sums_d);
    FAD_HIP_TRY(hipGetLastError());
    double sums[3];
    FAD_HIP_TRY(hipMemcpyAsync(sums, sums_d, sizeof(sums), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));

    out->kxx_mean = 2.0 * sums[0] / ((double)n * (double)(n - 1));
    out->kyy_mean = 2.0 * sums[1] / ((double)m * (double)(m - 1));
    out->kxy_mean = sums[2] / ((double)n * (double)m);
    out->mmd2 = out->kxx_mean + out->kyy_mean - 2.0 * out->kxy_mean;
    out->bandwidth = sigma;
    out->n = n;
    out->m = m;
    return FAD_OK;
}

}  // extern "C"
