// Micro-probe: issue rate / dependent latency of MFMA instructions on gfx950, and the shader clock.
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/mfma_rate scripts/probes/mfma_rate.hip && /tmp/mfma_rate
//   /tmp/mfma_rate shapes      32x32 against 16x16 MFMAs of equal FLOPs on random operands: wall time and in-kernel clock
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int KIND, int NACC>
__global__ __launch_bounds__(256) void probe(int iters, double* out, long long* cyc) {
    const long long t0 = __builtin_readcyclecounter();       // s_memtime: shader clock
    if (KIND == 0) {
        f64x4 acc[NACC];
        for (int i = 0; i < NACC; ++i) acc[i] = (f64x4){0, 0, 0, 0};
        double a = threadIdx.x * 1e-3, b = 1.0 + threadIdx.x * 1e-4;
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
        double s = 0; for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][3];
        out[blockIdx.x * 256 + threadIdx.x] = s;
    } else if (KIND == 1) {
        f32x4 acc[NACC];
        for (int i = 0; i < NACC; ++i) acc[i] = (f32x4){0, 0, 0, 0};
        float a = threadIdx.x * 1e-3f, b = 1.0f + threadIdx.x * 1e-4f;
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i], 0, 0, 0);
        float s = 0; for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][3];
        out[blockIdx.x * 256 + threadIdx.x] = s;
    } else {
        f32x16 acc[NACC];
        for (int i = 0; i < NACC; ++i) for (int q = 0; q < 16; ++q) acc[i][q] = 0;
        f16x8 a, b; for (int q = 0; q < 8; ++q) { a[q] = (_Float16)(threadIdx.x * 1e-3f); b[q] = (_Float16)1.0f; }
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[i], 0, 0, 0);
        float s = 0; for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][15];
        out[blockIdx.x * 256 + threadIdx.x] = s;
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) *cyc = __builtin_readcyclecounter() - t0;
}

template <int KIND, int NACC>
void run(const char* name, int wgs, int iters, double flop_per_mfma) {
    double* out; long long* cyc; hipMalloc(&out, (size_t)wgs * 256 * 8); hipMalloc(&cyc, 8);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    probe<KIND, NACC><<<wgs, 256>>>(iters, out, cyc);               // warm
    hipDeviceSynchronize();
    hipEventRecord(e0); probe<KIND, NACC><<<wgs, 256>>>(iters, out, cyc); hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); long long c; hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost);
    const double n_mfma_wave = (double)iters * NACC;
    const double tf = n_mfma_wave * 4 * wgs * flop_per_mfma / (ms * 1e-3) / 1e12;
    printf("%-28s wgs=%4d acc=%d: %8.3f ms  %7.1f cycles/MFMA(wave clk)  clk=%.2f GHz  %8.1f TFLOP/s\n", name, wgs, NACC, ms,
           (double)c / n_mfma_wave, (double)c / (ms * 1e6), tf);
    hipFree(out); hipFree(cyc);
}

// ------------------------------------------------------------------------------------------------------------------------------
// MFMA SHAPE against the clock the chip holds under load: bare loops on the same 64 x 64 x 32 (int8: x 64) output tile per wave and
// iteration -- 8 MFMAs of 32 x 32 or 16 of 16 x 16, equal FLOPs -- with operands in registers, filled from the hash generator of
// tile256_bench.hip (random mantissas: zeros let the chip clock higher and hide the difference), one or two waves per SIMD.  Reported:
// wall time per launch after a second of back-to-back launches, and the in-kernel clock (s_memtime against the 100 MHz s_memrealtime,
// median over the workgroups).
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t probe_hash(uint32_t i) {
    uint32_t h = i * 2654435761u; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    return h;
}
__device__ __forceinline__ f16x8 hash_f16x8(uint32_t seed) {      // ~N(0, 1) with full float16 mantissas (sum of four uniforms)
    f16x8 v;
    for (int q = 0; q < 8; ++q) {
        const uint32_t h = probe_hash(seed * 8u + q);
        const float u = ((h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + (h >> 24)) * (1.0f / 256.0f) - 1.9921875f;
        v[q] = (_Float16)(u * 1.7320508f);
    }
    return v;
}
__device__ __forceinline__ i32x4 hash_i8x16(uint32_t seed) {      // sixteen uniform int8
    i32x4 v;
    for (int q = 0; q < 4; ++q) v[q] = (int)probe_hash(seed * 4u + q);
    return v;
}

// SHAPE 0: f32_32x32x16_f16   1: f32_16x16x32_f16   2: i32_32x32x32_i8   3: i32_16x16x64_i8
template <int SHAPE>
__global__ __launch_bounds__(512) void shape_probe(int iters, float* out, long long* stamps) {
    const uint32_t me = blockIdx.x * blockDim.x + threadIdx.x;
    const long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    float sum = 0.f;
    if constexpr (SHAPE == 0) {               // rows 2 x 32, columns 2 x 32, two k-steps of 16
        f16x8 a[2][2], b[2][2];
        for (int i = 0; i < 2; ++i) for (int k = 0; k < 2; ++k) { a[i][k] = hash_f16x8(me * 16 + i * 2 + k); b[i][k] = hash_f16x8(me * 16 + 8 + i * 2 + k); }
        f32x16 acc[2][2];
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][k], b[j][k], acc[i][j], 0, 0, 0);
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) for (int q = 0; q < 16; ++q) sum += acc[i][j][q];
    } else if constexpr (SHAPE == 1) {        // rows 4 x 16, columns 4 x 16, one k-step of 32
        f16x8 a[4], b[4];
        for (int i = 0; i < 4; ++i) { a[i] = hash_f16x8(me * 16 + i); b[i] = hash_f16x8(me * 16 + 8 + i); }
        f32x4 acc[4][4];
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0, 0, 0, 0};
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) for (int q = 0; q < 4; ++q) sum += acc[i][j][q];
    } else if constexpr (SHAPE == 2) {        // rows 2 x 32, columns 2 x 32, two k-steps of 32
        i32x4 a[2][2], b[2][2];
        for (int i = 0; i < 2; ++i) for (int k = 0; k < 2; ++k) { a[i][k] = hash_i8x16(me * 16 + i * 2 + k); b[i][k] = hash_i8x16(me * 16 + 8 + i * 2 + k); }
        i32x16 acc[2][2];
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) for (int q = 0; q < 16; ++q) acc[i][j][q] = 0;
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i][k], b[j][k], acc[i][j], 0, 0, 0);
        int t = 0;
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) for (int q = 0; q < 16; ++q) t += acc[i][j][q];
        sum = (float)t;
    } else {                                  // rows 4 x 16, columns 4 x 16, one k-step of 64
        i32x4 a[4], b[4];
        for (int i = 0; i < 4; ++i) { a[i] = hash_i8x16(me * 16 + i); b[i] = hash_i8x16(me * 16 + 8 + i); }
        i32x4 acc[4][4];
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) acc[i][j] = (i32x4){0, 0, 0, 0};
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
        int t = 0;
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) for (int q = 0; q < 4; ++q) t += acc[i][j][q];
        sum = (float)t;
    }
    out[me] = sum;
    if (threadIdx.x == 0) {                   // the stamps go to a buffer of their own
        stamps[2 * blockIdx.x] = __builtin_readcyclecounter() - c0;
        stamps[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime() - r0;
    }
}

template <int SHAPE>
void run_shape(const char* name, int waves_per_simd, int iters) {
    const int wgs = 256, threads = 256 * waves_per_simd;
    float* out; long long* stamps; hipMalloc(&out, (size_t)wgs * threads * 4); hipMalloc(&stamps, (size_t)wgs * 16);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0); shape_probe<SHAPE><<<wgs, threads>>>(iters, out, stamps); hipEventRecord(e1); hipEventSynchronize(e1);
    float first; hipEventElapsedTime(&first, e0, e1);
    const int warm = (int)(1000.0f / first) + 1, reps = 20;          // a second of back-to-back launches, then the timed ones
    for (int i = 0; i < warm; ++i) shape_probe<SHAPE><<<wgs, threads>>>(iters, out, stamps);
    hipEventRecord(e0);
    for (int i = 0; i < reps; ++i) shape_probe<SHAPE><<<wgs, threads>>>(iters, out, stamps);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); ms /= reps;
    static long long h[512]; hipMemcpy(h, stamps, (size_t)wgs * 16, hipMemcpyDeviceToHost);
    double clk[256], cyc[256];
    for (int i = 0; i < wgs; ++i) { clk[i] = (double)h[2 * i] / ((double)h[2 * i + 1] * 10.0); cyc[i] = (double)h[2 * i]; }   // cycles per 10 ns tick -> GHz
    for (int i = 1; i < wgs; ++i) for (int j = i; j > 0 && clk[j] < clk[j - 1]; --j) { double t = clk[j]; clk[j] = clk[j - 1]; clk[j - 1] = t; }
    for (int i = 1; i < wgs; ++i) for (int j = i; j > 0 && cyc[j] < cyc[j - 1]; --j) { double t = cyc[j]; cyc[j] = cyc[j - 1]; cyc[j - 1] = t; }
    const double flop_iter = 2.0 * 64 * 64 * (SHAPE < 2 ? 32 : 64);                                  // per wave and iteration
    const double tf = flop_iter * iters * 4.0 * waves_per_simd * wgs / (ms * 1e-3) / 1e12;
    printf("%-22s %d wave(s)/SIMD: %8.3f ms/launch  %8.1f T(FL)OP/s  in-kernel clock %.3f GHz  %6.1f cycles per 64x64 tile step and SIMD\n", name, waves_per_simd, ms, tf,
           clk[wgs / 2], cyc[wgs / 2] / iters);
    hipFree(out); hipFree(stamps);
}

int main(int argc, char** argv) {
    if (argc > 1 && argv[1][0] == 's') {      // `mfma_rate shapes`: the shape comparison only
        const int it = 40000;
        for (int w = 1; w <= 2; ++w) {
            run_shape<0>("f32_32x32x16_f16", w, it);
            run_shape<1>("f32_16x16x32_f16", w, it);
            run_shape<0>("f32_32x32x16_f16", w, it);
            run_shape<1>("f32_16x16x32_f16", w, it);
            run_shape<2>("i32_32x32x32_i8", w, it);
            run_shape<3>("i32_16x16x64_i8", w, it);
            run_shape<2>("i32_32x32x32_i8", w, it);
            run_shape<3>("i32_16x16x64_i8", w, it);
        }
        return 0;
    }
    const int it = 20000;
    run<0, 1>("f64 16x16x4 dependent", 256, it, 2048);
    run<0, 4>("f64 16x16x4 4 chains", 256, it, 2048);
    run<0, 4>("f64 16x16x4 4 chains 2w/SIMD", 512, it, 2048);
    run<0, 4>("f64 16x16x4 4 chains 4w/SIMD", 1024, it, 2048);
    run<1, 1>("f32 16x16x4 dependent", 256, it, 2048);
    run<1, 4>("f32 16x16x4 4 chains", 256, it, 2048);
    run<2, 1>("f16 32x32x16 dependent", 256, it, 32768);
    run<2, 4>("f16 32x32x16 4 chains", 256, it, 32768);
    run<2, 4>("f16 32x32x16 4 chains 2w", 512, it, 32768);
    return 0;
}
