// The centroid update of fadtk_amd/csrc/kmeans_update.h on its own, below fad_kmeans: this file includes that header (which includes
// the key-index sort) and nothing else of the library.  kmeans::update runs on label sets the public entry cannot easily produce --
// all rows in one cluster (many chunks of one cluster), every cluster one row, empty clusters interleaved with full ones, clusters of
// chunk - 1, chunk and chunk + 1 rows -- for float32, float16 and bfloat16 rows, at depths on and off the 128-byte step.  Checked
// against host long double:
//   - every centroid of a cluster with rows within 1 float32 ulp + n_k 2^-52 max|x| of the long double mean (the float64 sum may round
//     differently from the long double one); exact on the integer-valued cases;
//   - its planes add up to the float32 centroid (times the operand scale g) exactly for float32 and bfloat16 rows and to 2^-22 for
//     float16's two planes, the padding columns are zero, h = -|g c|^2 / 2 to 1e-6 relative;
//   - an empty cluster keeps the bits of its centroid, planes and h;
//   - counts, starts and the most chunks of one cluster; a second run gives the same bits; the guard words behind cent / img / h / partial
//     come back untouched.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/kmeans_update_check tests/native/kmeans_update_check.hip
#include "../../fadtk_amd/csrc/kmeans_update.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace fad;

#define CK(x)                                                                                         \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__);              \
            exit(2);                                                                                  \
        }                                                                                             \
    } while (0)

static int failures = 0;
constexpr int64_t kGuardElems = 64;

template <typename T>
struct Dev {
    T* p = nullptr;
    int64_t n = 0;
    void alloc(int64_t count, const std::vector<T>& init) {            // count elements, then kGuardElems guard elements of 0x5a bytes
        n = count;
        CK(hipMalloc(&p, (size_t)(count + kGuardElems) * sizeof(T)));
        CK(hipMemset(p, 0x5a, (size_t)(count + kGuardElems) * sizeof(T)));
        if (!init.empty()) CK(hipMemcpy(p, init.data(), init.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    std::vector<T> get() const {
        std::vector<T> h((size_t)n);
        CK(hipMemcpy(h.data(), p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
    bool guard_ok() const {
        std::vector<unsigned char> g((size_t)kGuardElems * sizeof(T));
        CK(hipMemcpy(g.data(), p + n, g.size(), hipMemcpyDeviceToHost));
        for (unsigned char b : g)
            if (b != 0x5a) return false;
        return true;
    }
    void release() { CK(hipFree(p)); }
};

template <typename T>
static void run(const char* name, int64_t n, int64_t k, int64_t d, const std::vector<int32_t>& labels, bool integers, float g) {
    constexpr int P = kmeans::Planes<T>::value;
    const int64_t per = 128 / (int64_t)sizeof(T), dp = (d + per - 1) / per * per, k_pad = (k + 127) / 128 * 128, pitch = dp + per;
    std::mt19937 rng((uint32_t)(n * 31 + k * 7 + d));
    std::normal_distribution<float> normal(0.f, 2.f);
    std::uniform_int_distribution<int> ints(-3, 3);
    std::vector<T> rows((size_t)(n * pitch), T(0.f));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t c = 0; c < d; ++c) rows[(size_t)(i * pitch + c)] = (T)(integers ? (float)ints(rng) : normal(rng));
    std::vector<float> cent0((size_t)(k * d));
    for (auto& v : cent0) v = normal(rng);

    Dev<T> rows_d, img_d;
    Dev<float> cent_d, h_d;
    Dev<int32_t> lab_d;
    Dev<uint32_t> keys_d, sc_d, sb_d, counts_d, starts_d, chunk0_d, stats_d;
    Dev<double> partial_d;
    rows_d.alloc(n * pitch, rows);
    cent_d.alloc(k * d, cent0);
    img_d.alloc(k_pad * P * dp, {});
    h_d.alloc(k_pad, {});
    lab_d.alloc(n, labels);
    keys_d.alloc(4 * n, {});
    sc_d.alloc(kmeans::sort_counts_elems(n), {});
    sb_d.alloc(256, {});
    counts_d.alloc(k, {}); starts_d.alloc(k + 1, {}); chunk0_d.alloc(k + 1, {}); stats_d.alloc(2, {});
    partial_d.alloc(kmeans::chunks_bound(n, k) * d, {});
    kmeans::UpdateScratch w{};
    w.keys = keys_d.p; w.keys_tmp = keys_d.p + n; w.idx = keys_d.p + 2 * n; w.idx_tmp = keys_d.p + 3 * n;
    w.sort_counts = sc_d.p; w.sort_bases = sb_d.p; w.counts = counts_d.p; w.starts = starts_d.p; w.chunk0 = chunk0_d.p; w.stats = stats_d.p;
    w.partial = partial_d.p;

    // the operand of the given centroids first (what fad_kmeans does with init), then the update
    kmeans::centroid_finish_kernel<T><<<(unsigned)((k_pad + 3) / 4), 256>>>(nullptr, nullptr, nullptr, k, k_pad, d, dp, cent_d.p, img_d.p, h_d.p,
                                                                          g, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    const std::vector<T> img0 = img_d.get();
    const std::vector<float> h0 = h_d.get();
    std::vector<float> cent_run[2];
    std::vector<T> img_run[2];
    std::vector<float> h_run[2];
    for (int r = 0; r < 2; ++r) {
        if (r) {                                                       // a second run from the same state
            CK(hipMemcpy(cent_d.p, cent0.data(), cent0.size() * sizeof(float), hipMemcpyHostToDevice));
            CK(hipMemcpy(img_d.p, img0.data(), img0.size() * sizeof(T), hipMemcpyHostToDevice));
            CK(hipMemcpy(h_d.p, h0.data(), h0.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        CK(kmeans::update<T>(lab_d.p, n, k, k_pad, d, dp, rows_d.p, pitch, w, cent_d.p, img_d.p, h_d.p, g, nullptr));
        CK(hipDeviceSynchronize());
        cent_run[r] = cent_d.get(); img_run[r] = img_d.get(); h_run[r] = h_d.get();
    }
    const std::vector<float>& cent = cent_run[0];
    const std::vector<T>& img = img_run[0];
    const std::vector<float>& h = h_run[0];
    const std::vector<uint32_t> counts = counts_d.get(), starts = starts_d.get(), stats = stats_d.get();

    int bad = 0;
    bad += memcmp(cent_run[0].data(), cent_run[1].data(), cent.size() * sizeof(float)) != 0;
    bad += memcmp(img_run[0].data(), img_run[1].data(), img.size() * sizeof(T)) != 0;
    bad += memcmp(h_run[0].data(), h_run[1].data(), h.size() * sizeof(float)) != 0;
    std::vector<int64_t> want_count((size_t)k, 0);
    for (int32_t l : labels) want_count[(size_t)l] += 1;
    double xmax = 0.0;
    for (const T& v : rows) xmax = std::max(xmax, std::fabs((double)(float)v));
    int64_t run_start = 0, most = 0, empty = 0;
    for (int64_t c = 0; c < k; ++c) {
        bad += counts[(size_t)c] != (uint32_t)want_count[(size_t)c] || starts[(size_t)c] != (uint32_t)run_start;
        run_start += want_count[(size_t)c];
        most = std::max<int64_t>(most, (want_count[(size_t)c] + kmeans::kChunkRows - 1) / kmeans::kChunkRows);
        empty += want_count[(size_t)c] == 0;
    }
    bad += starts[(size_t)k] != (uint32_t)n || stats[0] != (uint32_t)most || stats[1] != (uint32_t)empty;
    std::vector<long double> sum((size_t)(k * d), 0.0L);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t c = 0; c < d; ++c) sum[(size_t)(labels[(size_t)i] * d + c)] += (long double)(float)rows[(size_t)(i * pitch + c)];
    for (int64_t c = 0; c < k; ++c) {
        const T* planes = img.data() + c * P * dp;
        if (want_count[(size_t)c] == 0) {                                // untouched: the bits of before
            bad += memcmp(&cent[(size_t)(c * d)], &cent0[(size_t)(c * d)], (size_t)d * sizeof(float)) != 0;
            bad += memcmp(planes, img0.data() + c * P * dp, (size_t)(P * dp) * sizeof(T)) != 0;
            bad += memcmp(&h[(size_t)c], &h0[(size_t)c], sizeof(float)) != 0;
            continue;
        }
        double norm = 0.0;
        for (int64_t col = 0; col < dp; ++col) {
            double carried = 0.0;
            for (int p = 0; p < P; ++p) carried += (double)(float)planes[p * dp + col];
            if (col >= d) { bad += carried != 0.0; continue; }
            const float got = cent[(size_t)(c * d + col)];
            const long double mean = sum[(size_t)(c * d + col)] / (long double)want_count[(size_t)c];
            const float want = (float)mean;
            const double ulp = (double)std::nextafter(std::fabs(want), INFINITY) - (double)std::fabs(want);
            // integer rows: every sum is exact, so the float32 of the quotient is the long double one's; else the tolerance above
            const double tol = ulp + (double)want_count[(size_t)c] * 0x1p-52 * xmax;
            if (integers) bad += got != want;
            else bad += !(std::fabs((double)got - (double)mean) <= tol);
            // the planes carry g c: exactly (float32, and bfloat16's three planes), to 2^-22 for float16's two (11 + 11 bits and a sign)
            const double cg = (double)got * (double)g;
            bad += !(std::fabs(carried - cg) <= (P == 2 ? std::fabs(cg) * 0x1p-21 + 0x1p-24 : 0.0));
            norm += (double)got * (double)g * (double)got * (double)g;
        }
        bad += !(std::fabs((double)h[(size_t)c] + 0.5 * norm) <= 1e-6 * (0.5 * norm) + 1e-30);
    }
    for (int64_t c = k; c < k_pad; ++c) bad += !(std::isinf(h[(size_t)c]) && h[(size_t)c] < 0);
    bad += !cent_d.guard_ok() || !img_d.guard_ok() || !h_d.guard_ok() || !partial_d.guard_ok() || !keys_d.guard_ok() || !counts_d.guard_ok()
           || !starts_d.guard_ok() || !chunk0_d.guard_ok() || !stats_d.guard_ok();
    printf("%-40s %-5s n=%lld k=%lld d=%lld most chunks %lld empty %lld: %s\n", name, sizeof(T) == 4 ? "fp32" : P == 2 ? "fp16" : "bf16",
           (long long)n, (long long)k, (long long)d, (long long)most, (long long)empty, bad ? "FAILED" : "ok");
    failures += bad != 0;
    rows_d.release(); img_d.release(); cent_d.release(); h_d.release(); lab_d.release(); keys_d.release(); sc_d.release(); sb_d.release();
    counts_d.release(); starts_d.release(); chunk0_d.release(); stats_d.release(); partial_d.release();
}

template <typename T>
static void all_cases(float g) {
    for (int integers = 0; integers < 2; ++integers) {
        const bool ii = integers != 0;
        {   // all rows in one cluster of several: many chunks, the others keep their bits
            const int64_t n = 5000, k = 9;
            run<T>("all rows in one cluster", n, k, 70, std::vector<int32_t>((size_t)n, 4), ii, g);
        }
        {   // every cluster one row, in a scrambled order
            const int64_t n = 300, k = 300;
            std::vector<int32_t> l((size_t)n);
            for (int64_t i = 0; i < n; ++i) l[(size_t)i] = (int32_t)((i * 7) % n);
            run<T>("every cluster one row", n, k, 17, l, ii, g);
        }
        {   // empty clusters interleaved: only the even labels are used
            const int64_t n = 2049, k = 130;
            std::vector<int32_t> l((size_t)n);
            for (int64_t i = 0; i < n; ++i) l[(size_t)i] = (int32_t)(2 * ((i * 13) % (k / 2)));
            run<T>("empty clusters interleaved", n, k, 128, l, ii, g);
        }
        {   // clusters of chunk - 1, chunk, chunk + 1 rows, and one row at D = 1
            const int64_t c = kmeans::kChunkRows, n = 3 * c + 1, k = 4;
            std::vector<int32_t> l;
            for (int64_t i = 0; i < c - 1; ++i) l.push_back(2);
            for (int64_t i = 0; i < c; ++i) l.push_back(0);
            for (int64_t i = 0; i < c + 1; ++i) l.push_back(3);
            l.push_back(1);
            run<T>("chunk - 1, chunk, chunk + 1, one row", n, k, 1, l, ii, g);
        }
    }
}

int main() {
    all_cases<float>(1.f);
    all_cases<_Float16>(1.f);
    all_cases<_Float16>(256.f);                                        // the scaled operand of float16 rows
    all_cases<__bf16>(1.f);
    if (failures) {
        printf("%d cases FAILED\n", failures);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
