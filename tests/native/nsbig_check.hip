// Kernel-by-kernel check of the BATCHED square-root chain (fadtk_amd/csrc/ns_fast_big.h) on the GPU against plain host float64
// arithmetic (test infrastructure, gfx950) -- the batch's counterpart of nsfast_check.hip, with the same report lines and tolerances.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/nsbig_check tests/native/nsbig_check.hip
//   tests/native/nsbig_check big_iter [d:nprob ...]      nsf_big<SP_FIRST | SP_T | SP_U, NJ = 1 | 2>
//   tests/native/nsbig_check big_i8   [d:nprob ...]      nsf_i8_big<I8_A>, <I8_G>, <I8_G, true>
//   tests/native/nsbig_check res128   [nprob ...]        nsf_res128<false>, <true> (D = 128), against the tiled route of ns_fast.h
// Every launch works on ONE device block whose image the host builds first: a shared part (the baseline's header and digit planes),
// then the problems `pstride` apart, then the records the host reads `hstride` apart.  Every field of a problem is followed by a guard
// of 256 bytes and the whole image starts out as 0xEE, so after a launch EVERY byte outside the fields the kernel is meant to write
// for the problems that are meant to run must be what it was: guards, operands, and everything of a problem that carries a skip word,
// a refused header (bad set / flag_gen == gen) or -- SP_FIRST -- a spectrum the chain declines.  Each problem has operands of its own
// seed with a gain of its own on one side, its own header scales and its own step scale mu[k]: a result that lands in the wrong
// problem or tile, or is formed with another problem's scalars, cannot match.  The references are float64 products of the values the
// uploaded planes hold.
//
// The wait switch of nsf_big: with FAD_BIG_STAGES = 3 a stage waits with at most ONE younger stage in flight, so `ahead * PP` is 3
// (NJ = 1) or 4 (NJ = 2) in the body of the k loop and 0 on its last step; the arms 6, 8, 9, 12, 15, 16, 18, 20 and 24 belong to ring
// depths of four and more and are unreachable here.  The shapes below walk 16, 24, 32, 48 and 64 k-steps through both reachable arms.
//
// Not covered: performance, FAD_BIG_STAGES != 3 and the ablation #ifdefs.  nsf_res128<true> keeps its iterate on the chip: its host record
// cannot be recomputed from planes it wrote and is checked through the trace estimate it stands for (see check_res128).
// Exit code 0 = all checks passed.
// (the LDS-DMA loads of ns_fast_big.h name m0 as a clobber, which clang remarks on for every instantiation: silenced for that header only)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#include "../../fadtk_amd/csrc/ns_fast_big.h"
#pragma clang diagnostic pop
#include "../../fadtk_amd/csrc/ns_fast_res.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

using namespace fad;
using namespace fad::nsf;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

static int g_fail = 0;
static void report(const char* what, double err, double tol) {
    const bool ok = (err <= tol) && (err == err);
    printf("  %-66s err %.3e  (tol %.1e)  %s\n", what, err, tol, ok ? "ok" : "FAIL");
    if (!ok) ++g_fail;
}
static const double kDigTol = std::ldexp(1.0, -41) * 1.01;

template <class F> static void parallel_for(int n, F f) {                  // (the references of the problems are independent)
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    for (int t = 0; t < std::min(n, 8); ++t) th.emplace_back([&] { for (;;) { const int i = next++; if (i >= n) break; f(i); } });
    for (auto& t : th) t.join();
}

// ---- helpers of nsfast_check.hip, here on a host image of the device block
static float h2f(uint16_t b) { _Float16 h; memcpy(&h, &b, 2); return (float)h; }
static void host_split(float v, uint16_t& hi, uint16_t& lo) {
    _Float16 h = (_Float16)v; _Float16 l = (_Float16)((v - (float)h) * 2048.f);
    memcpy(&hi, &h, 2); memcpy(&lo, &l, 2);
}
static float host_used(uint16_t hi, uint16_t lo) { return h2f(hi) + h2f(lo) * (1.f / 2048.f); }
static float host_round_split(float v) { uint16_t a, b; host_split(v, a, b); return host_used(a, b); }
static double dig_value(const int8_t* dg, int row, int k, int d) {
    static const double w[kDigits] = {std::ldexp(1.0, -40), std::ldexp(1.0, -33), std::ldexp(1.0, -26), std::ldexp(1.0, -19), std::ldexp(1.0, -12), std::ldexp(1.0, -5)};
    double v = 0.0;
    for (int p = 0; p < kDigits; ++p) { int byte; const size_t piece = dg_elem(row, k, p, d, byte); v += (double)dg[piece * 16 + byte] * w[p]; }
    return v;
}
static float fa_value(const uint16_t* w, int row, int k, int d) {
    int half; const size_t p0 = fa_elem(row, k, 0, d, half), p1 = fa_elem(row, k, 1, d, half);
    return host_used(w[p0 * 8 + half], w[p1 * 8 + half]);
}
// a SplitMat field: planes of X (4 d^2 bytes), then planes of X^T
struct HostSplit { std::vector<float> x, xt; };
static HostSplit fetch_split(const uint8_t* f, int d) {
    const size_t dd = (size_t)d * d;
    const uint16_t* a = reinterpret_cast<const uint16_t*>(f); const uint16_t* at = reinterpret_cast<const uint16_t*>(f + 4 * dd);
    HostSplit s; s.x.resize(dd); s.xt.resize(dd);
    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) { s.x[(size_t)r * d + c] = fa_value(a, r, c, d); s.xt[(size_t)r * d + c] = fa_value(at, c, r, d); }
    return s;
}
static void upload_split(uint8_t* f, const std::vector<float>& x, int d) {
    const size_t dd = (size_t)d * d;
    uint16_t* a = reinterpret_cast<uint16_t*>(f); uint16_t* at = reinterpret_cast<uint16_t*>(f + 4 * dd);
    for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c) {
            uint16_t hi, lo; host_split(x[(size_t)r * d + c], hi, lo);
            int half;
            a[fa_elem(r, c, 0, d, half) * 8 + half] = hi; a[fa_elem(r, c, 1, d, half) * 8 + half] = lo;
            at[fa_elem(c, r, 0, d, half) * 8 + half] = hi; at[fa_elem(c, r, 1, d, half) * 8 + half] = lo;
        }
}
static SplitMat dev_split(uint8_t* f, int d) { return SplitMat{reinterpret_cast<uint4*>(f), reinterpret_cast<uint4*>(f + 4 * (size_t)d * d)}; }
// digit planes (6 d^2 bytes) of W, or of W^T: digits_of<double> of ns_fast.h on the host
static void upload_digits(uint8_t* f, const std::vector<double>& w, int d, bool transposed) {
    int8_t* dg = reinterpret_cast<int8_t*>(f);
    for (int row = 0; row < d; ++row)
        for (int k = 0; k < d; ++k) {
            double t = (transposed ? w[(size_t)k * d + row] : w[(size_t)row * d + k]) * 32.0;
            for (int p = kDigits - 1; p >= 0; --p) {
                const double r = std::nearbyint(t);
                int byte; const size_t piece = dg_elem(row, k, p, d, byte);
                dg[piece * 16 + byte] = (int8_t)(int)r;
                t = (t - r) * 128.0;
            }
        }
}
static double max_abs_diff(const std::vector<float>& x, const std::vector<float>& y) {
    double m = 0.0; for (size_t i = 0; i < x.size(); ++i) m = std::fmax(m, std::fabs((double)x[i] - (double)y[i])); return m;
}
// A times (bT)^T, accumulated in ACC.  float operands (22 significant bits): products are exact in double.  Values on the 2^-40 grid
// (41 bits) are not: a double product rounds at 1e-16 of itself and d of them add up to the size of the bound on the exact product
// (4e-15 d / 512), so that reference is accumulated in long double
template <class ACC, class TA, class TB> static std::vector<double> host_mm_t(const std::vector<TA>& a, const std::vector<TB>& bT, int d) {
    std::vector<double> c((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            ACC s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            const TA* ai = &a[(size_t)i * d]; const TB* bj = &bT[(size_t)j * d];
            for (int k = 0; k < d; k += 4) { s0 += (ACC)ai[k] * (ACC)bj[k]; s1 += (ACC)ai[k + 1] * (ACC)bj[k + 1]; s2 += (ACC)ai[k + 2] * (ACC)bj[k + 2]; s3 += (ACC)ai[k + 3] * (ACC)bj[k + 3]; }
            c[(size_t)i * d + j] = (double)((s0 + s1) + (s2 + s3));
        }
    return c;
}
static std::vector<double> host_mm(const std::vector<float>& a, const std::vector<float>& b, int d) {      // C = A B in float64 on float operands
    std::vector<float> bt((size_t)d * d);
    for (int k = 0; k < d; ++k) for (int j = 0; j < d; ++j) bt[(size_t)j * d + k] = b[(size_t)k * d + j];
    return host_mm_t<double>(a, bt, d);
}
// per-tile statistics of nsf_i8<A> for a (normalised) matrix, and the bounds the first iteration derives from them
static void tile_stats(const std::vector<double>& An, int d, std::vector<double>& rec) {
    const int nb = d / 32;
    rec.assign((size_t)kTileStats * nb * nb, 0.0);
    for (int ty = 0; ty < nb; ++ty) for (int tx = 0; tx < nb; ++tx) {
        double sq = 0.0, tr = 0.0, mr = 0.0, mc = 0.0, cs[32] = {0};
        for (int r = 0; r < 32; ++r) {
            double rs = 0.0;
            for (int c = 0; c < 32; ++c) { const double w = An[(size_t)(ty * 32 + r) * d + tx * 32 + c]; const double v = (double)(float)w; sq += w * w; rs += std::fabs(v); cs[c] += std::fabs(v); if (ty * 32 + r == tx * 32 + c) tr += w; }
            mr = std::fmax(mr, rs);
        }
        for (int c = 0; c < 32; ++c) mc = std::fmax(mc, cs[c]);
        double* q = &rec[(size_t)kTileStats * (ty * nb + tx)];
        q[0] = sq; q[1] = tr; q[2] = mr; q[3] = mc;
    }
}
struct Bounds { double fro2, tr, u, c; };
static Bounds scale_from_stats(const std::vector<double>& rec, int d) {
    const int nb = d / 32;
    Bounds b{0.0, 0.0, 0.0, 0.0};
    double inf_b = 0.0, one_b = 0.0;
    for (int t = 0; t < nb * nb; ++t) { b.fro2 += rec[(size_t)kTileStats * t]; b.tr += rec[(size_t)kTileStats * t + 1]; }
    for (int x = 0; x < nb; ++x) {
        double p = 0.0, q = 0.0;
        for (int y = 0; y < nb; ++y) { p += rec[(size_t)kTileStats * (x * nb + y) + 2]; q += rec[(size_t)kTileStats * (y * nb + x) + 3]; }
        inf_b = std::fmax(inf_b, p); one_b = std::fmax(one_b, q);
    }
    b.u = std::sqrt(b.fro2); if (inf_b < b.u) b.u = inf_b; if (one_b < b.u) b.u = one_b;
    b.c = b.u / 2.9; const double wm = b.fro2 / b.tr; if (wm > b.c && wm <= b.u) b.c = wm;
    return b;
}
// ns_check.h's x_min estimate and step scale on the host (float transcendentals of libm instead of the device's: the bisection may take
// its last steps differently, 8 / 2^20 in the exponent = 2e-5 relative in l, 1e-6 in mu -- the comparison below allows 1e-5)
static double host_l0_from_participation(float pr, int d) {
    const float lg = log2f((float)d);
    auto S = [&](float p) {
        if (fabsf(p - 1.0f) < 1e-4f) return 0.5f * (1.0f + exp2f(-lg)) + lg * 0.69314718f;
        return 0.5f * (1.0f + exp2f(-p * lg)) + (exp2f((1.0f - p) * lg) - 1.0f) / (1.0f - p);
    };
    float lo = 0.0f, hi = 8.0f, pf = 4.0f;
    for (int it = 0; it < 20; ++it) { pf = 0.5f * (lo + hi); const float s1 = S(pf), val = s1 * s1 / S(2.0f * pf); if (val > pr) lo = pf; else hi = pf; }
    double l = (double)(exp2f(-0.5f * pf * lg) * (1.0f / 3.0f));
    if (l > 0.5) l = 0.5;
    if (l < 1e-5) l = 1e-5;
    return l;
}
static double host_step_scale(double& l) {
    if (!(l < 0.9)) { l = l * (3.0 - l * l) / 2.0; return 1.0; }
    const double m = std::sqrt(3.0 / (1.0 + l + l * l));
    l = m * l * (3.0 - m * m * l * l) / 2.0;
    return m;
}

// ---- the device block and its host image
struct Region { size_t off, bytes; };
struct Image {
    std::vector<uint8_t> before, after; uint8_t* dev = nullptr;
    void alloc(size_t n) { before.assign(n, 0xEE); after.assign(n, 0); CK(hipMalloc(&dev, n + 256)); }
    void release() { CK(hipFree(dev)); dev = nullptr; std::vector<uint8_t>().swap(before); std::vector<uint8_t>().swap(after); }
    void upload() { CK(hipMemcpy(dev, before.data(), before.size(), hipMemcpyHostToDevice)); }
    void fetch() { CK(hipMemcpy(after.data(), dev, after.size(), hipMemcpyDeviceToHost)); }
    template <class T> T* b(size_t off) { return reinterpret_cast<T*>(before.data() + off); }
    template <class T> const T* a(size_t off) const { return reinterpret_cast<const T*>(after.data() + off); }
    template <class T> T* d(size_t off) { return reinterpret_cast<T*>(dev + off); }
    // bytes that differ from the image outside the regions the launch may write
    double touched_outside(const std::vector<Region>& allowed) const {
        std::vector<uint8_t> t = after;
        for (const Region& r : allowed) memcpy(t.data() + r.off, before.data() + r.off, r.bytes);
        if (memcmp(t.data(), before.data(), t.size()) == 0) return 0.0;
        size_t n = 0, first = 0;
        for (size_t i = 0; i < t.size(); ++i) if (t[i] != before[i]) { if (!n) first = i; ++n; }
        printf("      (%zu bytes changed outside the launch's outputs, the first at offset %zu)\n", n, first);
        return (double)n;
    }
};
struct Layout {
    size_t o = 0;
    size_t take(size_t bytes) { const size_t at = o; o += ((bytes + 255) & ~(size_t)255) + 256; return at; }      // the field, then its guard
};

// ---- who runs: problem 1 carries a skip word in the launches with a shared baseline (SP_FIRST knows no skip word: there problem 1 is a
// spectrum the chain declines, in both kinds of launch), problem 2 a refused header in the launches of pairs; batches of more than
// five problems carry both in each launch (problem 5: the other kind)
// Which refusal a shape takes (set_headers): shared baseline -> flag_gen == gen on the B header of problem 5 (256:7, 8, 9, 20, 384:9, 768:9);
// pairs and an odd nprob -> flag_gen == gen on the A header of problem 2 (256:7, 9, 384:3, 9, 768:3, 9, 512:3, 1024:3); pairs and an even
// nprob -> `bad` on the B header of problem 2 (256:8, 256:20 only).  256:1 has no skipped, refused or declined problem.  A change to the
// shape list must keep one shape of each kind.
static bool is_bad(int k, int nprob, int pairs) { return nprob >= 3 && (pairs ? k == 2 : (k == 5 && nprob > 5)); }
static bool is_skip(int k, int nprob, int pairs) { return nprob >= 3 && (pairs ? (k == 5 && nprob > 5) : k == 1); }
static bool is_declined(int k, int nprob) { return nprob >= 3 && k == 1; }
static double scale_A(int k, int pairs) { return pairs ? std::ldexp(1.0, k & 1) : 0.5; }
static double scale_B(int k) { return std::ldexp(1.0, -(k % 3)); }
static double inv_s12(int k, int pairs) { return 1.0 / (scale_A(k, pairs) * scale_B(k)); }
static void set_headers(Image& im, size_t hA_shared, size_t hA0, size_t hB0, size_t stride, int nprob, int pairs, int gen) {
    MatHdr h; memset(&h, 0, sizeof(h));
    h.s = scale_A(0, 0); h.tr = 7.0; h.flag_gen = gen - 1;                  // (a stale token is no flag)
    *im.b<MatHdr>(hA_shared) = h;
    for (int k = 0; k < nprob; ++k) {
        MatHdr a, b; memset(&a, 0, sizeof(a)); memset(&b, 0, sizeof(b));
        a.s = scale_A(k, 1); a.tr = 7.0 + k; a.flag_gen = gen - 1;
        b.s = scale_B(k); b.tr = 100.0 + k; b.flag_gen = gen - 1;
        if (is_bad(k, nprob, pairs)) { if (pairs && (nprob & 1)) a.flag_gen = gen; else if (pairs) b.bad = 1; else b.flag_gen = gen; }
        *im.b<MatHdr>(hA0 + k * stride) = a; *im.b<MatHdr>(hB0 + k * stride) = b;
    }
}
static double tr_A(int k, int pairs) { return pairs ? 7.0 + k : 7.0; }
static bool same_s32(const Ns32State& a, const Ns32State& b) {
    bool s = a.done == b.done && a.finished == b.finished && a.ok == b.ok && a.final_iter == b.final_iter && a.failed == b.failed && a.upd_skip[0] == b.upd_skip[0] &&
             a.upd_skip[1] == b.upd_skip[1] && a.skip_corr == b.skip_corr && a.decided_at == b.decided_at && a.strict == b.strict && a.grew == b.grew;
    for (int i = 0; i < 16; ++i) s = s && a.res[i] == b.res[i];
    return s;
}

// =================================================================================================================================
// big_iter: nsf_big<SP_FIRST | SP_T | SP_U, NJ>
template <int NJ> static void launch_big(int mode, int d, int nprob, SplitArgs g) {
    static bool ready = false;
    if (!ready) {
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_big<SP_FIRST, NJ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBigLds));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_big<SP_T, NJ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBigLds));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_big<SP_U, NJ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBigLds));
        ready = true;
    }
    g.nprob = nprob;
    const int tt = big_tiles(d, NJ);
    if (mode == SP_FIRST) hipLaunchKernelGGL((nsf_big<SP_FIRST, NJ>), dim3((unsigned)big_grid(nprob, tt)), dim3(256), kBigLds, 0, g);
    else if (mode == SP_T) hipLaunchKernelGGL((nsf_big<SP_T, NJ>), dim3((unsigned)big_grid(nprob, tt)), dim3(256), kBigLds, 0, g);
    else hipLaunchKernelGGL((nsf_big<SP_U, NJ>), dim3((unsigned)(big_grid(nprob, 2 * tt) + nprob)), dim3(256), kBigLds, 0, g);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
}
static void run_big(int nj, int mode, int d, int nprob, const SplitArgs& g) { if (nj == 1) launch_big<1>(mode, d, nprob, g); else launch_big<2>(mode, d, nprob, g); }

struct IterProb {
    std::vector<float> Pw, Pq, Y, Z, T;                 // the two stand-ins of the product (flat / decaying), the iterates
    std::vector<double> Pd, Pdq, statsW, statsQ;
    std::vector<double> PP, PPq, ZY, YT, TZ;            // float64 references on the values the planes hold
    Bounds bw, bq;
    double l0q, mu0q, mu1q, lq;                          // scaled run: the host's x_min estimate and step scales
};

static void check_big_iter(int d, int nprob) {
    printf("== big_iter  d = %d, %d problems\n", d, nprob);
    const size_t dd = (size_t)d * d;
    const int nb = d / 32, t = d / 128, gen = 500 + d + nprob;
    const double l0_scale = 0.5, l0_min = 1e-4;
    char buf[200];
    std::vector<IterProb> pr(nprob);
    parallel_for(nprob, [&](int k) {
        IterProb& p = pr[k];
        std::mt19937_64 rng(77000 + 131 * d + k);
        std::normal_distribution<double> nd(0.0, 1.0);
        const double gain = 0.6 + 0.045 * k;                                  // the scale must absorb it
        const double decay = is_declined(k, nprob) ? 4.0 : 1.0 + 0.05 * k;      // a spectrum of its own: a step scale of its own
        p.Pw.resize(dd); p.Pq.resize(dd); p.Pd.resize(dd); p.Pdq.resize(dd); p.Y.resize(dd); p.Z.resize(dd); p.T.resize(dd);
        for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) {
            const size_t i = (size_t)r * d + c;
            const double q = (r == c ? std::pow(1.0 + r, -decay) : 0.0) + 1e-5 * nd(rng);
            // (the declined problem has no flat stand-in: without scaled steps the participation-ratio rule must turn it away)
            const double v = is_declined(k, nprob) ? q : gain * ((r == c ? 0.8 + 0.4 * ((r * 37) % 11) / 11.0 : 0.0) + 0.004 * nd(rng));
            p.Pd[i] = v; p.Pw[i] = (float)v; p.Pdq[i] = q; p.Pq[i] = (float)q;
            p.Y[i] = host_round_split((float)((1.0 + 0.015 * k) * ((r == c ? 0.8 + 0.4 * ((r * 29) % 13) / 13.0 : 0.0) + 0.01 * nd(rng))));
            p.Z[i] = host_round_split((float)((r == c ? 1.2 - 0.4 * ((r * 31) % 7) / 7.0 : 0.0) + 0.01 * nd(rng)));
            p.T[i] = host_round_split((float)((r == c ? 1.0 + 0.1 * ((r * 17) % 5) / 5.0 : 0.0) + 0.01 * nd(rng)));
        }
        tile_stats(p.Pd, d, p.statsW); tile_stats(p.Pdq, d, p.statsQ);
        p.bw = scale_from_stats(p.statsW, d); p.bq = scale_from_stats(p.statsQ, d);
        p.l0q = host_l0_from_participation((float)(p.bq.tr * p.bq.tr / p.bq.fro2), d) * l0_scale; if (p.l0q > 0.5) p.l0q = 0.5;
        double l = p.l0q; p.mu0q = host_step_scale(l); p.lq = l; double ln = l; p.mu1q = host_step_scale(ln);
    });
    parallel_for(5 * nprob, [&](int job) {
        IterProb& p = pr[job / 5];
        std::vector<float> u(dd);
        switch (job % 5) {
            case 0: for (size_t i = 0; i < dd; ++i) u[i] = host_round_split(p.Pw[i]); p.PP = host_mm(u, u, d); break;
            case 1: for (size_t i = 0; i < dd; ++i) u[i] = host_round_split(p.Pq[i]); p.PPq = host_mm(u, u, d); break;
            case 2: p.ZY = host_mm(p.Z, p.Y, d); break;
            case 3: p.YT = host_mm(p.Y, p.T, d); break;
            default: p.TZ = host_mm(p.T, p.Z, d); break;
        }
    });

    Layout L;
    const size_t hA = L.take(sizeof(MatHdr)), hB = L.take(sizeof(MatHdr)), st = L.take(sizeof(NsState)), s32 = L.take(sizeof(Ns32State));
    const size_t part_bytes = (size_t)2 * t * t * sizeof(double);
    const size_t partials = L.take(part_bytes), stats = L.take((size_t)kTileStats * nb * nb * sizeof(double));
    const size_t A64 = L.take(8 * dd), P = L.take(8 * dd), Y = L.take(8 * dd), Z = L.take(8 * dd), T = L.take(8 * dd), O1 = L.take(8 * dd), O2 = L.take(8 * dd);
    const size_t dig = L.take(6 * dd), digt = L.take(6 * dd);
    const size_t stride = L.o + 4096, shared = 512, base = shared;            // (pstride > payload: a guard region between the problems)
    Image im; im.alloc(shared + (size_t)nprob * stride);
    auto F = [&](size_t f, int k) { return base + f + (size_t)k * stride; };
    // operands every launch of this shape shares
    for (int k = 0; k < nprob; ++k) { upload_split(im.b<uint8_t>(F(Y, k)), pr[k].Y, d); upload_split(im.b<uint8_t>(F(Z, k)), pr[k].Z, d); upload_split(im.b<uint8_t>(F(T, k)), pr[k].T, d); }

    for (int pairs = 0; pairs < 2; ++pairs)
        for (int nj = 1; nj <= 2; ++nj) {
            const int tiles = big_tiles(d, nj), tx_n = (nj == 2) ? t : 2 * t, tw = 64 * nj;
            char tag[64]; snprintf(tag, sizeof(tag), "NJ %d %s", nj, pairs ? "pairs " : "shared");
            set_headers(im, 0, F(hA, 0), F(hB, 0), stride, nprob, pairs, gen);
            auto args = [&]() {
                SplitArgs g; memset(&g, 0, sizeof(g));
                g.d = d; g.gen = gen; g.hA = pairs ? im.d<MatHdr>(F(hA, 0)) : im.d<MatHdr>(0); g.hB = im.d<MatHdr>(F(hB, 0));
                g.pstride = (int64_t)stride; g.astride = pairs ? (int64_t)stride : 0;
                g.st = im.d<NsState>(F(st, 0)); g.s32 = im.d<Ns32State>(F(s32, 0));
                return g;
            };
            auto mat = [&](size_t f) { return dev_split(im.d<uint8_t>(F(f, 0)), d); };
            auto reset_outputs = [&]() {
                for (int k = 0; k < nprob; ++k) {
                    for (size_t f : {O1, O2}) memset(im.b<uint8_t>(F(f, k)), 0xEE, 8 * dd);
                    memset(im.b<uint8_t>(F(dig, k)), 0xEE, 6 * dd); memset(im.b<uint8_t>(F(digt, k)), 0xEE, 6 * dd);
                    memset(im.b<uint8_t>(F(partials, k)), 0xEE, part_bytes);
                    memset(im.b<uint8_t>(F(st, k)), 0, sizeof(NsState)); memset(im.b<uint8_t>(F(s32, k)), 0x55, sizeof(Ns32State));
                }
            };

            // ---------------- SP_FIRST, plain and with scaled steps
            for (int scaled = 0; scaled < 2; ++scaled) {
                reset_outputs();
                for (int k = 0; k < nprob; ++k) {
                    const IterProb& p = pr[k];
                    const std::vector<float>& Pm = scaled ? p.Pq : p.Pw; const std::vector<double>& Pdm = scaled ? p.Pdq : p.Pd;
                    upload_split(im.b<uint8_t>(F(P, k)), Pm, d);
                    double* a64 = im.b<double>(F(A64, k));
                    for (size_t i = 0; i < dd; ++i) a64[i] = Pdm[i] * inv_s12(k, pairs);
                    memcpy(im.b<double>(F(stats, k)), (scaled ? p.statsQ : p.statsW).data(), (size_t)kTileStats * nb * nb * sizeof(double));
                    im.b<NsState>(F(st, k))->mean_term = 0.25 + k;
                }
                im.upload();
                SplitArgs g = args();
                g.A[0] = mat(P); g.B[0] = mat(P); g.C[0] = mat(O1); g.C[1] = mat(O2); g.A64 = im.d<double>(F(A64, 0)); g.statsA = im.d<double>(F(stats, 0));
                if (scaled) { g.scaled = 1; g.lp_wide = 1; g.l0_scale = l0_scale; g.l0_min = l0_min; }
                run_big(nj, SP_FIRST, d, nprob, g);
                im.fetch();
                std::vector<Region> allowed;
                double e_c = 0.0, e_w = 0.0, e_y = 0.0, e_z = 0.0, e_o = 0.0, e_mu = 0.0, e_dec = 0.0;
                for (int k = 0; k < nprob; ++k) {
                    if (is_bad(k, nprob, pairs)) continue;
                    allowed.push_back({F(st, k), sizeof(NsState)}); allowed.push_back({F(s32, k), sizeof(Ns32State)});
                    const IterProb& p = pr[k];
                    const NsState s = *im.a<NsState>(F(st, k)); const Ns32State q = *im.a<Ns32State>(F(s32, k));
                    const bool words = s.tr1 == tr_A(k, pairs) && s.tr2 == 100.0 + k && s.mean_term == 0.25 + k && s.res_min == 1e300 && s.final_iter == -1 && s.conv == 0 &&
                                       s.nonfinite == 0 && s.done == 0 && s.finished == 0 && q.ok == 0 && q.final_iter == -1 && q.skip_corr == 1 && q.decided_at == -1 &&
                                       q.strict == 0 && q.grew == 0 && q.res[0] == 1e300;
                    if (is_declined(k, nprob)) {
                        const bool dec = words && q.failed == 1 && q.done == 1 && q.finished == 1 && q.upd_skip[0] == 1 && q.upd_skip[1] == 1 &&
                                         (!scaled || (s.mu[0] == 1.0 && s.mu[1] == 1.0 && s.l_cur == 1.0));
                        e_dec = std::fmax(e_dec, dec ? 0.0 : 1.0);
                        if (scaled && !(p.l0q < l0_min)) e_dec = 1.0;          // (the case must be one the rule declines)
                        continue;
                    }
                    allowed.push_back({F(O1, k), 8 * dd}); allowed.push_back({F(O2, k), 8 * dd});
                    const Bounds& b = scaled ? p.bq : p.bw;
                    const double c_ref = scaled ? b.u : b.c, inv12 = inv_s12(k, pairs);
                    e_c = std::fmax(e_c, std::fabs(s.c - c_ref * inv12) / (c_ref * inv12));
                    e_w = std::fmax(e_w, (words && q.failed == 0 && q.done == 0 && q.finished == 0 && q.upd_skip[0] == 0 && q.upd_skip[1] == 0) ? 0.0 : 1.0);
                    double mu0 = 1.0;
                    if (scaled) {
                        mu0 = s.mu[0];
                        e_mu = std::fmax(e_mu, std::fmax(std::fabs(s.mu[0] - p.mu0q), std::fmax(std::fabs(s.mu[1] - p.mu1q), std::fabs(s.l_cur - p.lq))));
                        if (!(p.l0q >= l0_min)) e_mu = 1.0;
                    }
                    const std::vector<double>& PPm = scaled ? p.PPq : p.PP;
                    const double inv_cn = 1.0 / c_ref, inv_c = inv_cn / inv12;
                    const float m1 = (float)(1.5 * mu0), m3 = (float)(0.5 * mu0 * mu0 * mu0);
                    const double* a64 = im.b<double>(F(A64, k));
                    HostSplit y1 = fetch_split(im.a<uint8_t>(F(O1, k)), d), z1 = fetch_split(im.a<uint8_t>(F(O2, k)), d);
                    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) {
                        const size_t i = (size_t)r * d + c;
                        const float y0 = (float)(a64[i] * inv_c);
                        const double want = (double)m1 * (double)y0 - (double)m3 * PPm[i] * (inv_cn * inv_cn);
                        e_y = std::fmax(e_y, std::fabs((double)y1.x[i] - want));
                        e_z = std::fmax(e_z, std::fabs((double)z1.x[i] - (double)host_round_split(((r == c) ? m1 : 0.f) - m3 * y0)));
                    }
                    e_o = std::fmax(e_o, std::fmax(max_abs_diff(y1.x, y1.xt), max_abs_diff(z1.x, z1.xt)));
                }
                const char* nm = scaled ? "FIRST scaled" : "FIRST";
                snprintf(buf, sizeof(buf), "%s %s: scale c of every problem (caller's units)", tag, nm); report(buf, e_c, 1e-12);
                snprintf(buf, sizeof(buf), "%s %s: state armed, traces and mean term kept", tag, nm); report(buf, e_w, 0.0);
                if (scaled) { snprintf(buf, sizeof(buf), "%s %s: mu[0], mu[1], l_cur of every problem vs host", tag, nm); report(buf, e_mu, 1e-5); }
                snprintf(buf, sizeof(buf), "%s %s: Y1 = 1.5 mu0 Y0 - 0.5 mu0^3 Y0^2 vs float64", tag, nm); report(buf, e_y, 3e-6);
                snprintf(buf, sizeof(buf), "%s %s: Z1 = T0 (split planes)", tag, nm); report(buf, e_z, scaled ? 1e-6 : 0.0);   // (scaled: the device contracts m1 - m3 y0 into one fma)
                snprintf(buf, sizeof(buf), "%s %s: planes of Y1^T / Z1^T hold the same values", tag, nm); report(buf, e_o, 0.0);
                if (nprob >= 3) { snprintf(buf, sizeof(buf), "%s %s: declined problem says failed / finished", tag, nm); report(buf, e_dec, 0.0); }
                snprintf(buf, sizeof(buf), "%s %s: guards, operands, declined and refused problems untouched", tag, nm); report(buf, im.touched_outside(allowed), 0.0);
            }

            // ---------------- SP_T, plain and with each problem's own mu[k]
            for (int scaled = 0; scaled < 2; ++scaled) {
                reset_outputs();
                for (int k = 0; k < nprob; ++k) {
                    NsState* s = im.b<NsState>(F(st, k)); s->mu[0] = 1.7; s->mu[1] = 1.05 + 0.02 * k; s->mu[2] = 1.01;
                    Ns32State* q = im.b<Ns32State>(F(s32, k)); memset(q, 0, sizeof(*q)); q->done = is_skip(k, nprob, pairs) ? 1 : 0;
                }
                im.upload();
                SplitArgs g = args();
                g.A[0] = mat(Z); g.B[0] = mat(Y); g.C[0] = mat(O1); g.alpha = -0.5f; g.beta_eye = 1.5f; g.gamma = 1.0f;
                g.partials = im.d<double>(F(partials, 0)); g.skip = &im.d<Ns32State>(F(s32, 0))->done; g.k = 1; g.scaled = scaled;
                run_big(nj, SP_T, d, nprob, g);
                im.fetch();
                std::vector<Region> allowed;
                double e_t = 0.0, e_o = 0.0, e_p = 0.0;
                for (int k = 0; k < nprob; ++k) {
                    if (is_bad(k, nprob, pairs) || is_skip(k, nprob, pairs)) continue;
                    allowed.push_back({F(O1, k), 8 * dd}); allowed.push_back({F(partials, k), (size_t)tiles * sizeof(double)});
                    const IterProb& p = pr[k];
                    const double m = 1.05 + 0.02 * k;
                    const float al = scaled ? (float)(-0.5 * m * m * m) : -0.5f, be = scaled ? (float)(1.5 * m) : 1.5f, ga = scaled ? be + al : 1.0f;
                    HostSplit ht = fetch_split(im.a<uint8_t>(F(O1, k)), d);
                    std::vector<double> ss(tiles, 0.0);
                    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) {
                        const size_t i = (size_t)r * d + c;
                        const double want = (double)al * p.ZY[i] + (r == c ? (double)be : 0.0);
                        e_t = std::fmax(e_t, std::fabs((double)ht.x[i] - want));
                        const double q = want - (r == c ? (double)ga : 0.0);
                        ss[(r / 128) * tx_n + c / tw] += q * q;                      // the kernel's own tile order: 128-row strips of tiles 64 NJ wide
                    }
                    e_o = std::fmax(e_o, max_abs_diff(ht.x, ht.xt));
                    const double* got = im.a<double>(F(partials, k));
                    for (int i = 0; i < tiles; ++i) e_p = std::fmax(e_p, std::fabs(got[i] - ss[i]) / ss[i]);
                }
                const char* nm = scaled ? "T scaled" : "T";
                snprintf(buf, sizeof(buf), "%s %s: T = 1.5 mu I - 0.5 mu^3 Z Y, every problem its mu[k]", tag, nm); report(buf, e_t, scaled ? 4e-6 : 3e-6);
                snprintf(buf, sizeof(buf), "%s %s: planes of T^T hold the same values", tag, nm); report(buf, e_o, 0.0);
                snprintf(buf, sizeof(buf), "%s %s: residual partials per tile (relative)", tag, nm); report(buf, e_p, 1e-3);
                snprintf(buf, sizeof(buf), "%s %s: guards, operands, skipped and refused problems untouched", tag, nm); report(buf, im.touched_outside(allowed), 0.0);
            }

            // ---------------- SP_U: Y' = Y T, Z' = T Z, digit planes of Y', the check of iteration 1 in the appended workgroups
            {
                reset_outputs();
                std::vector<double> res_ref(nprob);
                for (int k = 0; k < nprob; ++k) {
                    Ns32State* q = im.b<Ns32State>(F(s32, k)); memset(q, 0, sizeof(*q));
                    q->final_iter = -1; q->decided_at = -1; q->skip_corr = 1; q->res[0] = 1e300; q->res[1] = -7.0;
                    if (is_skip(k, nprob, pairs)) { q->upd_skip[1] = 1; q->finished = 1; q->done = 1; q->failed = 1; }
                    // what an SP_T launch would have left: residuals of 0.3 .. 0.7; problem 3's is small enough to predict the final iterate
                    const double want_res = (k == 3) ? 5e-4 : 0.3 + 0.4 * k / nprob;
                    double* pp = im.b<double>(F(partials, k)); double sum = 0.0;
                    for (int i = 0; i < tiles; ++i) { pp[i] = (want_res * want_res / 4.0) * (1.0 + 0.25 * (i % 3)) / tiles; sum += pp[i]; }
                    res_ref[k] = 2.0 * std::sqrt(sum);
                }
                im.upload();
                SplitArgs g = args();
                g.A[0] = mat(Y); g.B[0] = mat(T); g.C[0] = mat(O1); g.A[1] = mat(T); g.B[1] = mat(Z); g.C[1] = mat(O2);
                g.Cdig[0] = im.d<uint4>(F(dig, 0)); g.Cdig_t[0] = im.d<uint4>(F(digt, 0)); g.skip = &im.d<Ns32State>(F(s32, 0))->upd_skip[1];
                g.k = 1; g.max_low = 14; g.nslots = tiles; g.chk_partials = im.d<double>(F(partials, 0)); g.thr_pred = 2.5e-3 * d / 512.0;
                run_big(nj, SP_U, d, nprob, g);
                im.fetch();
                std::vector<Region> allowed;
                double e_y = 0.0, e_z = 0.0, e_o = 0.0, e_d = 0.0, e_r = 0.0, e_w = 0.0;
                for (int k = 0; k < nprob; ++k) {
                    allowed.push_back({F(s32, k), sizeof(Ns32State)});            // (the check workgroup of a problem runs whatever its header says)
                    const Ns32State q = *im.a<Ns32State>(F(s32, k)); const Ns32State q0 = *im.b<Ns32State>(F(s32, k));
                    if (is_skip(k, nprob, pairs)) {                                // closed earlier: the next update is switched off, nothing else moves
                        Ns32State w = q0; w.upd_skip[0] = 1;
                        e_w = std::fmax(e_w, same_s32(w, q) ? 0.0 : 1.0);
                    } else {
                        e_r = std::fmax(e_r, std::fabs(q.res[1] - res_ref[k]) / res_ref[k]);
                        Ns32State w = q0; w.res[1] = q.res[1];
                        if (k == 3) { w.ok = 1; w.skip_corr = 0; w.finished = 1; w.done = 1; w.final_iter = 2; w.decided_at = 1; w.upd_skip[0] = 1; }
                        e_w = std::fmax(e_w, same_s32(w, q) ? 0.0 : 1.0);
                    }
                    if (is_bad(k, nprob, pairs) || is_skip(k, nprob, pairs)) continue;
                    for (size_t f : {O1, O2}) allowed.push_back({F(f, k), 8 * dd});
                    allowed.push_back({F(dig, k), 6 * dd}); allowed.push_back({F(digt, k), 6 * dd});
                    const IterProb& p = pr[k];
                    HostSplit hy = fetch_split(im.a<uint8_t>(F(O1, k)), d), hz = fetch_split(im.a<uint8_t>(F(O2, k)), d);
                    for (size_t i = 0; i < dd; ++i) { e_y = std::fmax(e_y, std::fabs((double)hy.x[i] - p.YT[i])); e_z = std::fmax(e_z, std::fabs((double)hz.x[i] - p.TZ[i])); }
                    e_o = std::fmax(e_o, std::fmax(max_abs_diff(hy.x, hy.xt), max_abs_diff(hz.x, hz.xt)));
                    const int8_t* dgy = im.a<int8_t>(F(dig, k)); const int8_t* dgt = im.a<int8_t>(F(digt, k));
                    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c)
                        e_d = std::fmax(e_d, std::fmax(std::fabs(dig_value(dgy, r, c, d) - (double)hy.x[(size_t)r * d + c]), std::fabs(dig_value(dgt, c, r, d) - (double)hy.x[(size_t)r * d + c])));
                }
                snprintf(buf, sizeof(buf), "%s U: Y' = Y T", tag); report(buf, e_y, 3e-6);
                snprintf(buf, sizeof(buf), "%s U: Z' = T Z", tag); report(buf, e_z, 3e-6);
                snprintf(buf, sizeof(buf), "%s U: planes of Y'^T / Z'^T hold the same values", tag); report(buf, e_o, 0.0);
                snprintf(buf, sizeof(buf), "%s U: digit planes of Y' and Y'^T", tag); report(buf, e_d, kDigTol);
                snprintf(buf, sizeof(buf), "%s U: check workgroups recorded each problem's residual", tag); report(buf, e_r, 1e-3);
                snprintf(buf, sizeof(buf), "%s U: state words after the check (open / predicted / closed)", tag); report(buf, e_w, 0.0);
                snprintf(buf, sizeof(buf), "%s U: guards, operands, skipped and refused problems untouched", tag); report(buf, im.touched_outside(allowed), 0.0);
            }
        }
    im.release();
}

// =================================================================================================================================
// big_i8: nsf_i8_big<I8_A>, <I8_G>, <I8_G, true>
static void run_i8_big(int mode, bool withr, int d, int nprob, const I8Args& g) {
    static bool ready = false;
    if (!ready) {
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_i8_big<I8_A>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kI8BigLds));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_i8_big<I8_G>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kI8BigLds));
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_i8_big<I8_G, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kI8BigLds));
        ready = true;
    }
    const unsigned grid = (unsigned)big_grid(nprob, (d / 128) * (d / 64));
    if (mode == I8_A) hipLaunchKernelGGL((nsf_i8_big<I8_A>), dim3(grid), dim3(512), kI8BigLds, 0, g, nprob);
    else if (withr) hipLaunchKernelGGL((nsf_i8_big<I8_G, true>), dim3(grid), dim3(512), kI8BigLds, 0, g, nprob);
    else hipLaunchKernelGGL((nsf_i8_big<I8_G>), dim3(grid), dim3(512), kI8BigLds, 0, g, nprob);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
}

// a matrix on the fixed-point grid of 2^-40 that looks like a normalised covariance
static std::vector<double> grid_matrix(int d, uint64_t seed, double gain, int stepd) {
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> nd(0.0, 1.0);
    std::vector<double> m((size_t)d * d);
    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c)
        m[(size_t)r * d + c] = std::nearbyint(std::ldexp(gain * ((r == c ? 0.5 + 0.45 * ((r * stepd) % 13) / 13.0 : 0.0) + 0.03 * nd(rng)), 40)) * std::ldexp(1.0, -40);
    return m;
}

static void check_big_i8(int d, int nprob) {
    printf("== big_i8  d = %d, %d problems\n", d, nprob);
    const size_t dd = (size_t)d * d;
    const int nb = d / 32, gen = 900 + d + nprob;
    const size_t stat_bytes = (size_t)kTileStats * nb * nb * sizeof(double);
    char buf[200];

    {   // ---------------- I8_A: A = Sigma_a Sigma_b exact, planes of P, the tile statistics of nsf_i8<A>
        const std::vector<double> As = grid_matrix(d, 31000 + d, 1.0, 29);          // the shared baseline
        std::vector<std::vector<double>> Ak(nprob), Bt(nprob), An[2];
        An[0].resize(nprob); An[1].resize(nprob);
        parallel_for(nprob, [&](int k) { Ak[k] = grid_matrix(d, 32000 + 7 * d + k, 0.9, 31); Bt[k] = grid_matrix(d, 33000 + 11 * d + k, 0.5 + 0.02 * k, 23); });
        Layout L;
        const size_t hA = L.take(sizeof(MatHdr)), hB = L.take(sizeof(MatHdr)), skipw = L.take(sizeof(int)), st = L.take(sizeof(NsState));
        const size_t stats = L.take(stat_bytes), digA = L.take(6 * dd), digB = L.take(6 * dd), A64 = L.take(8 * dd), P = L.take(8 * dd);
        Layout S; const size_t s_hA = S.take(sizeof(MatHdr)), s_dig = S.take(6 * dd);
        const size_t stride = L.o + 4096, base = S.o;
        Image im; im.alloc(base + (size_t)nprob * stride);
        auto F = [&](size_t f, int k) { return base + f + (size_t)k * stride; };
        upload_digits(im.b<uint8_t>(s_dig), As, d, false);
        parallel_for(nprob, [&](int k) { upload_digits(im.b<uint8_t>(F(digA, k)), Ak[k], d, false); upload_digits(im.b<uint8_t>(F(digB, k)), Bt[k], d, false); });
        // the references: products of the values the planes hold (the B planes hold the rows of B^T)
        parallel_for(2 * nprob, [&](int job) {
            const int k = job >> 1, pairs = job & 1;
            const int8_t* da = pairs ? im.b<int8_t>(F(digA, k)) : im.b<int8_t>(s_dig); const int8_t* db = im.b<int8_t>(F(digB, k));
            std::vector<double> a(dd), bt(dd);
            for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) { a[(size_t)r * d + c] = dig_value(da, r, c, d); bt[(size_t)r * d + c] = dig_value(db, r, c, d); }
            An[pairs][k] = host_mm_t<long double>(a, bt, d);
        });
        for (int pairs = 0; pairs < 2; ++pairs) {
            const char* tag = pairs ? "pairs " : "shared";
            set_headers(im, s_hA, F(hA, 0), F(hB, 0), stride, nprob, pairs, gen);
            for (int k = 0; k < nprob; ++k) {
                *im.b<int>(F(skipw, k)) = is_skip(k, nprob, pairs) ? 1 : 0;
                memset(im.b<uint8_t>(F(st, k)), 0, sizeof(NsState));
                memset(im.b<uint8_t>(F(stats, k)), 0xEE, stat_bytes); memset(im.b<uint8_t>(F(A64, k)), 0xEE, 8 * dd); memset(im.b<uint8_t>(F(P, k)), 0xEE, 8 * dd);
            }
            im.upload();
            I8Args g; memset(&g, 0, sizeof(g));
            g.Adig = pairs ? im.d<uint4>(F(digA, 0)) : im.d<uint4>(s_dig); g.Bdig = im.d<uint4>(F(digB, 0)); g.d = d; g.gen = gen;
            g.hA = pairs ? im.d<MatHdr>(F(hA, 0)) : im.d<MatHdr>(s_hA); g.hB = im.d<MatHdr>(F(hB, 0));
            g.pstride = (int64_t)stride; g.astride = pairs ? (int64_t)stride : 0; g.skip = im.d<int>(F(skipw, 0));
            g.stats = im.d<double>(F(stats, 0)); g.A64 = im.d<double>(F(A64, 0)); g.P = dev_split(im.d<uint8_t>(F(P, 0)), d); g.st = im.d<NsState>(F(st, 0));
            run_i8_big(I8_A, false, d, nprob, g);
            im.fetch();
            std::vector<Region> allowed;
            double e_a = 0.0, e_p = 0.0, e_o = 0.0, e0 = 0.0, e1 = 0.0, e2 = 0.0;
            for (int k = 0; k < nprob; ++k) {
                if (is_bad(k, nprob, pairs) || is_skip(k, nprob, pairs)) continue;
                allowed.push_back({F(stats, k), stat_bytes}); allowed.push_back({F(A64, k), 8 * dd}); allowed.push_back({F(P, k), 8 * dd});
                const std::vector<double>& A = An[pairs][k];
                const double* a64 = im.a<double>(F(A64, k)); const double inv12 = inv_s12(k, pairs);
                HostSplit hp = fetch_split(im.a<uint8_t>(F(P, k)), d);
                double amax = 0.0, ep = 0.0;
                for (size_t i = 0; i < dd; ++i) {
                    e_a = std::fmax(e_a, std::fabs(a64[i] / inv12 - A[i]));
                    ep = std::fmax(ep, std::fabs((double)hp.x[i] - A[i])); amax = std::fmax(amax, std::fabs(A[i]));
                }
                e_p = std::fmax(e_p, ep / amax); e_o = std::fmax(e_o, max_abs_diff(hp.x, hp.xt));
                std::vector<double> want; tile_stats(A, d, want);
                const double* got = im.a<double>(F(stats, k));
                for (int t = 0; t < nb * nb; ++t) {
                    e0 = std::fmax(e0, std::fabs(got[4 * t] - want[4 * t]) / want[4 * t]);
                    e1 = std::fmax(e1, std::fabs(got[4 * t + 1] - want[4 * t + 1]));
                    e2 = std::fmax(e2, std::fmax(std::fabs(got[4 * t + 2] - want[4 * t + 2]) / want[4 * t + 2], std::fabs(got[4 * t + 3] - want[4 * t + 3]) / want[4 * t + 3]));
                }
            }
            snprintf(buf, sizeof(buf), "%s A: A (float64, normalised units) vs host product of the digits", tag); report(buf, e_a, 4e-15 * d / 512.0 + 1e-15);
            snprintf(buf, sizeof(buf), "%s A: split planes of P (relative to max |A|)", tag); report(buf, e_p, 3.0e-7);
            snprintf(buf, sizeof(buf), "%s A: planes of P^T hold the same values", tag); report(buf, e_o, 0.0);
            snprintf(buf, sizeof(buf), "%s A: per-tile sum a^2", tag); report(buf, e0, 1e-12);
            snprintf(buf, sizeof(buf), "%s A: per-tile trace share", tag); report(buf, e1, 1e-13);
            snprintf(buf, sizeof(buf), "%s A: per-tile largest row / column sum of |a|", tag); report(buf, e2, 1e-5);
            snprintf(buf, sizeof(buf), "%s A: guards, operands, skipped and refused problems untouched", tag); report(buf, im.touched_outside(allowed), 0.0);
        }
        im.release();
    }

    {   // ---------------- I8_G (shared baseline) and I8_G with the planes of kVerScale R (pairs): G = Y Y exact on the iterate `sel` selects
        struct GProb { std::vector<float> Y[2], Z[2]; std::vector<double> G, A2; double c; int sel; };
        std::vector<GProb> pr(nprob);
        parallel_for(nprob, [&](int k) {
            GProb& p = pr[k];
            std::mt19937_64 rng(55000 + 17 * d + k);
            std::normal_distribution<double> nd(0.0, 1.0);
            p.c = 0.5 + 0.1 * k; p.sel = 2 + ((k + k / 3) & 1);                  // even and odd final iterates side by side
            for (int s = 0; s < 2; ++s) {
                p.Y[s].resize(dd); p.Z[s].resize(dd);
                for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) {
                    const size_t i = (size_t)r * d + c;
                    p.Y[s][i] = host_round_split((float)((1.0 + 0.015 * k) * ((r == c ? (s ? 0.7 : 0.8) + 0.4 * ((r * (s ? 23 : 29)) % 13) / 13.0 : 0.0) + 0.004 * nd(rng))));
                    p.Z[s][i] = host_round_split((float)((r == c ? (s ? 1.3 : 1.2) - 0.4 * ((r * 31) % 7) / 7.0 : 0.0) + 0.004 * nd(rng)));
                }
            }
            const std::vector<float>& Yf = p.Y[p.sel & 1];
            p.G = host_mm(Yf, Yf, d);
            p.A2.resize(dd);
            for (size_t i = 0; i < dd; ++i) p.A2[i] = p.c * (p.G[i] + 1e-7 * nd(rng));              // R is small but not zero
        });
        Layout L;
        const size_t hA = L.take(sizeof(MatHdr)), hB = L.take(sizeof(MatHdr)), st = L.take(sizeof(NsState)), s32 = L.take(sizeof(Ns32State));
        size_t digY[2], digYt[2], Y[2], Z[2];
        for (int s = 0; s < 2; ++s) { digY[s] = L.take(6 * dd); digYt[s] = L.take(6 * dd); Y[s] = L.take(8 * dd); Z[s] = L.take(8 * dd); }
        const size_t A64 = L.take(8 * dd), Rv = L.take(8 * dd);
        Layout H;                                                                // what the host reads, hstride apart
        const size_t rec_bytes = (size_t)(kTileStats + 2) * nb * nb * sizeof(double);
        const size_t h_stats = H.take(rec_bytes), h_words = H.take(kHostWords * sizeof(int)), h_vals = H.take(kHostVals * sizeof(double));
        const size_t stride = L.o + 4096, hstride = H.o + 1024, base = 512, hbase = base + (size_t)nprob * stride;
        Image im; im.alloc(hbase + (size_t)nprob * hstride);
        auto F = [&](size_t f, int k) { return base + f + (size_t)k * stride; };
        auto FH = [&](size_t f, int k) { return hbase + f + (size_t)k * hstride; };
        parallel_for(nprob, [&](int k) {
            for (int s = 0; s < 2; ++s) {
                std::vector<double> y(pr[k].Y[s].begin(), pr[k].Y[s].end());
                upload_digits(im.b<uint8_t>(F(digY[s], k)), y, d, false); upload_digits(im.b<uint8_t>(F(digYt[s], k)), y, d, true);
                upload_split(im.b<uint8_t>(F(Y[s], k)), pr[k].Y[s], d); upload_split(im.b<uint8_t>(F(Z[s], k)), pr[k].Z[s], d);
            }
            memcpy(im.b<double>(F(A64, k)), pr[k].A2.data(), 8 * dd);
        });
        for (int pairs = 0; pairs < 2; ++pairs) {
            const bool withr = pairs != 0;
            const char* tag = withr ? "pairs  G+R" : "shared G";
            set_headers(im, 0, F(hA, 0), F(hB, 0), stride, nprob, pairs, gen);
            for (int k = 0; k < nprob; ++k) {
                NsState* s = im.b<NsState>(F(st, k)); memset(s, 0, sizeof(*s));
                s->c = pr[k].c; s->tr1 = tr_A(k, pairs); s->tr2 = 100.0 + k; s->mean_term = 0.25 + k; s->mu[0] = (k & 1) ? 1.0 : 1.3; s->too_few[1] = k & 1;
                Ns32State* q = im.b<Ns32State>(F(s32, k)); memset(q, 0, sizeof(*q));
                q->ok = 1; q->final_iter = pr[k].sel; q->decided_at = pr[k].sel - 1; q->finished = 1; q->done = 1; q->skip_corr = is_skip(k, nprob, pairs) ? 1 : 0; q->strict = k & 1;
                for (int i = 0; i < 16; ++i) q->res[i] = 0.001 * (i + 1) + k;
                memset(im.b<uint8_t>(F(Rv, k)), 0xEE, 8 * dd);
                memset(im.b<uint8_t>(FH(h_stats, k)), 0xEE, rec_bytes); memset(im.b<uint8_t>(FH(h_words, k)), 0xEE, kHostWords * sizeof(int)); memset(im.b<uint8_t>(FH(h_vals, k)), 0xEE, kHostVals * sizeof(double));
            }
            im.upload();
            I8Args g; memset(&g, 0, sizeof(g));
            g.Adig = im.d<uint4>(F(digY[0], 0)); g.Bdig = im.d<uint4>(F(digYt[0], 0)); g.Adig_alt = im.d<uint4>(F(digY[1], 0)); g.Bdig_alt = im.d<uint4>(F(digYt[1], 0));
            g.sel = &im.d<Ns32State>(F(s32, 0))->final_iter; g.skip = &im.d<Ns32State>(F(s32, 0))->skip_corr;
            g.d = d; g.gen = gen; g.hA = pairs ? im.d<MatHdr>(F(hA, 0)) : im.d<MatHdr>(0); g.hB = im.d<MatHdr>(F(hB, 0));
            g.pstride = (int64_t)stride; g.hstride = (int64_t)hstride; g.astride = pairs ? (int64_t)stride : 0;
            g.stats = im.d<double>(FH(h_stats, 0)); g.st = im.d<NsState>(F(st, 0)); g.A64in = im.d<double>(F(A64, 0)); g.s32 = im.d<Ns32State>(F(s32, 0));
            for (int s = 0; s < 2; ++s) { g.Y[s] = dev_split(im.d<uint8_t>(F(Y[s], 0)), d); g.Z[s] = dev_split(im.d<uint8_t>(F(Z[s], 0)), d); }
            g.host_words = im.d<int>(FH(h_words, 0)); g.host_vals = im.d<double>(FH(h_vals, 0)); g.scaled = 1;
            if (withr) g.Rv = dev_split(im.d<uint8_t>(F(Rv, 0)), d);
            run_i8_big(I8_G, withr, d, nprob, g);
            im.fetch();
            std::vector<Region> allowed;
            double e_c = 0.0, e_r2 = 0.0, e_t = 0.0, e_zm = 0.0, e_w = 0.0, e_v = 0.0, e_rv = 0.0, e_ro = 0.0;
            for (int k = 0; k < nprob; ++k) {
                const GProb& p = pr[k];
                // the snapshot is written for every problem, the skipped and the refused one included
                allowed.push_back({FH(h_words, k), 13 * sizeof(int)}); allowed.push_back({FH(h_words, k) + 14 * sizeof(int), sizeof(int)});
                allowed.push_back({FH(h_vals, k), 20 * sizeof(double)});
                const bool bad = is_bad(k, nprob, pairs), skipped = bad || is_skip(k, nprob, pairs);
                const int* hw = im.a<int>(FH(h_words, k)); const double* hv = im.a<double>(FH(h_vals, k));
                const NsState* s = im.b<NsState>(F(st, k)); const Ns32State* q = im.b<Ns32State>(F(s32, k));
                const bool words = hw[0] == (bad ? 1 : 0) && hw[1] == 0 && hw[2] == 0 && hw[3] == 0 && hw[4] == (k & 1) && hw[5] == 1 && hw[6] == 0 && hw[7] == p.sel &&
                                   hw[8] == p.sel - 1 && hw[9] == (k & 1) && hw[10] == 1 && hw[11] == (skipped ? 1 : 0) && hw[12] == gen && hw[14] == ((k & 1) ? 0 : 1);
                e_w = std::fmax(e_w, words ? 0.0 : 1.0);
                double ev = std::fabs(hv[0] - s->c) + std::fabs(hv[1] - s->tr1) + std::fabs(hv[2] - s->tr2) + std::fabs(hv[3] - s->mean_term);
                for (int i = 0; i < 16; ++i) ev += std::fabs(hv[4 + i] - q->res[i]);
                e_v = std::fmax(e_v, ev);
                if (skipped) continue;
                allowed.push_back({FH(h_stats, k), rec_bytes});
                if (withr) allowed.push_back({F(Rv, k), 8 * dd});
                const std::vector<float>& Yf = p.Y[p.sel & 1]; const std::vector<float>& Zf = p.Z[p.sel & 1];
                const double* sg = im.a<double>(FH(h_stats, k));
                double corr = 0.0, r2 = 0.0, trY = 0.0, c_got = 0.0, r_got = 0.0, t_got = 0.0, rmax = 0.0, er = 0.0;
                HostSplit hr; if (withr) hr = fetch_split(im.a<uint8_t>(F(Rv, k)), d);
                for (int r = 0; r < d; ++r) {
                    trY += Yf[(size_t)r * d + r];
                    for (int c = 0; c < d; ++c) {
                        const double R = p.A2[(size_t)r * d + c] / p.c - p.G[(size_t)r * d + c];
                        corr += (double)Zf[(size_t)c * d + r] * R; r2 += R * R;
                        if (withr) { er = std::fmax(er, std::fabs((double)hr.x[(size_t)r * d + c] - R * kVerScale)); rmax = std::fmax(rmax, std::fabs(R * kVerScale)); }
                    }
                }
                for (int i = 0; i < nb * nb; ++i) { c_got += sg[4 * i]; r_got += sg[4 * i + 1]; t_got += sg[4 * i + 2]; }
                e_c = std::fmax(e_c, std::fabs(c_got - corr)); e_r2 = std::fmax(e_r2, std::fabs(r_got - r2) / r2); e_t = std::fmax(e_t, std::fabs(t_got - trY));
                if (withr) { e_rv = std::fmax(e_rv, er / rmax); e_ro = std::fmax(e_ro, max_abs_diff(hr.x, hr.xt)); }
                // block (by, bx) of the record holds |Z| of rows 32 bx .. and columns 32 by ..: its largest partial row sum, then column sum.
                // The device adds float magnitudes in float64, as the host does: the two agree to rounding, so the bound dominates the
                // true sums (1 - got / true <= 1e-6, the single-problem check's slack) and is not loose either.
                const double* zmax = sg + (size_t)kTileStats * nb * nb;
                for (int by = 0; by < nb; ++by) for (int bx = 0; bx < nb; ++bx) {
                    double mrow = 0.0, mcol = 0.0, cs[32] = {0};
                    for (int zr = 0; zr < 32; ++zr) {
                        double rs = 0.0;
                        for (int zc = 0; zc < 32; ++zc) { const double a = std::fabs((double)Zf[(size_t)(32 * bx + zr) * d + 32 * by + zc]); rs += a; cs[zc] += a; }
                        mrow = std::fmax(mrow, rs);
                    }
                    for (int zc = 0; zc < 32; ++zc) mcol = std::fmax(mcol, cs[zc]);
                    e_zm = std::fmax(e_zm, std::fmax(std::fabs(1.0 - zmax[2 * (by * nb + bx)] / mrow), std::fabs(1.0 - zmax[2 * (by * nb + bx) + 1] / mcol)));
                }
            }
            snprintf(buf, sizeof(buf), "%s: tr(Z R) (absolute, |R| ~ 1e-7)", tag); report(buf, e_c, 2e-11 * d / 512.0);
            snprintf(buf, sizeof(buf), "%s: ||R||_F^2", tag); report(buf, e_r2, 1e-5);
            snprintf(buf, sizeof(buf), "%s: tr Y", tag); report(buf, e_t, 1e-10);
            snprintf(buf, sizeof(buf), "%s: |Z| row / column bounds per block dominate the true sums", tag); report(buf, e_zm, 1e-6);
            snprintf(buf, sizeof(buf), "%s: state snapshot per problem at hstride (words)", tag); report(buf, e_w, 0.0);
            snprintf(buf, sizeof(buf), "%s: state snapshot per problem at hstride (values)", tag); report(buf, e_v, 0.0);
            if (withr) {
                snprintf(buf, sizeof(buf), "%s: planes of kVerScale R (relative to max |R'|)", tag); report(buf, e_rv, 2e-3);
                snprintf(buf, sizeof(buf), "%s: planes of R'^T hold the same values", tag); report(buf, e_ro, 0.0);
            }
            snprintf(buf, sizeof(buf), "%s: guards, operands, skipped and refused problems untouched", tag); report(buf, im.touched_outside(allowed), 0.0);
        }
        im.release();
    }
}

// =================================================================================================================================
// res128: nsf_res128<false> and <true> (ns_fast_res.h): the whole iteration of a problem of D = 128 in one workgroup.
// Problems: A = Sigma_b Sigma_k from digit planes (shared baseline, one song per problem); even problems have a flat spectrum, odd ones decay
// like i^-0.5 (participation ratio ~80 of 128: above the 32 the chain asks for, below the 102 under which a scaled launch scales its steps);
// problem 2 of a batch of five or more has a refused header.  Each batch is launched plain and with scaled = 1.
// What can be held against host float64:
//   * <false> writes the planes of its final Y (both orientations) and Z^T: finite, the two orientations identical, ||I - Z Y||_F of those
//     planes against the residual the kernel recorded, ||A / c - Y Y||_F to the size of that residual, c and the words of both states.
//   * <true> writes A (exact product: K2's bound), c, the states and the host record.  Its iterate never leaves the chip, and a host run of
//     the iteration cannot reproduce the float32 accumulation order of the MFMAs, so tr(Z R), ||R||^2 and tr Y are NOT comparable one by
//     one at K8's tolerances.  What the record stands for is: tr sqrt(A) = sqrt(c) (tr Y + tr(Z R) / 2) up to est = zn^3 ||R||^2 / 8 +
//     zn res ||R|| / 2, zn^2 = ||Z||_1 ||Z||_inf (frechet.hip: fast_decide_one -- the second-order term of the root's expansion at Y^2 and
//     the part of the first-order term Z misses as an inverse of Y).  Two routes that each stay within their own est of the same number
//     differ by at most est_1 + est_2.  The record of <true> is held against (a) the tiled route nsf_i8<A> -> nsf_split -> nsf_digitize ->
//     nsf_i8<G> on the same digit planes and (b) the float64 correction the host forms itself on the planes <false> wrote.
//   * the rules of nsf_check are replayed on the recorded residuals: ok / final_iter / decided_at must be what they give.
static double host_scale_cap(double res, int d) { double rr = res / std::sqrt((double)d); if (!(rr < 0.66)) rr = 0.66; return std::sqrt(1.0 / (1.0 - rr)); }
struct Replay { int ok = 0, failed = 0, final_iter = -1, decided_at = -1; bool sure = true; };
static Replay replay_rules(const double* res, int max_low, double thr_pred, int scaled, double l0, int d) {
    Replay o;
    double l_cur = l0, mu = scaled ? host_step_scale(l_cur) : 1.0, prev = 1e300;
    bool grew = false;
    for (int k = 1; k < 16; ++k) {
        if (scaled && std::fabs(l_cur - 0.9) < 1e-3) o.sure = false;       // (the host's l0 differs from the device's in its last digits: see host_l0_from_participation)
        double lk = l_cur; mu = scaled ? host_step_scale(lk) : 1.0;
        if (scaled && k > 1) { const double cap = host_scale_cap(prev, d); if (cap < mu) mu = cap; }
        const double r = res[k];
        if (scaled) { if (r == r && r < 1.0) { const double lr = std::sqrt(1.0 - r); if (lr > l_cur) l_cur = lr; } l_cur = mu * l_cur * (3.0 - mu * mu * l_cur * l_cur) / 2.0; if (l_cur > 1.0) l_cur = 1.0; }
        const bool finite = (r == r) && !std::isinf(r);
        const bool grows = k >= 4 && r > prev && r > 1e-3;
        const bool give_up = grows && (!scaled || grew);
        grew = grows;
        if (!finite || k + 1 >= max_low || give_up) { o.failed = 1; o.final_iter = k; o.decided_at = k; return o; }
        if (r <= 1e-3 && (r > 0.3 * prev || r <= 1e-6)) { o.ok = 1; o.final_iter = k; o.decided_at = k; return o; }
        const double bound = 0.75 * r * r + 0.25 * r * r * r;
        prev = r;
        if (bound <= thr_pred && mu == 1.0) { o.ok = 1; o.final_iter = k + 1; o.decided_at = k; return o; }
    }
    o.failed = 1; return o;
}
// what the host makes of a record (frechet.hip: fast_decide_one): the trace estimate in the caller's units and the bound on what it neglects
struct Estimate { double tr, est, r2, corr, trY; };
static Estimate estimate_of(const double* sx, const int* hw, const double* hv, int nb) {
    double corr = 0.0, r2 = 0.0, tr = 0.0, zinf = 0.0, zone = 0.0;
    for (int t = 0; t < nb * nb; ++t) { corr += sx[kTileStats * t]; r2 += sx[kTileStats * t + 1]; tr += sx[kTileStats * t + 2]; }
    const double* zmax = sx + (size_t)kTileStats * nb * nb;
    for (int x = 0; x < nb; ++x) {
        double rs = 0.0, cs = 0.0;
        for (int y = 0; y < nb; ++y) { rs += zmax[2 * (y * nb + x)]; cs += zmax[2 * (x * nb + y) + 1]; }
        zinf = std::fmax(zinf, rs); zone = std::fmax(zone, cs);
    }
    const int fi = hw[7];
    double res = hv[4 + (fi & 15)];
    if (hw[8] == fi - 1) { const double rp = hv[4 + ((fi - 1) & 15)]; res = 0.75 * rp * rp + 0.25 * rp * rp * rp; if (res < 2e-6) res = 2e-6; }
    const double zn = std::sqrt(zinf * zone), rn = std::sqrt(r2), sc = std::sqrt(hv[0]);
    return Estimate{sc * (tr + 0.5 * corr), sc * (zn * zn * zn * rn * rn / 8.0 + zn * res * rn / 2.0), r2, corr, tr};
}

static void check_res128(int nprob) {
    printf("== res128  %d problems\n", nprob);
    constexpr int d = 128, nb = 4;
    const size_t dd = (size_t)d * d;
    const int gen = 1300 + nprob, max_low = 14;
    const double thr_pred = 2.5e-3 * d / 512.0, l0_scale = 1.0, sA = 0.5;
    const size_t stat_bytes = (size_t)kTileStats * nb * nb * sizeof(double), rec_bytes = (size_t)(kTileStats + 2) * nb * nb * sizeof(double);
    char buf[200];
    auto bad_k = [&](int k) { return nprob >= 5 && k == 2; };
    auto decays = [](int k) { return (k & 1) != 0; };
    auto inv12_of = [&](int k) { return 1.0 / (sA * scale_B(k)); };

    // ---- operands on the 2^-40 grid: symmetric, diagonal plus a little symmetric noise
    auto sym_grid = [&](uint64_t seed, double gain, int kind, int stepd) {
        std::mt19937_64 rng(seed); std::normal_distribution<double> nd(0.0, 1.0);
        std::vector<double> m(dd);
        for (int r = 0; r < d; ++r) for (int c = r; c < d; ++c) {
            const double dg = kind ? std::pow(1.0 + r, -0.5) : 0.55 + 0.4 * ((r * stepd) % 13) / 13.0;
            const double v = std::nearbyint(std::ldexp(gain * ((r == c ? dg : 0.0) + 0.0005 * nd(rng)), 40)) * std::ldexp(1.0, -40);
            m[(size_t)r * d + c] = v; m[(size_t)c * d + r] = v;
        }
        return m;
    };
    Layout S; const size_t s_hA = S.take(sizeof(MatHdr)), s_dig = S.take(6 * dd);
    Layout L;
    const size_t hB = L.take(sizeof(MatHdr)), st = L.take(sizeof(NsState)), s32 = L.take(sizeof(Ns32State)), stats = L.take(stat_bytes), partials = L.take(nb * nb * sizeof(double));
    const size_t digB = L.take(6 * dd), A64 = L.take(8 * dd), P = L.take(8 * dd), T = L.take(8 * dd);
    size_t Y[2], Z[2], digY[2], digYt[2];
    for (int s = 0; s < 2; ++s) { Y[s] = L.take(8 * dd); Z[s] = L.take(8 * dd); digY[s] = L.take(6 * dd); digYt[s] = L.take(6 * dd); }
    Layout H; const size_t h_stats = H.take(rec_bytes), h_words = H.take(kHostWords * sizeof(int)), h_vals = H.take(kHostVals * sizeof(double));
    const size_t stride = L.o + 4096, hstride = H.o + 1024, base = S.o, hbase = base + (size_t)nprob * stride;
    Image im; im.alloc(hbase + (size_t)nprob * hstride);
    auto F = [&](size_t f, int k) { return base + f + (size_t)k * stride; };
    auto FH = [&](size_t f, int k) { return hbase + f + (size_t)k * hstride; };
    upload_digits(im.b<uint8_t>(s_dig), sym_grid(91000, 1.0, 0, 29), d, false);
    std::vector<std::vector<double>> An(nprob);                              // the exact product in normalised units, from the planes as uploaded
    struct Sc { double c_tile, c_full, l0; bool taken; };
    std::vector<Sc> sc[2]; sc[0].resize(nprob); sc[1].resize(nprob);
    std::vector<std::vector<double>> statsH(nprob);
    parallel_for(nprob, [&](int k) {
        upload_digits(im.b<uint8_t>(F(digB, k)), sym_grid(92000 + k, 0.6 + 0.02 * (k % 16), decays(k) ? 1 : 0, 23 + (k % 5)), d, false);
        const int8_t* da = im.b<int8_t>(s_dig); const int8_t* db = im.b<int8_t>(F(digB, k));
        std::vector<double> a(dd), bt(dd);
        for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) { a[(size_t)r * d + c] = dig_value(da, r, c, d); bt[(size_t)r * d + c] = dig_value(db, r, c, d); }
        An[k] = host_mm_t<long double>(a, bt, d);
        tile_stats(An[k], d, statsH[k]);
        const Bounds bt_ = scale_from_stats(statsH[k], d);
        double fro2 = 0.0, tr = 0.0, one_b = 0.0;
        for (int c = 0; c < d; ++c) { double cs = 0.0; for (int r = 0; r < d; ++r) { const double v = An[k][(size_t)r * d + c]; fro2 += v * v; cs += std::fabs(v); if (r == c) tr += v; } one_b = std::fmax(one_b, cs); }
        double u = std::sqrt(fro2); if (one_b < u) u = one_b;
        double cf = u / 2.9; const double wm = fro2 / tr; if (wm > cf && wm <= u) cf = wm;
        const bool taken = tr * tr < 0.8 * d * fro2;                       // a scaled launch scales this problem's steps
        double l0 = host_l0_from_participation((float)(tr * tr / fro2), d) * l0_scale; if (l0 > 0.5) l0 = 0.5;
        for (int scaled = 0; scaled < 2; ++scaled) {
            Sc& q = sc[scaled][k];
            q.taken = scaled && taken; q.l0 = q.taken ? l0 : 1.0;
            q.c_tile = q.taken ? bt_.u : bt_.c; q.c_full = q.taken ? u : cf;
        }
        if (tr * tr < 0.25 * d * fro2) printf("      (problem %d would be declined: participation ratio %.1f)\n", k, tr * tr / fro2);
    });
    {
        const Bounds b0 = scale_from_stats(statsH[0], d), b1 = scale_from_stats(statsH[nprob > 1 ? 1 : 0], d);
        printf("      (participation ratio of problem 0: %.1f, of problem %d: %.1f of %d)\n", b0.tr * b0.tr / b0.fro2, nprob > 1 ? 1 : 0, b1.tr * b1.tr / b1.fro2, d);
        if (nprob > 1) report("res128: the odd problems decay enough for scaled steps, none is declined", (sc[1][1].taken && !sc[1][0].taken) ? 0.0 : 1.0, 0.0);
    }
    auto set_state = [&](int s32_fill) {
        MatHdr h; memset(&h, 0, sizeof(h)); h.s = sA; h.tr = 7.0; h.flag_gen = gen - 1; *im.b<MatHdr>(s_hA) = h;
        for (int k = 0; k < nprob; ++k) {
            MatHdr b; memset(&b, 0, sizeof(b)); b.s = scale_B(k); b.tr = 100.0 + k; b.flag_gen = gen - 1;
            if (bad_k(k)) { if (nprob & 1) b.flag_gen = gen; else b.bad = 1; }
            *im.b<MatHdr>(F(hB, k)) = b;
            NsState* s = im.b<NsState>(F(st, k)); memset(s, 0, sizeof(*s)); s->mean_term = 0.25 + k;
            memset(im.b<uint8_t>(F(s32, k)), s32_fill, sizeof(Ns32State));
            for (size_t f : {Y[0], Y[1], Z[0], Z[1], P, T}) memset(im.b<uint8_t>(F(f, k)), 0xEE, 8 * dd);
            for (size_t f : {digY[0], digY[1], digYt[0], digYt[1]}) memset(im.b<uint8_t>(F(f, k)), 0xEE, 6 * dd);
            memset(im.b<uint8_t>(F(partials, k)), 0xEE, nb * nb * sizeof(double));
            memset(im.b<uint8_t>(FH(h_stats, k)), 0xEE, rec_bytes); memset(im.b<uint8_t>(FH(h_words, k)), 0xEE, kHostWords * sizeof(int)); memset(im.b<uint8_t>(FH(h_vals, k)), 0xEE, kHostVals * sizeof(double));
        }
    };
    auto res_args = [&](int scaled) {
        ResArgs r; memset(&r, 0, sizeof(r));
        r.gen = gen; r.max_low = max_low; r.thr_pred = thr_pred; r.hA = im.d<MatHdr>(s_hA); r.hB = im.d<MatHdr>(F(hB, 0)); r.pstride = (int64_t)stride;
        r.A64 = im.d<double>(F(A64, 0)); r.statsA = im.d<double>(F(stats, 0)); r.st = im.d<NsState>(F(st, 0)); r.s32 = im.d<Ns32State>(F(s32, 0));
        for (int s = 0; s < 2; ++s) { r.Y[s] = dev_split(im.d<uint8_t>(F(Y[s], 0)), d); r.Z[s] = dev_split(im.d<uint8_t>(F(Z[s], 0)), d); }
        r.scaled = scaled; r.l0_scale = l0_scale;
        return r;
    };
    // the words both kernels must leave, against the replay of the rules on the residuals they recorded
    auto check_words = [&](const NsState& s, const Ns32State& q, const Sc& w, int scaled, double c_ref, int k, double& e_c, double& e_w, double& e_rule, int& unsure) {
        e_c = std::fmax(e_c, std::fabs(s.c - c_ref * inv12_of(k)) / (c_ref * inv12_of(k)));
        const bool words = s.tr1 == 7.0 && s.tr2 == 100.0 + k && s.mean_term == 0.25 + k && s.done == 0 && s.nonfinite == 0 && q.finished == 1 && q.done == 1 &&
                           q.upd_skip[0] == 1 && q.upd_skip[1] == 1 && q.skip_corr == (q.ok ? 0 : 1) && q.failed == (q.ok ? 0 : 1) && q.strict == 0;
        e_w = std::fmax(e_w, words ? 0.0 : 1.0);
        const Replay rp = replay_rules(q.res, max_low, thr_pred, scaled, w.l0, d);
        if (!rp.sure) { ++unsure; return; }
        e_rule = std::fmax(e_rule, (rp.ok == q.ok && rp.failed == q.failed && rp.final_iter == q.final_iter && rp.decided_at == q.decided_at) ? 0.0 : 1.0);
    };

    struct Fin { int ok = 0; double tr = 0.0, est = 0.0; };
    std::vector<Fin> fin_host[2], fin_full[2], fin_tiled(nprob);
    for (int scaled = 0; scaled < 2; ++scaled) {
        char tag[32]; snprintf(tag, sizeof(tag), scaled ? "scaled" : "plain ");
        fin_host[scaled].resize(nprob); fin_full[scaled].resize(nprob);
        // ---------------- nsf_res128<false>: A and its tile statistics given, the final iterate's planes out
        set_state(0x55);
        for (int k = 0; k < nprob; ++k) {
            double* a64 = im.b<double>(F(A64, k)); for (size_t i = 0; i < dd; ++i) a64[i] = An[k][i] * inv12_of(k);
            memcpy(im.b<double>(F(stats, k)), statsH[k].data(), stat_bytes);
        }
        im.upload();
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_res128<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kResLds));
        hipLaunchKernelGGL(nsf_res128<false>, dim3((unsigned)nprob), dim3(256), kResLds, 0, res_args(scaled));
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        im.fetch();
        {
            std::vector<Region> allowed;
            double e_c = 0.0, e_w = 0.0, e_rule = 0.0, e_fin = 0.0, e_o = 0.0, e_res = 0.0, e_yy = 0.0;
            int unsure = 0, n_flat_open = 0;
            for (int k = 0; k < nprob; ++k) {
                if (bad_k(k)) continue;
                allowed.push_back({F(st, k), sizeof(NsState)}); allowed.push_back({F(s32, k), sizeof(Ns32State)});
                const NsState s = *im.a<NsState>(F(st, k)); const Ns32State q = *im.a<Ns32State>(F(s32, k));
                const Sc& w = sc[scaled][k];
                check_words(s, q, w, scaled, w.c_tile, k, e_c, e_w, e_rule, unsure);
                if (!q.ok || q.final_iter < 1 || q.final_iter > 15) { if (!decays(k)) ++n_flat_open; continue; }        // (a problem that failed leaves no planes: everything of it must be untouched)
                const int par = q.final_iter & 1;
                allowed.push_back({F(Y[par], k), 8 * dd}); allowed.push_back({F(Z[par], k) + 4 * dd, 4 * dd});
                HostSplit hy = fetch_split(im.a<uint8_t>(F(Y[par], k)), d);
                std::vector<float> zt(dd);                                    // Z^T planes only: Z[r][c] sits at (c, r) of them
                { const uint16_t* at = reinterpret_cast<const uint16_t*>(im.a<uint8_t>(F(Z[par], k)) + 4 * dd); for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) zt[(size_t)r * d + c] = fa_value(at, c, r, d); }
                bool finite = true; for (size_t i = 0; i < dd; ++i) finite = finite && std::isfinite(hy.x[i]) && std::isfinite(hy.xt[i]) && std::isfinite(zt[i]);
                e_fin = std::fmax(e_fin, finite ? 0.0 : 1.0); e_o = std::fmax(e_o, max_abs_diff(hy.x, hy.xt));
                const std::vector<double> ZY = host_mm(zt, hy.x, d), YY = host_mm(hy.x, hy.x, d);
                const double c = w.c_tile;
                double r_host = 0.0, rr2 = 0.0, corr = 0.0, trY = 0.0, nA = 0.0, zinf = 0.0, zone = 0.0;
                std::vector<double> cs(d, 0.0);
                for (int r = 0; r < d; ++r) {
                    double rs = 0.0;
                    for (int cc = 0; cc < d; ++cc) {
                        const size_t i = (size_t)r * d + cc;
                        const double e = (r == cc ? 1.0 : 0.0) - ZY[i]; r_host += e * e;
                        const double R = An[k][i] / c - YY[i]; rr2 += R * R; nA += (An[k][i] / c) * (An[k][i] / c);
                        corr += (double)zt[(size_t)cc * d + r] * R;
                        rs += std::fabs((double)zt[i]); cs[cc] += std::fabs((double)zt[i]);
                    }
                    trY += hy.x[(size_t)r * d + r]; zinf = std::fmax(zinf, rs);
                }
                for (int cc = 0; cc < d; ++cc) zone = std::fmax(zone, cs[cc]);
                r_host = std::sqrt(r_host); nA = std::sqrt(nA);
                // The residual the kernel vouches for its final iterate with: the one it measured on it (closed at the floor), or the bound
                // 0.75 r^2 + 0.25 r^3 of the step it predicted from (nsf_check).  The device forms Z Y on the float32-accumulating MFMA: every
                // element within 3e-6 of the exact product (nsfast_check's bound for the same product, K4 / K5), so the two Frobenius norms
                // differ by at most 3e-6 d, next to K5's 1e-3 relative.
                const bool floor_ = q.final_iter == q.decided_at;
                const double rp = q.res[q.decided_at & 15], r_rec = floor_ ? rp : 0.75 * rp * rp + 0.25 * rp * rp * rp, noise = 3e-6 * d;
                const double e1 = floor_ ? std::fabs(r_host - r_rec) - 1e-3 * r_rec : r_host - r_rec * (1.0 + 1e-3);
                e_res = std::fmax(e_res, e1 / noise);
                // Y = (A / c) Z in exact arithmetic, so Y Y - A / c = (A / c) (Z Y - I): at most ||A / c||_F r.  Each iteration's products
                // add at most 3e-6 per element to Y (3e-6 d in norm), which Y Y doubles (||Y||_2 <= 1).
                e_yy = std::fmax(e_yy, std::sqrt(rr2) / (nA * (r_host + noise) + 2.0 * noise * q.final_iter));
                if (k < 3) printf("      (%s problem %d: final_iter %d decided_at %d  ||I - Z Y|| host %.3e recorded %.3e  ||A/c - Y Y|| %.3e)\n", tag, k, q.final_iter, q.decided_at, r_host, r_rec, std::sqrt(rr2));
                const double zn = std::sqrt(zinf * zone), rn = std::sqrt(rr2), rb = floor_ ? std::fmax(r_host, r_rec) : std::fmax(r_rec, 2e-6);
                const double scc = std::sqrt(c * inv12_of(k));
                fin_host[scaled][k] = Fin{1, scc * (trY + 0.5 * corr), scc * (zn * zn * zn * rn * rn / 8.0 + zn * rb * rn / 2.0)};
            }
            snprintf(buf, sizeof(buf), "%s res: scale c of every problem (caller's units)", tag); report(buf, e_c, 1e-12);
            snprintf(buf, sizeof(buf), "%s res: state words closed, traces and mean term kept", tag); report(buf, e_w, 0.0);
            snprintf(buf, sizeof(buf), "%s res: ok / final_iter / decided_at follow nsf_check's rules on res[]", tag); report(buf, e_rule, 0.0);
            if (unsure) printf("      (%d problem(s) with a step bound within 1e-3 of 0.9: rules not replayed)\n", unsure);
            snprintf(buf, sizeof(buf), "%s res: every flat problem converged", tag); report(buf, (double)n_flat_open, 0.0);
            snprintf(buf, sizeof(buf), "%s res: final Y, Y^T, Z^T finite", tag); report(buf, e_fin, 0.0);
            snprintf(buf, sizeof(buf), "%s res: planes of Y^T hold the same values", tag); report(buf, e_o, 0.0);
            snprintf(buf, sizeof(buf), "%s res: ||I - Z Y||_F vs the recorded residual (excess / 3e-6 d)", tag); report(buf, e_res, 1.0);
            snprintf(buf, sizeof(buf), "%s res: ||A/c - Y Y||_F within the residual's size (ratio)", tag); report(buf, e_yy, 1.0);
            snprintf(buf, sizeof(buf), "%s res: guards, operands, other planes, failed and refused problems untouched", tag); report(buf, im.touched_outside(allowed), 0.0);
        }

        // ---------------- nsf_res128<true>: digit planes in, A, the states and the host record out
        set_state(0x55);
        for (int k = 0; k < nprob; ++k) { memset(im.b<uint8_t>(F(A64, k)), 0xEE, 8 * dd); memset(im.b<uint8_t>(F(stats, k)), 0xEE, stat_bytes); }
        im.upload();
        {
            ResArgs r = res_args(scaled);
            r.Adig = im.d<uint4>(s_dig); r.Bdig = im.d<uint4>(F(digB, 0)); r.hstride = (int64_t)hstride;
            r.stats = im.d<double>(FH(h_stats, 0)); r.host_words = im.d<int>(FH(h_words, 0)); r.host_vals = im.d<double>(FH(h_vals, 0));
            CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nsf_res128<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kResLdsFull));
            hipLaunchKernelGGL(nsf_res128<true>, dim3((unsigned)nprob), dim3(256), kResLdsFull, 0, r);
            CK(hipGetLastError()); CK(hipDeviceSynchronize());
        }
        im.fetch();
        {
            std::vector<Region> allowed;
            double e_a = 0.0, e_c = 0.0, e_w = 0.0, e_rule = 0.0, e_snap = 0.0, e_rec = 0.0, e_bad = 0.0;
            int unsure = 0;
            for (int k = 0; k < nprob; ++k) {
                const int* hw = im.a<int>(FH(h_words, k)); const double* hv = im.a<double>(FH(h_vals, k));
                allowed.push_back({FH(h_words, k), 13 * sizeof(int)}); allowed.push_back({FH(h_vals, k), 20 * sizeof(double)});
                if (bad_k(k)) { e_bad = std::fmax(e_bad, (hw[0] == 1 && hw[11] == 1 && hw[12] == gen) ? 0.0 : 1.0); continue; }
                allowed.push_back({F(st, k), sizeof(NsState)}); allowed.push_back({F(s32, k), sizeof(Ns32State)}); allowed.push_back({F(A64, k), 8 * dd});
                const NsState s = *im.a<NsState>(F(st, k)); const Ns32State q = *im.a<Ns32State>(F(s32, k));
                const Sc& w = sc[scaled][k];
                const double* a64 = im.a<double>(F(A64, k));
                for (size_t i = 0; i < dd; ++i) e_a = std::fmax(e_a, std::fabs(a64[i] / inv12_of(k) - An[k][i]));
                check_words(s, q, w, scaled, w.c_full, k, e_c, e_w, e_rule, unsure);
                // the snapshot: the words and values of the states as the kernel left them
                bool snap = hw[0] == 0 && hw[1] == s.done && hw[2] == s.nonfinite && hw[3] == s.too_few[0] && hw[4] == s.too_few[1] && hw[5] == q.ok && hw[6] == q.failed &&
                            hw[7] == q.final_iter && hw[8] == q.decided_at && hw[9] == q.strict && hw[10] == q.finished && hw[11] == (q.ok ? 0 : 1) && hw[12] == gen &&
                            hv[0] == s.c && hv[1] == s.tr1 && hv[2] == s.tr2 && hv[3] == s.mean_term;
                for (int i = 1; i <= q.decided_at && i < 16; ++i) snap = snap && hv[4 + i] == q.res[i];
                e_snap = std::fmax(e_snap, snap ? 0.0 : 1.0);
                if (!q.ok) continue;
                allowed.push_back({FH(h_stats, k), rec_bytes});
                const double* sx = im.a<double>(FH(h_stats, k));
                bool rec = std::isfinite(sx[0]) && sx[1] > 0.0 && std::isfinite(sx[1]) && sx[2] > 0.0 && std::isfinite(sx[2]) && sx[kTileStats * nb * nb] > 0.0 && sx[kTileStats * nb * nb + 1] > 0.0;
                for (int i = 3; i < (kTileStats + 2) * nb * nb; ++i) if (i != kTileStats * nb * nb && i != kTileStats * nb * nb + 1) rec = rec && sx[i] == 0.0;
                e_rec = std::fmax(e_rec, rec ? 0.0 : 1.0);
                const Estimate e = estimate_of(sx, hw, hv, nb);
                fin_full[scaled][k] = Fin{1, e.tr, e.est};
            }
            snprintf(buf, sizeof(buf), "%s full: A (float64, normalised units) vs host product of the digits", tag); report(buf, e_a, 4e-15 * d / 512.0 + 1e-15);
            snprintf(buf, sizeof(buf), "%s full: scale c from the exact ||A||_1, ||A||_F, tr A", tag); report(buf, e_c, 1e-12);
            snprintf(buf, sizeof(buf), "%s full: state words closed, traces and mean term kept", tag); report(buf, e_w, 0.0);
            snprintf(buf, sizeof(buf), "%s full: ok / final_iter / decided_at follow nsf_check's rules on res[]", tag); report(buf, e_rule, 0.0);
            if (unsure) printf("      (%d problem(s) with a step bound within 1e-3 of 0.9: rules not replayed)\n", unsure);
            snprintf(buf, sizeof(buf), "%s full: host snapshot holds the states as left", tag); report(buf, e_snap, 0.0);
            snprintf(buf, sizeof(buf), "%s full: record finite, norms filed under tile (0, 0), the rest zero", tag); report(buf, e_rec, 0.0);
            if (nprob >= 5) { snprintf(buf, sizeof(buf), "%s full: refused problem's snapshot says bad / skipped", tag); report(buf, e_bad, 0.0); }
            snprintf(buf, sizeof(buf), "%s full: guards, operands, planes, failed and refused problems untouched", tag); report(buf, im.touched_outside(allowed), 0.0);
        }
    }

    // ---------------- the tiled route on the same planes (plain steps): nsf_i8<A>, nsf_split<FIRST>, (T, U) x 13, nsf_digitize, nsf_i8<G>
    set_state(0);
    for (int k = 0; k < nprob; ++k) { memset(im.b<uint8_t>(F(A64, k)), 0xEE, 8 * dd); memset(im.b<uint8_t>(F(stats, k)), 0xEE, stat_bytes); }
    im.upload();
    {
        auto mat = [&](size_t f) { return dev_split(im.d<uint8_t>(F(f, 0)), d); };
        const unsigned B = (unsigned)nprob;
        I8Args a; memset(&a, 0, sizeof(a));
        a.Adig = im.d<uint4>(s_dig); a.Bdig = im.d<uint4>(F(digB, 0)); a.d = d; a.gen = gen; a.hA = im.d<MatHdr>(s_hA); a.hB = im.d<MatHdr>(F(hB, 0)); a.pstride = (int64_t)stride;
        a.stats = im.d<double>(F(stats, 0)); a.A64 = im.d<double>(F(A64, 0)); a.P = mat(P); a.st = im.d<NsState>(F(st, 0));
        hipLaunchKernelGGL((nsf_i8<1, I8_A>), dim3(nb, nb, B), dim3(512), 0, 0, a);
        auto split_args = [&]() {
            SplitArgs g; memset(&g, 0, sizeof(g));
            g.d = d; g.gen = gen; g.hA = im.d<MatHdr>(s_hA); g.hB = im.d<MatHdr>(F(hB, 0)); g.pstride = (int64_t)stride; g.st = im.d<NsState>(F(st, 0)); g.s32 = im.d<Ns32State>(F(s32, 0));
            return g;
        };
        Ns32State* s32_0 = im.d<Ns32State>(F(s32, 0));
        SplitArgs g = split_args();
        g.A[0] = mat(P); g.B[0] = mat(P); g.C[0] = mat(Y[1]); g.C[1] = mat(Z[1]); g.A64 = im.d<double>(F(A64, 0)); g.statsA = im.d<double>(F(stats, 0));
        hipLaunchKernelGGL((nsf_split<1, SP_FIRST>), dim3(nb, nb, B), dim3(512), 0, 0, g);
        for (int k = 1; k < max_low; ++k) {
            const int cur = k & 1;
            g = split_args();
            g.A[0] = mat(Z[cur]); g.B[0] = mat(Y[cur]); g.C[0] = mat(T); g.alpha = -0.5f; g.beta_eye = 1.5f; g.gamma = 1.0f;
            g.partials = im.d<double>(F(partials, 0)); g.skip = &s32_0->done; g.k = k;
            hipLaunchKernelGGL((nsf_split<1, SP_T>), dim3(nb, nb, B), dim3(512), 0, 0, g);
            g = split_args();
            g.A[0] = mat(Y[cur]); g.B[0] = mat(T); g.C[0] = mat(Y[cur ^ 1]); g.A[1] = mat(T); g.B[1] = mat(Z[cur]); g.C[1] = mat(Z[cur ^ 1]);
            g.skip = &s32_0->upd_skip[k & 1]; g.k = k; g.max_low = max_low; g.nslots = nb * nb; g.chk_partials = im.d<double>(F(partials, 0)); g.thr_pred = thr_pred;
            hipLaunchKernelGGL((nsf_split<1, SP_U>), dim3(nb, nb, 3 * B), dim3(512), 0, 0, g);
        }
        DigArgs dg; memset(&dg, 0, sizeof(dg));
        dg.d = d; dg.gen = gen; dg.hA = im.d<MatHdr>(s_hA); dg.hB = im.d<MatHdr>(F(hB, 0)); dg.pstride = (int64_t)stride; dg.s32 = s32_0;
        for (int s = 0; s < 2; ++s) { dg.Y[s] = mat(Y[s]); dg.dig[s] = im.d<uint4>(F(digY[s], 0)); dg.dig_t[s] = im.d<uint4>(F(digYt[s], 0)); }
        hipLaunchKernelGGL(nsf_digitize, dim3((unsigned)((dd / 16 + 255) / 256), 2, B), dim3(256), 0, 0, dg);
        memset(&a, 0, sizeof(a));
        a.Adig = dg.dig[0]; a.Bdig = dg.dig_t[0]; a.Adig_alt = dg.dig[1]; a.Bdig_alt = dg.dig_t[1]; a.sel = &s32_0->final_iter;
        a.d = d; a.gen = gen; a.hA = im.d<MatHdr>(s_hA); a.hB = im.d<MatHdr>(F(hB, 0)); a.pstride = (int64_t)stride; a.hstride = (int64_t)hstride;
        a.skip = &s32_0->skip_corr; a.stats = im.d<double>(FH(h_stats, 0)); a.st = im.d<NsState>(F(st, 0)); a.A64in = im.d<double>(F(A64, 0));
        for (int s = 0; s < 2; ++s) { a.Y[s] = mat(Y[s]); a.Z[s] = mat(Z[s]); }
        a.s32 = s32_0; a.host_words = im.d<int>(FH(h_words, 0)); a.host_vals = im.d<double>(FH(h_vals, 0));
        hipLaunchKernelGGL((nsf_i8<1, I8_G>), dim3(nb, nb, B), dim3(512), 0, 0, a);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
    }
    im.fetch();
    for (int k = 0; k < nprob; ++k) {
        const int* hw = im.a<int>(FH(h_words, k)); const double* hv = im.a<double>(FH(h_vals, k));
        if (bad_k(k) || hw[12] != gen || hw[0] || hw[1] || hw[6] || !hw[5] || hw[11]) continue;
        const Estimate e = estimate_of(im.a<double>(FH(h_stats, k)), hw, hv, nb);
        fin_tiled[k] = Fin{1, e.tr, e.est};
    }
    for (int scaled = 0; scaled < 2; ++scaled) {
        double e_t = 0.0, e_h = 0.0; int n_missing = 0;
        for (int k = 0; k < nprob; ++k) {
            const Fin& f = fin_full[scaled][k];
            const Fin& t = fin_tiled[k]; const Fin& h = fin_host[scaled][k];
            if (!bad_k(k) && !decays(k) && !(f.ok && t.ok && h.ok)) ++n_missing;
            if (!f.ok) continue;
            if (t.ok) { e_t = std::fmax(e_t, std::fabs(f.tr - t.tr) / (f.est + t.est)); }
            if (h.ok) { e_h = std::fmax(e_h, std::fabs(f.tr - h.tr) / (f.est + h.est)); }
            if (k < 3) printf("      (%s problem %d: tr sqrt A  full %.12e +- %.1e  tiled %.12e +- %.1e  host on <false> %.12e +- %.1e)\n", scaled ? "scaled" : "plain ", k, f.tr, f.est, t.tr, t.est, h.tr, h.est);
        }
        const char* tag = scaled ? "scaled" : "plain ";
        snprintf(buf, sizeof(buf), "%s full: every flat problem converged on all three routes", tag); report(buf, (double)n_missing, 0.0);
        snprintf(buf, sizeof(buf), "%s full: sqrt(c) (tr Y + tr(Z R) / 2) vs the tiled route (/ (est + est))", tag); report(buf, e_t, 1.0);
        snprintf(buf, sizeof(buf), "%s full: sqrt(c) (tr Y + tr(Z R) / 2) vs host float64 on <false>'s planes", tag); report(buf, e_h, 1.0);
    }
    im.release();
}

int main(int argc, char** argv) {
    const std::string section = argc > 1 ? argv[1] : "";
    if (section != "big_iter" && section != "big_i8" && section != "res128") { printf("usage: nsbig_check big_iter|big_i8 [d:nprob ...] | res128 [nprob ...]\n"); return 2; }
    if (section == "res128") {
        std::vector<int> batches;
        for (int i = 2; i < argc; ++i) { const int n = atoi(argv[i]); if (n < 1 || n > 64) { printf("bad batch %s (1 .. 64)\n", argv[i]); return 2; } batches.push_back(n); }
        if (batches.empty()) batches = {1, 5, 64};
        for (int n : batches) check_res128(n);
        printf(g_fail ? "FAILED: %d check(s)\n" : "all checks passed\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::vector<std::pair<int, int>> shapes;
    for (int i = 2; i < argc; ++i) {
        int d = 0, n = 0;
        if (sscanf(argv[i], "%d:%d", &d, &n) != 2 || (d != 256 && d != 384 && d != 512 && d != 768 && d != 1024) || n < 1 || n > 32) { printf("bad shape %s (d:nprob)\n", argv[i]); return 2; }
        shapes.push_back({d, n});
    }
    if (shapes.empty()) shapes = {{256, 1}, {256, 7}, {256, 8}, {256, 9}, {256, 20}, {384, 3}, {384, 9}, {768, 3}, {768, 9}, {512, 3}, {1024, 3}};
    for (auto s : shapes) { if (section == "big_iter") check_big_iter(s.first, s.second); else check_big_i8(s.first, s.second); }
    printf(g_fail ? "FAILED: %d check(s)\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
