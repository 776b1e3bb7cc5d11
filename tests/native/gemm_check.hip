// Element-by-element check of the MFMA GEMM kernels (fadtk_amd/csrc/gemm_f64.hip, gemm_f32.hip) on the GPU against host arithmetic
// in long double (test infrastructure, gfx950).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/gemm_check tests/native/gemm_check.hip && tests/native/gemm_check [section ...]
// Sections: f64 (gemm_f64_launch: every instantiation, every feature), f64big (more problems than grid layers), stats (the
// fp32-operand / statistics epilogues: gemm_f64_product_stats_launch, gemm_f64_correction_launch), f32 (gemm_f32.hip).  No argument =
// all.  Exit code 0 = all checks passed, 1 = a check failed, 2 = a HIP error.
//
// The two translation units are included as they are; the three host symbols they need are supplied here, and num_cus() returns a
// global this tool sets: that is what makes every instantiation reachable on purpose at small d (1 -> always 64 x 64 tiles;
// huge -> always 32 x 32 and, for d % 64 == 0, the 8-wave kernel; work64 + 1 -> the 4-wave 32 x 32 kernel).
//
// Reference and tolerance (derived, not measured).  The host accumulates ref_ij = sum_k a_ik b_kj and S_ij = sum_k |a_ik| |b_kj| in
// long double over the same double / float operand values.  Any order of IEEE multiply-adds satisfies |fl(sum a b) - sum a b| <= g_n S
// with g_n = n u / (1 - n u); alpha * acc + beta adds two roundings, so element (i, j) must satisfy
//     |C_ij - (alpha ref_ij + beta delta_ij)| <= (d + 2) u (|alpha| S_ij + |beta| delta_ij),    u = 2^-53 (fp64 kernels), 2^-24 (gemm_f32)
// and every check of that kind prints  max_ij err / bound  and passes at <= 1.  (The long double reference itself is off by at most
// (d + 1) 2^-64 S: 1/2048 of the fp64 bound, nothing of the fp32 one.)  Reduced statistics compose the same way; the two shapes are
// SqAcc (sums of squares) and LinAcc (plain sums) below, each with its formula.
// Every output buffer is filled with 0xEE bytes before each launch, so what nobody wrote (a missed tile, a skipped problem, the padding
// between problems) is told from what was written, bit for bit.
#include "../../fadtk_amd/csrc/gemm_f64.hip"
#include "../../fadtk_amd/csrc/gemm_f32.hip"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

static int g_num_cus = 256;
namespace fad {
char* err_buf() { static thread_local char buf[512]; return buf; }
int set_error(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(err_buf(), 512, fmt, ap); va_end(ap);
    return code;
}
int num_cus(int) { return g_num_cus; }
}  // namespace fad

using namespace fad;
typedef long double ld;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

static const double U64 = 0x1p-53, U32 = 0x1p-24;
static int g_fail = 0, g_checks = 0;
static double g_max_ratio = 0.0;
static void report(const char* what, double err, double tol) {
    const bool ok = (err <= tol) && (err == err);
    printf("  %-86s err %.3e  (tol %.1e)  %s\n", what, err, tol, ok ? "ok" : "FAIL");
    ++g_checks;
    if (!ok) ++g_fail;
}
// err / bound of a derived bound: passes at <= 1
static void report_ratio(const std::string& what, double ratio) {
    if (ratio == ratio && ratio > g_max_ratio) g_max_ratio = ratio;
    report((what + ": err / bound").c_str(), ratio, 1.0);
}
// a count of violations (bitwise comparisons, poison): passes at 0
static void report_count(const std::string& what, double n) { report(what.c_str(), n, 0.0); }
// running maximum that a NaN cannot slip through
static void upd(double& m, double r) { if (r != r) m = INFINITY; else if (r > m) m = r; }
static double ratio_of(ld err, ld bound) { return (bound > 0) ? (double)(err / bound) : (err == 0 ? 0.0 : INFINITY); }

static std::vector<void*> g_allocs;
template <typename T> static T* dalloc(size_t n) {
    T* p; CK(hipMalloc(&p, n * sizeof(T) + 64)); CK(hipMemset(p, 0xEE, n * sizeof(T) + 64)); g_allocs.push_back(p); return p;
}
template <typename T> static T* dupload(const std::vector<T>& v) {
    T* p = dalloc<T>(v.size()); CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); return p;
}
template <typename T> static std::vector<T> d2h(const T* p, size_t n) {
    std::vector<T> v(n); CK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return v;
}
template <typename T> static void poison(T* p, size_t n) { CK(hipMemset(p, 0xEE, n * sizeof(T))); }
static void free_all() { for (void* p : g_allocs) CK(hipFree(p)); g_allocs.clear(); }
static void dsync() { CK(hipDeviceSynchronize()); CK(hipGetLastError()); }
// bytes of [p, p + bytes) that are no longer 0xEE
static size_t touched(const void* p, size_t bytes) {
    const unsigned char* q = static_cast<const unsigned char*>(p);
    size_t n = 0; for (size_t i = 0; i < bytes; ++i) n += (q[i] != 0xEE); return n;
}
template <typename T> static size_t bit_diffs(const std::vector<T>& a, const std::vector<T>& b) {
    size_t n = 0; for (size_t i = 0; i < a.size(); ++i) n += (memcmp(&a[i], &b[i], sizeof(T)) != 0); return n;
}

struct Rng {
    std::mt19937_64 g; std::normal_distribution<double> n{0.0, 1.0};
    explicit Rng(uint64_t seed) : g(seed) {}
    double gauss() { double v = n(g); if (std::fabs(v) < 1e-3) v = (v < 0) ? -1e-3 : 1e-3; return v; }      // magnitude ~1, never zero
    double uni(double a, double b) { return a + (b - a) * (double)(g() >> 11) * 0x1p-53; }
};

// P = A B and S = |A| |B| in long double (row-major d x d operands of type T)
template <typename T> static void host_prod(const T* A, const T* B, int d, std::vector<ld>& P, std::vector<ld>& S) {
    static std::vector<ld> bt;
    bt.resize((size_t)d * d); P.resize((size_t)d * d); S.resize((size_t)d * d);
    for (int k = 0; k < d; ++k) for (int j = 0; j < d; ++j) bt[(size_t)j * d + k] = (ld)B[(size_t)k * d + j];
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            const T* a = A + (size_t)i * d; const ld* b = &bt[(size_t)j * d];
            ld p = 0, s = 0;
            for (int k = 0; k < d; ++k) { const ld q = (ld)a[k] * b[k]; p += q; s += fabsl(q); }
            P[(size_t)i * d + j] = p; S[(size_t)i * d + j] = s;
        }
}

// Sum of squares of N terms, each known as e^ with |e - e^| <= b on the device:
//   |e^2 - e^^2| <= (2 |e^| + b) b, the square itself rounds by u (|e^| + b)^2, the N-term sum (any order) by N u sum (|e^| + b)^2
//   bound = sum_terms [ (2 |e^| + b) b + u (|e^| + b)^2 ] + (N + 8) u sum_terms (|e^| + b)^2          (u = 2^-53: these sums are double)
struct SqAcc {
    ld e = 0, tb = 0, mag = 0; int n = 0;
    void add(ld eh, ld b) { const ld m = fabsl(eh) + b; e += eh * eh; tb += (2 * fabsl(eh) + b) * b + U64 * m * m; mag += m * m; ++n; }
    ld bound() const { return tb + (ld)(n + 8) * U64 * mag; }
};
// Plain sum of N terms, each known as t^ with |t - t^| <= b:   bound = sum_terms b + (N + 8) u sum_terms (|t^| + b)
struct LinAcc {
    ld e = 0, tb = 0, mag = 0; int n = 0;
    void add(ld th, ld b) { e += th; tb += b; mag += fabsl(th) + b; ++n; }
    ld bound() const { return tb + (ld)(n + 8) * U64 * mag; }
};

// ================================================================================================ gemm_f64_launch
enum Variant { V64, V32W4, V32W8 };       // the tile the case is MEANT to reach; full / edge follows from d % 64
struct TSpec { bool shareA = false, shareB = false; double alpha = 1.0, beta = 0.0, gamma = 0.0; bool partials = false, mu = false; };
struct Case {
    std::string name; int d = 64; Variant v = V64; int ntypes = 1; int64_t batch = 1; TSpec t[2];
    int pad = 0;            // doubles between the C of consecutive problems (they keep the poison)
    int pstride = 0;        // partial_stride argument (0 = the slots)
    bool skip = false, sym = false, upper = false, check = false, spread = false, twice = false;
    uint64_t seed = 1;
};
static bool skipped(const Case& c, int64_t b) { return c.skip && (((uint64_t)b * 2654435761ull) >> 16) % 3 == 1; }     // (no period: chunk starts do not align with it)

static void run_case(const Case& c) {
    const int d = c.d, bt = (c.v == V64) ? 64 : 32, nt = c.ntypes;
    const int64_t dd = (int64_t)d * d, NB = c.batch;
    const int64_t so = dd + 2;          // every operand matrix is followed by two NaNs: a read past its last row poisons the product
    const int t = (int)cdiv(d, bt), slots = t * t, pstr = c.pstride ? c.pstride : slots;
    const bool full = (d % 64) == 0;
    const int64_t t64 = cdiv(d, 64), work64 = (c.sym ? t64 * (t64 + 1) / 2 : t64 * t64) * nt * NB;
    g_num_cus = (c.v == V64) ? 1 : (c.v == V32W8 || !full) ? (1 << 30) : (int)work64 + 1;
    const char* vname = (bt == 64) ? (full ? "<64,2,full>" : "<64,2,edge>")
                        : !full ? "<32,3,ksplit,edge>" : (c.v == V32W8) ? "<32,1,ksplit,full,8 waves>" : "<32,1,ksplit,full,4 waves>";
    // the launch rule restated: which kernel this num_cus selects (a case that drifted to another one fails here)
    const int bt_rule = (work64 >= g_num_cus) ? 64 : 32;
    const int64_t m0 = std::min<int64_t>(NB, 65535 / (nt + (c.check ? 1 : 0)));
    const bool w8_rule = bt_rule == 32 && full && (int64_t)(d / 32) * (d / 32) * m0 * nt <= g_num_cus;
    const bool drift = bt_rule != bt || (bt == 32 && full && w8_rule != (c.v == V32W8));
    const std::string tag = c.name + " d=" + std::to_string(d) + " b=" + std::to_string((long long)NB) + " " + vname;

    // ---- operands
    Rng rng(c.seed * 7919 + d);
    std::vector<double> hA[2], hB[2];
    for (int i = 0; i < nt; ++i) {
        const int64_t nA = c.t[i].shareA ? 1 : NB, nB = c.t[i].shareB ? 1 : NB;
        hA[i].assign(nA * so, NAN); hB[i].assign(nB * so, NAN);
        if (c.sym) {
            // commuting symmetric factors with an exactly symmetric product: M symmetric with entries k / 2^18 (|k| <= 2^21), A = M M
            // (multiples of 2^-36 below 2^14: exact in double), B = M + 0.75 I.  A B needs ~80 bits, so the kernel does round.
            std::vector<ld> M(dd);
            for (int64_t p = 0; p < nA; ++p) {
                for (int r = 0; r < d; ++r) for (int q = r; q < d; ++q) {
                    double k = std::nearbyint(rng.gauss() * 0x1p18); if (k == 0) k = 1; k = std::fmax(-0x1p21, std::fmin(0x1p21, k));
                    M[(size_t)r * d + q] = M[(size_t)q * d + r] = (ld)k * 0x1p-18L;
                }
                for (int r = 0; r < d; ++r) for (int q = 0; q < d; ++q) {
                    ld s = 0; for (int k = 0; k < d; ++k) s += M[(size_t)r * d + k] * M[(size_t)k * d + q];
                    hA[i][p * so + (size_t)r * d + q] = (double)s;
                    hB[i][p * so + (size_t)r * d + q] = (double)(M[(size_t)r * d + q] + (r == q ? 0.75L : 0.0L));
                }
            }
        } else {
            for (int64_t p = 0; p < nA; ++p) for (int64_t e = 0; e < dd; ++e) hA[i][p * so + e] = rng.gauss();
            for (int64_t p = 0; p < nB; ++p) for (int64_t e = 0; e < dd; ++e) hB[i][p * so + e] = rng.gauss();
            if (c.spread) {      // rows of A and columns of B over ~1e-3 .. 1e3: a swapped row / column index cannot hide
                for (int64_t p = 0; p < nA; ++p) for (int r = 0; r < d; ++r) { const double s = std::pow(10.0, rng.uni(-3, 3)); for (int q = 0; q < d; ++q) hA[i][p * so + (size_t)r * d + q] *= s; }
                for (int64_t p = 0; p < nB; ++p) for (int q = 0; q < d; ++q) { const double s = std::pow(10.0, rng.uni(-3, 3)); for (int r = 0; r < d; ++r) hB[i][p * so + (size_t)r * d + q] *= s; }
            }
            if (c.upper) for (int64_t p = 0; p < nB; ++p) for (int r = 0; r < d; ++r) for (int q = 0; q < r; ++q) hB[i][p * so + (size_t)r * d + q] = 0.0;
        }
    }
    const int64_t sc = dd + c.pad;
    const int mu_stride = 3, skip_stride = kStateInts;
    std::vector<double> hmu(NB * mu_stride, NAN);
    for (int64_t b = 0; b < NB; ++b) hmu[b * mu_stride] = 0.7 + 0.013 * (double)(b % 41);
    std::vector<int> hskip(NB * skip_stride, 0);
    for (int64_t b = 0; b < NB; ++b) hskip[b * skip_stride] = skipped(c, b) ? 1 : 0;
    double *dA[2] = {}, *dB[2] = {}, *dC[2] = {}, *dP[2] = {};
    GemmType ty[2];
    double* dmu = dupload(hmu);
    for (int i = 0; i < nt; ++i) {
        dA[i] = dupload(hA[i]); dB[i] = dupload(hB[i]); dC[i] = dalloc<double>(NB * sc);
        if (c.t[i].partials) dP[i] = dalloc<double>(NB * pstr);
        ty[i] = GemmType{dA[i], c.t[i].shareA ? 0 : so, dB[i], c.t[i].shareB ? 0 : so, dC[i], sc, c.t[i].alpha, c.t[i].beta, c.t[i].gamma, dP[i]};
        ty[i].b_upper = c.upper ? 1 : 0; ty[i].sym = c.sym ? 1 : 0;
        if (c.t[i].mu) { ty[i].mu = dmu; ty[i].mu_stride = mu_stride; }
    }
    int* dskip = c.skip ? dupload(hskip) : nullptr;
    // ---- the check that rides on the launch: fresh states, residual partials and Y of its own (Y = the A operand of type 0)
    const int cn = 3, cps = 4, ck_k = 1;
    std::vector<NsState> hst;
    std::vector<double> hcp;
    NsState* dst = nullptr;
    NsCheckArgs ck; memset(&ck, 0, sizeof(ck));
    if (c.check) {
        hst.resize(NB); memset(hst.data(), 0, NB * sizeof(NsState));
        hcp.assign(NB * cps, NAN);
        for (int64_t b = 0; b < NB; ++b) {
            hst[b].res_min = INFINITY; hst[b].mu[ck_k] = 0.9 + 0.002 * (double)(b % 97);
            for (int s = 0; s < cn; ++s) hcp[b * cps + s] = rng.uni(0.1, 2.0);
        }
        dst = dupload(hst);
        ck.k = ck_k; ck.max_iter = 50; ck.st_all = dst; ck.partials_all = dupload(hcp); ck.nslots = cn; ck.pstride = cps;
        ck.Yall = dA[0]; ck.stride = c.t[0].shareA ? 0 : so; ck.d = d; ck.tol_res = 0.0; ck.tol_tr = 0.0;
    }

    // ---- launch (twice for the determinism cases; without and then with the check for the check cases)
    const int runs = (c.twice || c.check) ? 2 : 1;
    std::vector<double> C[2], P[2], C0[2], P0[2];
    int ret = 0;
    for (int r = 0; r < runs; ++r) {
        for (int i = 0; i < nt; ++i) { poison(dC[i], NB * sc); if (dP[i]) poison(dP[i], NB * pstr); C0[i].swap(C[i]); P0[i].swap(P[i]); }
        ret = gemm_f64_launch(d, ty, nt, NB, dskip, skip_stride, 0, 0, c.pstride, (c.check && r == runs - 1) ? &ck : nullptr);
        dsync();
        for (int i = 0; i < nt; ++i) { C[i] = d2h(dC[i], NB * sc); if (dP[i]) P[i] = d2h(dP[i], NB * pstr); }
    }
    report_count(tag + ": slots returned = cdiv(d, BT)^2, kernel as meant", std::fabs((double)(ret - slots)) + (drift ? 1.0 : 0.0));
    if (ret != slots) { printf("    returned %d, expected %d (%s)\n", ret, slots, err_buf()); free_all(); return; }
    if (runs == 2) {
        size_t nd = 0;
        for (int i = 0; i < nt; ++i) { nd += bit_diffs(C[i], C0[i]); if (dP[i]) nd += bit_diffs(P[i], P0[i]); }
        report_count(tag + (c.check ? ": C, partials bitwise equal with and without the check" : ": second launch bitwise equal (C, partials)"), (double)nd);
    }

    // ---- compare, problem by problem
    double rC = 0, rSlot = 0, rSum = 0; size_t nPoison = 0, nMirrorSlot = 0, nAsym = 0;
    std::vector<ld> Pr, S;
    std::vector<SqAcc> tile(slots);
    for (int i = 0; i < nt; ++i)
        for (int64_t b = 0; b < NB; ++b) {
            const double* Cb = &C[i][b * sc];
            nPoison += touched(Cb + dd, c.pad * sizeof(double));
            if (dP[i]) nPoison += touched(P[i].data() + b * pstr + slots, (pstr - slots) * sizeof(double));
            if (skipped(c, b)) {         // a finished problem: nothing of it may be written
                nPoison += touched(Cb, dd * sizeof(double));
                if (dP[i]) nPoison += touched(P[i].data() + b * pstr, slots * sizeof(double));
                continue;
            }
            host_prod(&hA[i][c.t[i].shareA ? 0 : b * so], &hB[i][c.t[i].shareB ? 0 : b * so], d, Pr, S);
            double alpha = c.t[i].alpha, beta = c.t[i].beta, gamma = c.t[i].gamma;
            if (c.t[i].mu) { const double m = hmu[b * mu_stride]; alpha = -0.5 * m * m * m; beta = 1.5 * m; gamma = beta + alpha; }
            for (auto& a : tile) a = SqAcc();
            for (int r = 0; r < d; ++r)
                for (int q = 0; q < d; ++q) {
                    const size_t e = (size_t)r * d + q;
                    const ld want = (ld)alpha * Pr[e] + (r == q ? (ld)beta : 0.0L);
                    const ld bound = (ld)(d + 2) * U64 * (fabsl((ld)alpha) * S[e] + (r == q ? fabsl((ld)beta) : 0.0L));
                    upd(rC, ratio_of(fabsl((ld)Cb[e] - want), bound));
                    // residual term e = C_ij - gamma delta_ij: known to the C bound plus the rounding of the subtraction
                    const ld eh = want - (r == q ? (ld)gamma : 0.0L);
                    tile[(r / bt) * t + q / bt].add(eh, bound + U64 * (fabsl(eh) + bound));
                }
            const bool mirrored = c.sym && bt == 64;
            if (mirrored)       // off-diagonal tiles are stored twice: bit for bit symmetric there
                for (int r = 0; r < d; ++r) for (int q = 0; q < d; ++q)
                    if (r / 64 < q / 64) nAsym += (memcmp(&Cb[(size_t)r * d + q], &Cb[(size_t)q * d + r], 8) != 0);
            if (dP[i]) {
                // slot ty * t + tx holds its own tile's share of ||C - gamma I||_F^2 (SqAcc bound); with mirrored tiles the upper one
                // carries twice its share and the lower one reads 0.0; the sum over the slots is the full residual
                ld sumGot = 0, sumWant = 0, sumBound = 0;
                for (int y = 0; y < t; ++y) for (int x = 0; x < t; ++x) {
                    const double got = P[i][b * pstr + y * t + x];
                    const SqAcc& a = tile[y * t + x];
                    sumGot += got; sumWant += a.e; sumBound += a.bound();
                    if (mirrored && x < y) { nMirrorSlot += (got != 0.0 || std::signbit(got)); continue; }
                    const ld f = (mirrored && x > y) ? 2.0L : 1.0L;
                    upd(rSlot, ratio_of(fabsl((ld)got - f * a.e), f * a.bound()));
                }
                upd(rSum, ratio_of(fabsl(sumGot - sumWant), sumBound));
            }
        }
    report_ratio(tag + ": C", rC);
    if (c.pad || c.skip || c.pstride) report_count(tag + ": padding, spare slots, skipped problems keep the poison (bytes)", (double)nPoison);
    if (dP[0] || dP[1]) { report_ratio(tag + ": residual partial of every slot", rSlot); report_ratio(tag + ": sum of the partials = ||C - gamma I||_F^2", rSum); }
    if (c.sym && bt == 64) {
        report_count(tag + ": C_ij == C_ji bitwise across off-diagonal tiles", (double)nAsym);
        if (dP[0]) report_count(tag + ": residual slots of mirror tiles read 0.0", (double)nMirrorSlot);
    }
    if (c.check) {
        // res[k] = 2 sqrt(sum of nslots partials) / mu_k^3: the sum is off by <= (nslots + 8) u relative, sqrt, the cube and the
        // division by a few u more: (nslots + 16) u relative.  tr[k] = sum_i Y_ii: LinAcc with exact terms.
        auto st = d2h(dst, NB);
        double rRes = 0, rTr = 0;
        for (int64_t b = 0; b < NB; ++b) {
            ld s = 0; for (int q = 0; q < cn; ++q) s += hcp[b * cps + q];
            const ld m = hst[b].mu[ck_k], want = 2.0L * sqrtl(s) / (m * m * m);
            upd(rRes, ratio_of(fabsl((ld)st[b].res[ck_k] - want), (ld)(cn + 16) * U64 * want));
            LinAcc tr; const double* Y = &hA[0][c.t[0].shareA ? 0 : b * so];
            for (int r = 0; r < d; ++r) tr.add(Y[(size_t)r * d + r], 0);
            upd(rTr, ratio_of(fabsl((ld)st[b].tr[ck_k] - tr.e), tr.bound()));
        }
        report_ratio(tag + ": st.res[k] = 2 sqrt(sum partials) / mu_k^3", rRes);
        report_ratio(tag + ": st.tr[k] = tr Y", rTr);
    }
    free_all();
}

static Case mk(const char* name, int d, Variant v, int64_t batch = 1) { Case c; c.name = name; c.d = d; c.v = v; c.batch = batch; return c; }
static void t_product(TSpec& t) { t.alpha = -0.5; t.beta = 1.5; t.gamma = 1.0; t.partials = true; }

static void section_f64() {
    printf("section f64: gemm_f64_launch\n");
    // all five instantiations, plain product (odd d: scalar loads)
    for (int d : {64, 128, 192, 256}) for (Variant v : {V64, V32W4}) { Case c = mk("plain", d, v); c.spread = (d == 192); run_case(c); }
    for (int d : {1, 2, 17, 31, 33, 63, 65, 130, 200, 255}) for (Variant v : {V64, V32W4}) { Case c = mk("plain", d, v); c.spread = (d == 130 || d == 255); run_case(c); }
    for (int d : {64, 128, 256, 512}) run_case(mk("plain", d, V32W8));
    // alpha, beta I, gamma and the residual partials of every slot (XCD remap active at t % 4 == 0: d = 256 / 64, 128 / 32, 512 / 32)
    { const int ds[] = {256, 192, 130, 128, 192, 200, 512}; const Variant vs[] = {V64, V64, V64, V32W4, V32W8, V32W4, V32W8};
      for (int i = 0; i < 7; ++i) { Case c = mk("T product", ds[i], vs[i]); t_product(c.t[0]); c.pstride = (i & 1) ? 0 : (int)(cdiv(ds[i], 32) * cdiv(ds[i], 32)) + 3; run_case(c); } }
    // device-side step scale
    for (Variant v : {V64, V32W4}) for (int d : {128, 65}) { Case c = mk("mu", d, v, 3); t_product(c.t[0]); c.t[0].mu = true; run_case(c); }
    // batch and strides: shared and per-problem operands, padding between the C of consecutive problems
    for (int64_t nb : {1, 3, 9}) for (int sh = 0; sh < 3; ++sh) {
        Case a = mk("strides", 96, V64, nb), b = mk("strides", 64, V32W4, nb);
        for (Case* c : {&a, &b}) { c->t[0].shareA = (sh == 1); c->t[0].shareB = (sh == 2); c->pad = 7; c->t[0].alpha = 1.25; run_case(*c); }
    }
    // two GEMM types in one launch
    { const int ds[] = {128, 128, 100, 64}; const Variant vs[] = {V64, V32W4, V32W4, V32W8}; const int64_t bs[] = {3, 3, 2, 1};
      for (int i = 0; i < 4; ++i) {
          Case c = mk(i == 0 ? "two types, partials on type 0" : "two types, partials on both", ds[i], vs[i], bs[i]); c.ntypes = 2;
          t_product(c.t[0]); c.t[1].alpha = 0.75; c.t[1].beta = -2.0; c.t[1].gamma = 0.25; c.t[1].partials = (i != 0); c.t[1].shareB = (i == 2); c.pad = (i == 1) ? 4 : 0;
          run_case(c);
      } }
    // finished problems
    { Case c = mk("skip", 128, V64, 9); t_product(c.t[0]); c.skip = true; run_case(c); }
    { Case c = mk("skip", 70, V32W4, 9); c.ntypes = 2; t_product(c.t[0]); t_product(c.t[1]); c.t[1].alpha = 2.0; c.skip = true; c.pad = 2; run_case(c); }
    { Case c = mk("skip", 64, V32W8, 4); t_product(c.t[0]); c.skip = true; run_case(c); }
    // symmetric product hint: honoured at BT 64 (d / 64 = 4: XCD map rotated by problem index), ignored at BT 32
    for (int d : {128, 192, 256, 130}) { Case c = mk("sym", d, V64, 9); c.sym = true; t_product(c.t[0]); run_case(c); }
    { Case c = mk("sym, two types", 256, V64, 3); c.sym = true; c.ntypes = 2; t_product(c.t[0]); c.t[1].alpha = 1.0; run_case(c); }
    for (int d : {128, 130}) { Case c = mk("sym (ignored)", d, V32W4, 9); c.sym = true; t_product(c.t[0]); run_case(c); }
    // B upper triangular: shared by all problems (as its one caller does) and once per problem
    for (int d : {64, 96, 130, 200, 256}) for (int bt = 0; bt < 2; ++bt) for (int m = 0; m < 3; ++m) {
        Case c = mk(m == 2 ? "b_upper, B per problem" : "b_upper, B shared", d, bt ? V64 : (m == 0 ? V32W8 : V32W4), m == 0 ? 1 : 5);
        c.upper = true; c.t[0].shareB = (m != 2); c.t[0].partials = (m == 1); run_case(c);
    }
    for (Variant v : {V64, V32W8}) { Case c = mk("b_upper, B shared", 768, v); c.upper = true; c.t[0].shareB = true; run_case(c); }
    // the check riding on the launch
    { Case c = mk("check", 128, V64, 3); c.ntypes = 2; c.t[1].alpha = -1.0; c.check = true; run_case(c); }
    { Case c = mk("check", 64, V32W8, 1); c.check = true; run_case(c); }
    { Case c = mk("check", 33, V32W4, 3); c.check = true; t_product(c.t[0]); run_case(c); }
    // determinism, one case per instantiation
    { const int ds[] = {256, 200, 256, 256, 200}; const Variant vs[] = {V64, V64, V32W8, V32W4, V32W4};
      for (int i = 0; i < 5; ++i) { Case c = mk("determinism", ds[i], vs[i], 2); t_product(c.t[0]); c.twice = true; run_case(c); } }
    // argument errors: nothing is launched
    { GemmType ty[3]; memset(ty, 0, sizeof(ty));
      report_count("ntypes = 3 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f64_launch(64, ty, 3, 1, nullptr, 0, 0, 0) - FAD_ERR_INVALID)));
      report_count("batch = 0 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f64_launch(64, ty, 1, 0, nullptr, 0, 0, 0) - FAD_ERR_INVALID)));
      dsync(); }
}

static void section_f64big() {
    printf("section f64big: more problems than grid layers (d = 16)\n");
    // 70 000 problems of one type: two chunks of 65 535; shared B, mu, skip, partials with a spare slot: every `done` offset
    { Case c = mk("chunks", 16, V64, 70000); t_product(c.t[0]); c.t[0].mu = true; c.t[0].shareB = true; c.skip = true; c.pstride = 2; c.pad = 3; run_case(c); }
    // 40 000 problems of two types: 32 767 per chunk
    { Case c = mk("chunks, two types", 16, V32W4, 40000); c.ntypes = 2; t_product(c.t[0]); t_product(c.t[1]); c.t[1].alpha = 0.5; c.t[0].shareB = true; c.t[1].shareA = true; c.skip = true; run_case(c); }
    // 40 000 problems of one type with the check riding: 32 767 per chunk, the checker's state / partials / Y offsets are crossed
    { Case c = mk("chunks, check", 16, V64, 40000); t_product(c.t[0]); c.check = true; run_case(c); }
}

// ================================================================================================ statistics epilogues
// rowabs[bj][row] = sum over the columns of block bj of |M[row][col]|, colabs[bi][col] = sum over the rows of block bi (32-wide blocks)
static void abs_sums_check(const std::vector<double>& stats, int d, const std::vector<ld>& M, const std::vector<ld>& Mb, double& rRow, double& rCol) {
    const int nb = d / 32;
    for (int blk = 0; blk < nb; ++blk)
        for (int i = 0; i < d; ++i) {
            LinAcc row, col;
            for (int q = 0; q < 32; ++q) {
                const size_t er = (size_t)i * d + blk * 32 + q, ec = (size_t)(blk * 32 + q) * d + i;
                row.add(fabsl(M[er]), Mb[er]); col.add(fabsl(M[ec]), Mb[ec]);
            }
            upd(rRow, ratio_of(fabsl((ld)stats[(size_t)blk * d + i] - row.e), row.bound()));
            upd(rCol, ratio_of(fabsl((ld)stats[(size_t)(nb + blk) * d + i] - col.e), col.bound()));
        }
}
static double h_round_f16(double v) { return (double)(float)(_Float16)(float)v; }
static double h_round_bf16(double v) {
    float f = (float)v; uint32_t u; memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u); u &= 0xffff0000u; memcpy(&f, &u, 4);
    return (double)f;
}
// numpy's rule for ||mu1 - mu2||^2 restated (ns_mean.h): exact = the value is an ordered sum and must match bit for bit; otherwise
// a float64 sum of d squares of once-rounded differences: (d + 8) u sum (2 u per term + the d-term sum, any order)
static double host_mean_term(const std::vector<double>& m1, const std::vector<double>& m2, int dt, bool& exact, ld& bound) {
    const int d = (int)m1.size();
    exact = false; bound = 0;
    if (dt == FAD_F16 || dt == FAD_BF16) {
        auto rnd = (dt == FAD_F16) ? h_round_f16 : h_round_bf16;
        float acc = 0.f;
        for (int i = 0; i < d; ++i) { const float g = (float)rnd(rnd(m1[i]) - rnd(m2[i])); acc = fmaf(g, g, acc); }
        exact = true; return rnd((double)acc);
    }
    if (dt == FAD_F32) {
        double acc = 0.0;
        for (int i = 0; i < d; ++i) { const double g = (double)(float)((double)(float)m1[i] - (double)(float)m2[i]); acc += g * g; }   // g * g is exact in double
        exact = true; return (double)(float)acc;
    }
    ld s = 0;
    for (int i = 0; i < d; ++i) {
        double b = m2[i];
        if (dt >= 16) { const int q = dt & 3; b = (q == FAD_F16) ? h_round_f16(b) : (q == FAD_BF16) ? h_round_bf16(b) : (q == FAD_F32) ? (double)(float)b : b; }
        const ld df = (ld)m1[i] - (ld)b; s += df * df;
    }
    bound = (ld)(d + 8) * U64 * s;
    return (double)s;
}

static void stats_product_case(int d, const std::vector<int>& dtypes) {
    const size_t dd = (size_t)d * d; const int nb = d / 32;
    Rng rng(4242 + d);
    std::vector<double> C1(dd), C2(dd), m1(d), m2(d);
    for (auto& v : C1) v = rng.gauss();
    for (auto& v : C2) v = rng.gauss();              // NOT symmetric: a row / column or tx / ty swap cannot cancel
    for (int r = 0; r < d; ++r) { const double s = std::pow(10.0, rng.uni(-1.5, 1.5)); for (int q = 0; q < d; ++q) C1[(size_t)r * d + q] *= s; }
    for (auto& v : m1) v = rng.gauss();
    for (auto& v : m2) v = rng.gauss();
    std::vector<ld> Pr, S, Pb(dd);
    host_prod(C1.data(), C2.data(), d, Pr, S);
    for (size_t e = 0; e < dd; ++e) Pb[e] = (ld)(d + 2) * U64 * S[e];
    double *dC1 = dupload(C1), *dC2 = dupload(C2), *dm1 = dupload(m1), *dm2 = dupload(m2), *dA = dalloc<double>(dd);
    const size_t ns = 2 * (size_t)nb * d + 8 * (size_t)nb * nb;
    double* dstats = dalloc<double>(ns);
    NsState* dst = dalloc<NsState>(1);
    for (int dt : dtypes) {
        const std::string tag = "product + stats d=" + std::to_string(d) + " mean_dtype=" + std::to_string(dt);
        poison(dA, dd); poison(dstats, ns); poison(dst, 1);
        NsProductExt ext; memset(&ext, 0, sizeof(ext));
        ext.stats = dstats; ext.mu1 = dm1; ext.mu2 = dm2; ext.mean_dtype = dt; ext.st = dst;
        const int ret = gemm_f64_product_stats_launch(d, dC1, dC2, dA, nullptr, ext, 0);
        dsync();
        report_count(tag + ": launched", std::fabs((double)ret));
        auto A = d2h(dA, dd); auto st = d2h(dstats, ns); auto state = d2h(dst, 1);
        double rA = 0, rRow = 0, rCol = 0, rSq = 0, rTr = 0; size_t bad = 0;
        for (size_t e = 0; e < dd; ++e) upd(rA, ratio_of(fabsl((ld)A[e] - Pr[e]), Pb[e]));
        abs_sums_check(st, d, Pr, Pb, rRow, rCol);
        for (int y = 0; y < nb; ++y) for (int x = 0; x < nb; ++x) {
            // record of tile (y, x): sum v^2 (twice: SqAcc), shares of tr A (LinAcc with the C bound), tr C1, tr C2 (LinAcc, exact terms)
            const double* rec = &st[2 * (size_t)nb * d + 8 * (size_t)(y * nb + x)];
            SqAcc sq; LinAcc ta, t1, t2;
            for (int r = 0; r < 32; ++r) for (int q = 0; q < 32; ++q) {
                const size_t e = (size_t)(y * 32 + r) * d + x * 32 + q;
                sq.add(Pr[e], Pb[e]);
                if (y * 32 + r == x * 32 + q) { ta.add(Pr[e], Pb[e]); t1.add(C1[e], 0); t2.add(C2[e], 0); }
            }
            upd(rSq, ratio_of(fabsl((ld)rec[0] - sq.e), sq.bound())); upd(rSq, ratio_of(fabsl((ld)rec[1] - sq.e), sq.bound()));
            if (y == x) { upd(rTr, ratio_of(fabsl((ld)rec[2] - ta.e), ta.bound())); upd(rTr, ratio_of(fabsl((ld)rec[3] - t1.e), t1.bound())); upd(rTr, ratio_of(fabsl((ld)rec[4] - t2.e), t2.bound())); }
            else bad += (rec[2] != 0.0) + (rec[3] != 0.0) + (rec[4] != 0.0);
            bad += touched(rec + 5, 3 * sizeof(double));
        }
        report_ratio(tag + ": A = C1 C2", rA);
        report_ratio(tag + ": rowabs[bj][row]", rRow);
        report_ratio(tag + ": colabs[bi][col]", rCol);
        report_ratio(tag + ": sum v^2 per tile", rSq);
        report_ratio(tag + ": trace shares of A, C1, C2 (diagonal tiles)", rTr);
        report_count(tag + ": trace shares of off-diagonal tiles are 0.0, spare words keep the poison", (double)bad);
        bool exact; ld bound;
        const double want = host_mean_term(m1, m2, dt, exact, bound);
        if (exact) report_count(tag + ": mean term bit for bit", memcmp(&want, &state[0].mean_term, 8) != 0 ? 1.0 : 0.0);
        else report_ratio(tag + ": mean term", ratio_of(fabsl((ld)state[0].mean_term - (ld)want), bound));
        NsState p; memset(&p, 0xEE, sizeof(p)); p.mean_term = state[0].mean_term;
        report_count(tag + ": the rest of the state keeps the poison", memcmp(&p, &state[0], sizeof(p)) != 0 ? 1.0 : 0.0);
    }
    {   // a finished problem: A and the statistics stay untouched
        poison(dA, dd); poison(dstats, ns);
        int* dskip = dupload(std::vector<int>(1, 1));
        NsProductExt ext; memset(&ext, 0, sizeof(ext));
        ext.stats = dstats; ext.mu1 = dm1; ext.mu2 = dm2; ext.mean_dtype = FAD_F64; ext.st = dst;
        gemm_f64_product_stats_launch(d, dC1, dC2, dA, dskip, ext, 0); dsync();
        auto A = d2h(dA, dd); auto st = d2h(dstats, ns);
        report_count("product + stats d=" + std::to_string(d) + ": skip set -> A and stats keep the poison (bytes)", (double)(touched(A.data(), dd * 8) + touched(st.data(), ns * 8)));
    }
    free_all();
}

static void stats_correction_case(int d) {
    const size_t dd = (size_t)d * d; const int nb = d / 32;
    Rng rng(777 + d);
    // the ping-pong pair holds DIFFERENT matrices, so the wrong choice fails; Z is not symmetric
    std::vector<float> Y[2], Z[2];
    for (int s = 0; s < 2; ++s) { Y[s].resize(dd); Z[s].resize(dd); for (auto& v : Y[s]) v = (float)rng.gauss(); for (auto& v : Z[s]) v = (float)rng.gauss();
        for (int r = 0; r < d; ++r) { const float sc = (float)std::pow(10.0, rng.uni(-1.5, 1.5)); for (int q = 0; q < d; ++q) Z[s][(size_t)r * d + q] *= sc; } }
    std::vector<double> A64(dd); for (auto& v : A64) v = rng.gauss() * std::sqrt((double)d);
    const double cval = 1.7;
    float *dY[2] = {dupload(Y[0]), dupload(Y[1])}, *dZ[2] = {dupload(Z[0]), dupload(Z[1])};
    double* dA64 = dupload(A64);
    const size_t ns = 2 * (size_t)nb * d + 8 * (size_t)nb * nb;
    double* dstats = dalloc<double>(ns);
    NsState hs; memset(&hs, 0, sizeof(hs)); hs.c = cval;
    NsState* dst = dupload(std::vector<NsState>(1, hs));
    for (int selv : {2, 3, -1}) {           // even, odd, no selector (-> the first pair)
        const int s = (selv == 3) ? 1 : 0;
        const std::string tag = "correction d=" + std::to_string(d) + (selv < 0 ? " sel=none" : " *sel=" + std::to_string(selv));
        poison(dstats, ns);
        int* dsel = (selv < 0) ? nullptr : dupload(std::vector<int>(1, selv));
        NsProductExt ext; memset(&ext, 0, sizeof(ext));
        ext.stats = dstats; ext.st = dst; ext.A64 = dA64; ext.Z32 = dZ[0]; ext.Z32_alt = dZ[1];
        const int ret = gemm_f64_correction_launch(d, dY[0], dY[1], dsel, nullptr, ext, 0);
        dsync();
        report_count(tag + ": launched", std::fabs((double)ret));
        auto st = d2h(dstats, ns);
        std::vector<ld> G, S, Zl(dd), Zb(dd, 0.0L);
        host_prod(Y[s].data(), Y[s].data(), d, G, S);
        for (size_t e = 0; e < dd; ++e) Zl[e] = (ld)Z[s][e];
        double rRow = 0, rCol = 0, rZR = 0, rRR = 0, rTr = 0; size_t bad = 0;
        abs_sums_check(st, d, Zl, Zb, rRow, rCol);          // row / column sums of |Z| (exact terms), through the transposed mirror tile
        LinAcc totZR; SqAcc totRR; LinAcc totTr; ld gotZR = 0, gotRR = 0, gotTr = 0;
        for (int y = 0; y < nb; ++y) for (int x = 0; x < nb; ++x) {
            const double* rec = &st[2 * (size_t)nb * d + 8 * (size_t)(y * nb + x)];
            LinAcc zr, tr; SqAcc rr;
            for (int r = 0; r < 32; ++r) for (int q = 0; q < 32; ++q) {
                const int i = y * 32 + r, j = x * 32 + q; const size_t e = (size_t)i * d + j;
                // R_ij = A64_ij * (1 / c) - G_ij: G to the product bound, the quotient to 4 u (division, product), the difference to u
                const ld ac = (ld)A64[e] / (ld)cval, Rh = ac - G[e];
                const ld bR = (ld)(d + 2) * U64 * S[e] + 4 * U64 * fabsl(ac) + U64 * fabsl(Rh);
                const ld z = Zl[(size_t)j * d + i];
                zr.add(z * Rh, fabsl(z) * bR + U64 * fabsl(z) * (fabsl(Rh) + bR)); totZR.add(z * Rh, fabsl(z) * bR + U64 * fabsl(z) * (fabsl(Rh) + bR));
                rr.add(Rh, bR); totRR.add(Rh, bR);
                if (i == j) { tr.add((ld)Y[s][e], 0); totTr.add((ld)Y[s][e], 0); }
            }
            upd(rZR, ratio_of(fabsl((ld)rec[0] - zr.e), zr.bound()));
            upd(rRR, ratio_of(fabsl((ld)rec[1] - rr.e), rr.bound()));
            if (y == x) upd(rTr, ratio_of(fabsl((ld)rec[2] - tr.e), tr.bound())); else bad += (rec[2] != 0.0);
            bad += touched(rec + 3, 5 * sizeof(double));
            gotZR += rec[0]; gotRR += rec[1]; gotTr += rec[2];
        }
        report_ratio(tag + ": rowabs of Z", rRow);
        report_ratio(tag + ": colabs of Z", rCol);
        report_ratio(tag + ": tile shares of tr(Z R)", rZR);
        report_ratio(tag + ": tile shares of ||R||_F^2", rRR);
        report_ratio(tag + ": tile shares of tr Y", rTr);
        report_ratio(tag + ": sum of tiles = tr(Z R)", ratio_of(fabsl(gotZR - totZR.e), totZR.bound()));
        report_ratio(tag + ": sum of tiles = ||R||_F^2", ratio_of(fabsl(gotRR - totRR.e), totRR.bound()));
        report_ratio(tag + ": sum of tiles = tr Y", ratio_of(fabsl(gotTr - totTr.e), totTr.bound()));
        report_count(tag + ": tr Y shares of off-diagonal tiles are 0.0, spare words keep the poison", (double)bad);
    }
    {
        poison(dstats, ns);
        int* dskip = dupload(std::vector<int>(1, 1));
        NsProductExt ext; memset(&ext, 0, sizeof(ext));
        ext.stats = dstats; ext.st = dst; ext.A64 = dA64; ext.Z32 = dZ[0]; ext.Z32_alt = dZ[1];
        gemm_f64_correction_launch(d, dY[0], dY[1], nullptr, dskip, ext, 0); dsync();
        auto st = d2h(dstats, ns);
        report_count("correction d=" + std::to_string(d) + ": skip set -> stats keep the poison (bytes)", (double)touched(st.data(), ns * 8));
    }
    free_all();
}

static void section_stats() {
    printf("section stats: gemm_f64_product_stats_launch (MODE 1), gemm_f64_correction_launch (MODE 2)\n");
    stats_product_case(64, {FAD_F64, FAD_F16, FAD_BF16, FAD_F32, FAD_MEAN_SECOND_ONLY | FAD_F16});
    stats_product_case(128, {FAD_F64, FAD_BF16});
    stats_product_case(512, {FAD_F16, FAD_F32});
    stats_product_case(1088, {FAD_F16, FAD_BF16});          // the 1024-wide window of the ordered sum wraps
    for (int d : {64, 128, 512}) stats_correction_case(d);
    NsProductExt ext; memset(&ext, 0, sizeof(ext));
    report_count("product + stats d=96 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f64_product_stats_launch(96, nullptr, nullptr, nullptr, nullptr, ext, 0) - FAD_ERR_INVALID)));
    report_count("correction d=32 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f64_correction_launch(32, nullptr, nullptr, nullptr, nullptr, ext, 0) - FAD_ERR_INVALID)));
    dsync();
}

// ================================================================================================ gemm_f32.hip
// The fp32 bound assumes v_mfma_f32_32x32x2_f32 rounds each multiply-add no worse than IEEE.
static void f32_compare(const std::string& tag, int d, const std::vector<float>& A, const std::vector<float>& B, float alpha, float beta, float gamma,
                        const std::vector<float>& C, const std::vector<double>* part) {
    const int t = d / 32;
    std::vector<ld> Pr, S; host_prod(A.data(), B.data(), d, Pr, S);
    std::vector<SqAcc> tile((size_t)t * t);
    double rC = 0, rSlot = 0;
    for (int r = 0; r < d; ++r) for (int q = 0; q < d; ++q) {
        const size_t e = (size_t)r * d + q;
        const ld want = (ld)alpha * Pr[e] + (r == q ? (ld)beta : 0.0L);
        const ld bound = (ld)(d + 2) * U32 * (fabsl((ld)alpha) * S[e] + (r == q ? fabsl((ld)beta) : 0.0L));
        upd(rC, ratio_of(fabsl((ld)C[e] - want), bound));
        const ld eh = want - (r == q ? (ld)gamma : 0.0L);
        tile[(r / 32) * t + q / 32].add(eh, bound + U64 * (fabsl(eh) + bound));       // (the residual is formed in double)
    }
    report_ratio(tag + ": C", rC);
    if (part) {
        for (int s = 0; s < t * t; ++s) upd(rSlot, ratio_of(fabsl((ld)(*part)[s] - tile[s].e), tile[s].bound()));
        report_ratio(tag + ": residual partial of every slot", rSlot);
    }
}

static void f32_case(int d, int ntypes, bool check, bool skip) {
    const size_t dd = (size_t)d * d; const int slots = (d / 32) * (d / 32);
    Rng rng(99 + d + 7 * ntypes);
    const float al[2] = {-0.5f, 0.75f}, be[2] = {1.5f, -0.25f}, ga[2] = {1.0f, 0.5f};
    std::vector<float> A[2], B[2];
    Gemm32Args g; memset(&g, 0, sizeof(g));
    float* dC[2] = {}; double* dP[2] = {};
    for (int i = 0; i < ntypes; ++i) {
        A[i].resize(dd); B[i].resize(dd);
        for (auto& v : A[i]) v = (float)rng.gauss();
        for (auto& v : B[i]) v = (float)rng.gauss();
        if (i == 1) for (int r = 0; r < d; ++r) { const float s = (float)std::pow(10.0, rng.uni(-2, 2)); for (int q = 0; q < d; ++q) A[i][(size_t)r * d + q] *= s; }
        g.A[i] = dupload(A[i]); g.B[i] = dupload(B[i]); g.C[i] = dC[i] = dalloc<float>(dd); g.partials[i] = dP[i] = dalloc<double>(slots + 1);
        g.alpha[i] = al[i]; g.beta_eye[i] = be[i]; g.gamma[i] = ga[i];
    }
    g.ntypes = ntypes;
    if (skip) g.skip = dupload(std::vector<int>(1, 1));
    const int k = 1, cn = 5;
    std::vector<double> hcp(cn + 1, NAN); for (int s = 0; s < cn; ++s) hcp[s] = rng.uni(0.1, 2.0);
    Ns32State s32; memset(&s32, 0, sizeof(s32)); NsState s64; memset(&s64, 0, sizeof(s64));
    Ns32State* dst = dupload(std::vector<Ns32State>(1, s32));
    g.k = k; g.max_low = 30; g.nslots = cn; g.thr_pred = 0.0; g.chk_partials = dupload(hcp); g.st = dst; g.st64 = dupload(std::vector<NsState>(1, s64));
    const std::string tag = std::string("gemm_f32 d=") + std::to_string(d) + " types=" + std::to_string(ntypes) + (check ? " +check" : "") + (skip ? " skip" : "");
    std::vector<float> C[2], C0[2]; std::vector<double> P[2], P0[2];
    const int runs = check ? 2 : 1;
    int ret = 0;
    for (int r = 0; r < runs; ++r) {
        for (int i = 0; i < ntypes; ++i) { poison(dC[i], dd); poison(dP[i], slots + 1); C0[i].swap(C[i]); P0[i].swap(P[i]); }
        g.check = (check && r == runs - 1) ? 1 : 0;
        ret = gemm_f32_launch(d, g, 0); dsync();
        for (int i = 0; i < ntypes; ++i) { C[i] = d2h(dC[i], dd); P[i] = d2h(dP[i], slots + 1); }
    }
    report_count(tag + ": slots returned = (d / 32)^2", std::fabs((double)(ret - slots)));
    if (skip) {
        size_t n = 0; for (int i = 0; i < ntypes; ++i) n += touched(C[i].data(), dd * 4) + touched(P[i].data(), (slots + 1) * 8);
        report_count(tag + ": C and partials keep the poison (bytes)", (double)n);
        free_all(); return;
    }
    if (check) {
        size_t nd = 0; for (int i = 0; i < ntypes; ++i) nd += bit_diffs(C[i], C0[i]) + bit_diffs(P[i], P0[i]);
        report_count(tag + ": C, partials bitwise equal with and without the check", (double)nd);
        // res[k] = 2 sqrt(sum of nslots partials): (nslots + 16) u relative, as for the fp64 check
        auto st = d2h(dst, 1);
        ld s = 0; for (int q = 0; q < cn; ++q) s += hcp[q];
        const ld want = 2.0L * sqrtl(s);
        report_ratio(tag + ": st.res[k] = 2 sqrt(sum chk_partials)", ratio_of(fabsl((ld)st[0].res[k] - want), (ld)(cn + 16) * U64 * want));
    }
    size_t spare = 0;
    for (int i = 0; i < ntypes; ++i) {
        spare += touched(P[i].data() + slots, 8);
        f32_compare(tag + " type " + std::to_string(i), d, A[i], B[i], al[i], be[i], ga[i], C[i], &P[i]);
    }
    report_count(tag + ": the word after the last slot keeps the poison", (double)spare);
    free_all();
}

static void f32_first_case(int d) {
    const size_t dd = (size_t)d * d; const int slots = (d / 32) * (d / 32);
    Rng rng(555 + d);
    std::vector<double> A64(dd); for (auto& v : A64) v = rng.gauss() * 1.3;
    const double cval = 1.9, inv = 1.0 / cval;
    // every operation below is an IEEE double operation or a cast: the device must produce the same bits
    std::vector<float> Y0(dd), T0(dd);
    for (int r = 0; r < d; ++r) for (int q = 0; q < d; ++q) {
        const size_t e = (size_t)r * d + q;
        const double p = A64[e] * inv;
        Y0[e] = (float)p; T0[e] = (float)((r == q ? 1.5 : 0.0) - 0.5 * (double)(float)p);
    }
    Gemm32Args g; memset(&g, 0, sizeof(g));
    float *dY1 = dalloc<float>(dd), *dZ1 = dalloc<float>(dd); double* dP = dalloc<double>(slots);
    NsState s64; memset(&s64, 0, sizeof(s64)); s64.c = cval;
    g.C[0] = dY1; g.C[1] = dZ1; g.alpha[0] = 1.0f; g.beta_eye[0] = 0.0f; g.gamma[0] = 1.0f; g.partials[0] = dP;
    g.ntypes = 1; g.A64 = dupload(A64); g.st64 = dupload(std::vector<NsState>(1, s64));
    const int ret = gemm_f32_first_launch(d, g, 0); dsync();
    const std::string tag = "gemm_f32_first d=" + std::to_string(d);
    report_count(tag + ": launched", std::fabs((double)ret));
    auto Y1 = d2h(dY1, dd); auto Z1 = d2h(dZ1, dd); auto P = d2h(dP, slots);
    report_count(tag + ": Z1 = T0 = (float)(1.5 delta - 0.5 (float)(a / c)) bit for bit", (double)bit_diffs(Z1, T0));
    f32_compare(tag + " Y1 = Y0 T0", d, Y0, T0, 1.0f, 0.0f, 1.0f, Y1, &P);
    free_all();
}

static void section_f32() {
    printf("section f32: gemm_f32_launch, gemm_f32_first_launch\n");
    for (int d : {64, 128, 320, 512, 1024}) { f32_case(d, 1, false, false); f32_case(d, 2, true, false); }
    f32_case(128, 2, false, true);
    for (int d : {64, 320, 1024}) f32_first_case(d);
    Gemm32Args g; memset(&g, 0, sizeof(g));
    report_count("gemm_f32 d=96 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f32_launch(96, g, 0) - FAD_ERR_INVALID)));
    report_count("gemm_f32 d=32 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f32_launch(32, g, 0) - FAD_ERR_INVALID)));
    report_count("gemm_f32_first d=96 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f32_first_launch(96, g, 0) - FAD_ERR_INVALID)));
    report_count("gemm_f32_first d=32 -> FAD_ERR_INVALID", std::fabs((double)(gemm_f32_first_launch(32, g, 0) - FAD_ERR_INVALID)));
    dsync();
}

int main(int argc, char** argv) {
    struct { const char* name; void (*fn)(); } sections[] = {{"f64", section_f64}, {"f64big", section_f64big}, {"stats", section_stats}, {"f32", section_f32}};
    for (int a = 1; a < argc; ++a) {
        bool known = false; for (auto& s : sections) known |= (std::string(argv[a]) == s.name);
        if (!known) { printf("unknown section %s (f64, f64big, stats, f32)\n", argv[a]); return 1; }
    }
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    for (auto& s : sections) {
        bool run = (argc < 2); for (int a = 1; a < argc; ++a) run |= (std::string(argv[a]) == s.name);
        if (!run) continue;
        const int c0 = g_checks, f0 = g_fail; g_max_ratio = 0.0;
        s.fn();
        printf("section %s: %d checks, %d failed, largest err / bound %.3f\n", s.name, g_checks - c0, g_fail - f0, g_max_ratio);
    }
    if (g_fail) printf("%d checks FAILED\n", g_fail); else printf("all checks passed\n");
    return g_fail ? 1 : 0;
}
