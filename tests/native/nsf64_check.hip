// The float64 Newton-Schulz iteration below the public entry (fadtk_amd/csrc/frechet_f64.hip, ns_check.h), kernel by kernel on the GPU
// against host arithmetic in long double (test infrastructure, gfx950).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/nsf64_check tests/native/nsf64_check.hip
//   tests/native/nsf64_check [stats | schedule | first | check | run <problem file> ...]         (no argument = all but run)
// Exit code 0 = all checks passed, 1 = a check failed, 2 = a HIP error.
//
// gemm_f64.hip and frechet_f64.hip are included as they are; the host symbols they need (set_error, err_buf, num_cus, DevBuf,
// NsWorkspace::release) are supplied here.  ns_check_block is a __device__ function: the `check` section calls it from a one-line
// kernel of its own.  Every output buffer is filled with 0xEE bytes before each launch, so what nobody wrote is told from what was
// written, bit for bit.  Derived bounds print  err / bound  and pass at <= 1; exact expectations print a count and pass at 0.
//
// stats     ns_tilestats + ns_prepare on a given A (and C1, C2, mu1, mu2 for the traces and the mean term).  The host sums the same
//           doubles in long double: ||A||_F^2 (SqAcc), sum a_ij a_ji, tr A, tr C1, tr C2, the row and column sums of |A| (LinAcc) --
//           the bounds of tests/native/gemm_check.hip: a sum of N terms in any order is off by at most (N + 8) u sum |t|, u = 2^-53.
//           The tile partials are added up on the host and held to those bounds; the scale c of the armed state is held to what the
//           bounds of its inputs allow (sqrt, min, quotient: host_rule), and the host's branch of the rule -- U / 2.5, tr(A^2) / tr A, or
//           U with scaled steps -- has to be clear of every threshold by 4 bounds, else the CASE is reported as drifted (a failure of
//           the test's operands, not of the kernel).  Operands: a flat spectrum (I + small noise: the weighted mean), a k^-2 diagonal
//           with noise (participation ratio ~2.5: scaled steps, c = U), a non-normal upper triangle (tr(A^2) / tr A = 1 although every
//           norm is ~d: U / 2.5), Gaussian noise (tr A of either sign, cancellation in the cross term).  That the flat operand takes the
//           weighted mean at every d, the k^-2 one the scaled start and the non-normal one U / 2.5 at d >= 31 is asserted per case.
// schedule  mu[0..63] of the same states.  Not scaled: 64 ones, exactly.  Scaled: l_0 is recovered from mu_0^2 = 3 / (1 + l + l^2); the
//           recovery is uncertain by dl = 8 u (3 / mu_0^2) / (1 + 2 l) (two roundings of mu_0, one of the quotient, cancellation
//           against 1) + 128 u l (the device's own recurrence rounds ~8 times per step over at most 16 steps), and both l -> mu(l) (falling) and l -> the next l (rising) are monotone, so every later mu_k has to lie
//           between the recurrences started at l_0 - dl and l_0 + dl, widened by 8 u; the first k with l_k >= 0.9 and all after it hold
//           exactly 1.  l_0 itself against the float64 bisection of the same equation:
//             * 20 halvings of [0, 8] return the midpoint of an interval of width 8 / 2^19 that holds the root: |p - p*| <= 8 / 2^20;
//             * a comparison val(p) > pr can only go wrong within dp = e_v val / |val'| of the root, e_v the relative error of val in
//               float: every exp2f argument x (|x| <= 16 log2 d) carries the errors of __log2f and two roundings, r = 2^-20, so
//               exp2f(x) is off by ln 2 |x| r + 2^-22 relative; S(p) = (1 + e1) / 2 + (e2 - 1) / (1 - p) by
//               dS = e1 e(x1) / 2 + (e2 e(x2) + 2^-24 (e2 + 1)) / |1 - p| + 4 2^-24 S  (the quotient amplifies the rounding of e2 - 1
//               near p = 1), val = S(p)^2 / S(2p) by e_v = 2 dS(p) / S(p) + dS(2p) / S(2p) + 4 2^-24  (pr's own cast included);
//             * l_0 = exp2f(-p lg / 2) / 3:  dl / l <= (ln d / 2) (8 / 2^20 + dp) + ln 2 (p lg / 2) r + 2^-22 + 3 2^-24.
//           (val' by a central difference of the float64 function.)  The clamp to [1e-5, 0.5] is applied on both sides.
// first     ns_first: Y0 = A (1 / c) within two roundings of a / c; T0 = 1.5 mu delta - 0.5 mu^3 y from the DEVICE's y within
//           u |t| + 3.1 u |0.5 mu^3 y| + u 1.5 mu delta (mu^3 is two products, FMA or not); Z1 == T0 bitwise; the partial slots add up to
//           ||T0 - (1.5 mu - 0.5 mu^3) I||_F^2 within SqAcc of the device's own t; a problem that is done writes nothing; padding
//           between problems and slots past the grid keep the poison.  d * d is no multiple of 256.
// check     ns_check_block on synthetic partials and diagonal Y: a table of (residual, trace, mu) sequences whose expected state after
//           EVERY check is written out as literals beside the rule of ns_check.h it demonstrates.  Residuals are dyadic with few
//           bits, so (mu^3 r / 2)^2, its square root and the division by mu^3 are exact and res[k] is compared bit for bit.
// run       run_ns whole, on problems read from a file that tests/test_gpu_native.py writes from tests/frechet_f64_reference.py
//           (inputs, the emulation's stop code and count, the eigenvalue value and the bound on it): a batch with strides, with a
//           shared first covariance where the file has one, every problem alone, first_chunk = 1, 2, 4, 7, 8 and reuse_prepared.  The
//           decisions are the device's, so the chunking must not change a bit of the answer.  Prints every problem's residual and
//           trace history.
#include "../../fadtk_amd/csrc/gemm_f64.hip"
#include "../../fadtk_amd/csrc/frechet_f64.hip"

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
int DevBuf::reserve(size_t bytes) {
    if (p && cap >= bytes) return FAD_OK;
    release();
    FAD_HIP_TRY(hipMalloc(&p, bytes + 256));
    cap = bytes;
    return FAD_OK;
}
void DevBuf::release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
void NsWorkspace::release() {
    mats.release(); small.release(); stage.release();
    if (pinned) (void)hipHostFree(pinned);
    pinned = nullptr; pinned_cap = 0;
}
}  // namespace fad

using namespace fad;
typedef long double ld;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

static const double U64 = 0x1p-53;
static int g_fail = 0, g_checks = 0;
static double g_max_ratio = 0.0;
static void report(const char* what, double err, double tol) {
    const bool ok = (err <= tol) && (err == err);
    printf("  %-100s err %.3e  (tol %.1e)  %s\n", what, err, tol, ok ? "ok" : "FAIL");
    ++g_checks;
    if (!ok) ++g_fail;
}
static void report_ratio(const std::string& what, double ratio) {
    if (ratio == ratio && ratio > g_max_ratio) g_max_ratio = ratio;
    report((what + ": err / bound").c_str(), ratio, 1.0);
}
static void report_count(const std::string& what, double n) { report(what.c_str(), n, 0.0); }
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
static void free_all() { for (void* p : g_allocs) CK(hipFree(p)); g_allocs.clear(); }
static void dsync() { CK(hipDeviceSynchronize()); CK(hipGetLastError()); }
static size_t touched(const void* p, size_t bytes) {
    const unsigned char* q = static_cast<const unsigned char*>(p);
    size_t n = 0; for (size_t i = 0; i < bytes; ++i) n += (q[i] != 0xEE); return n;
}
static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

struct Rng {
    std::mt19937_64 g; std::normal_distribution<double> n{0.0, 1.0};
    explicit Rng(uint64_t seed) : g(seed) {}
    double gauss() { return n(g); }
    double uni(double a, double b) { return a + (b - a) * (double)(g() >> 11) * 0x1p-53; }
};

// (tests/native/gemm_check.hip has the derivations)
struct SqAcc {
    ld e = 0, tb = 0, mag = 0; int n = 0;
    void add(ld eh, ld b) { const ld m = fabsl(eh) + b; e += eh * eh; tb += (2 * fabsl(eh) + b) * b + U64 * m * m; mag += m * m; ++n; }
    ld bound() const { return tb + (ld)(n + 8) * U64 * mag; }
};
struct LinAcc {
    ld e = 0, tb = 0, mag = 0; int n = 0;
    void add(ld th, ld b) { e += th; tb += b; mag += fabsl(th) + b; ++n; }
    ld bound() const { return tb + (ld)(n + 8) * U64 * mag; }
};

// a state as clear_states leaves it: the flags cleared, everything else poison
static NsState cleared_state() {
    NsState s; memset(&s, 0xEE, sizeof(s));
    s.too_few[0] = s.too_few[1] = 0; s.done = 0; s.finished = 0; s.nonfinite = 0; s.conv = 0; s.final_iter = -1; s.upd_skip[0] = s.upd_skip[1] = 0;
    return s;
}
// ... and as ns_prepare arms it (res[] / tr[] stay poison: a check may only read what an earlier check wrote)
static NsState armed_state(double c) {
    NsState s = cleared_state();
    s.c = c; s.tr1 = s.tr2 = s.mean_term = 0.0; s.res_last = 0.0; s.tr_last = 0.0; s.res_min = 1e300; s.tr_safe = 0.0; s.has_safe = 0; s.pad_ = 0;
    for (int k = 0; k < kMaxIter; ++k) s.mu[k] = 1.0;
    return s;
}

// ================================================================================================ stats + schedule
enum Kind { FLAT, DECAY, NONNORMAL, NOISE, ZERO, NAN_A, NAN_C1, INF_MU, OVERFLOW_A };
static const char* kind_name(int k) {
    static const char* n[] = {"flat", "k^-2", "non-normal", "noise", "zero", "NaN in A", "NaN in C1", "Inf in mu", "overflowing |A|_F^2"};
    return n[k];
}
static void make_A(int kind, int d, Rng& rng, double* A) {
    for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) {
        double v = 0.0;
        switch (kind) {
            case FLAT: v = (i == j ? 1.0 : 0.0) + 0.02 * rng.uni(0.0, 1.0) / d; break;
            case DECAY: v = (i == j ? 1.0 / ((double)(i + 1) * (i + 1)) : 0.0) + 1e-4 * rng.gauss() / ((double)(i + 1) * (j + 1) * d); break;
            case NONNORMAL: v = (i == j) ? 1.0 : (j > i ? 1.0 + 0.1 * rng.uni(0.0, 1.0) : 0.0); break;
            case OVERFLOW_A: v = 1e160 * rng.gauss(); break;
            case ZERO: v = 0.0; break;
            default: v = rng.gauss(); break;
        }
        A[(size_t)i * d + j] = v;
    }
    // d = 1: tr(A^2) / tr A and U coincide, so the branch hangs on "<=" between equal numbers; an entry of eight bits makes a * a, its
    // quotient by a and its square root exact, and both sides take the same branch
    if (d == 1 && kind <= NOISE) { A[0] = std::nearbyint(A[0] * 64.0) / 64.0; if (A[0] == 0.0) A[0] = 1.0 / 64.0; }
    if (kind == NAN_A) A[(size_t)(d / 2) * d + d / 3] = NAN;
}

// sum_{k=1..d} k^-p by the trapezoid rule, its inverse by bisection, in float64 (header: schedule)
static double host_S(double p, int d) {
    const double lg = std::log((double)d), ends = 0.5 * (1.0 + std::exp(-p * lg));
    if (std::fabs(p - 1.0) < 1e-12) return ends + lg;
    return ends + (std::exp((1.0 - p) * lg) - 1.0) / (1.0 - p);
}
static double host_val(double p, int d) { const double s = host_S(p, d); return s * s / host_S(2.0 * p, d); }
static double host_p(double pr, int d) {
    double lo = 0.0, hi = 8.0;
    for (int it = 0; it < 200; ++it) { const double p = 0.5 * (lo + hi); if (host_val(p, d) > pr) lo = p; else hi = p; }
    return 0.5 * (lo + hi);
}
static double exp2_err(double x) { return std::log(2.0) * std::fabs(x) * 0x1p-20 + 0x1p-22; }
static double dS_float(double p, int d) {
    const double lg2 = std::log2((double)d), e1 = std::exp2(-p * lg2), e2 = std::exp2((1.0 - p) * lg2);
    const double den = std::fmax(std::fabs(1.0 - p), 1e-4);
    return 0.5 * e1 * exp2_err(p * lg2) + (e2 * exp2_err((1.0 - p) * lg2) + 0x1p-24 * (e2 + 1.0)) / den + 4 * 0x1p-24 * host_S(p, d);
}
// relative bound on |l0(device) - l0(host)| before the clamp
static double l0_rel_bound(double p, int d) {
    const double ev = 2.0 * dS_float(p, d) / host_S(p, d) + dS_float(2.0 * p, d) / host_S(2.0 * p, d) + 4 * 0x1p-24;
    const double h = 1e-4, slope = std::fabs(host_val(p + h, d) - host_val(std::fmax(p - h, 0.0), d)) / (p + h - std::fmax(p - h, 0.0));
    const double dp = (slope > 0) ? ev * host_val(p, d) / slope : INFINITY;
    return 0.5 * std::log((double)d) * (8.0 / 1048576.0 + dp) + std::log(2.0) * 0.5 * p * std::log2((double)d) * 0x1p-20 + 0x1p-22 + 3 * 0x1p-24;
}
static double clamp_l0(double l) { return l > 0.5 ? 0.5 : (l < 1e-5 ? 1e-5 : l); }
// the recurrence from l0: mu[k] and the number of scaled steps
static int host_schedule(double l, double* mu) {
    int k = 0;
    for (; k < kMaxIter && l < 0.9; ++k) { const double m = std::sqrt(3.0 / (1.0 + l + l * l)); l = m * l * (3.0 - m * m * l * l) / 2.0; mu[k] = m; }
    const int n = k;
    for (; k < kMaxIter; ++k) mu[k] = 1.0;
    return n;
}

struct HostRule {
    ld fro2, trA2, trA, tr1, tr2, inf_norm, one_norm, mean;
    ld b_fro2, b_trA2, b_trA, b_tr1, b_tr2, b_inf, b_one, b_mean;
    std::vector<ld> row, col, b_row, b_col;
    bool bad = false, zero = false, scaled = false, hopeless = false, drifted = false;
    int branch = 0;             // 0 = U / 2.5, 1 = weighted mean, 2 = U (scaled)
    ld c = 0, b_c = 0, pr = 0;
};
static bool clear_of(ld x, ld y, ld bx, ld by) { return fabsl(x - y) > 4 * (bx + by); }
static HostRule host_rule(const double* A, const double* C1, const double* C2, const double* mu1, const double* mu2, int d, bool allow_scaled) {
    HostRule h;
    SqAcc fro; LinAcc cross, tra, t1, t2, mean;
    h.row.assign(d, 0); h.col.assign(d, 0); h.b_row.assign(d, 0); h.b_col.assign(d, 0);
    std::vector<LinAcc> rows(d), cols(d);
    for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) {
        const ld a = A[(size_t)i * d + j], at = A[(size_t)j * d + i];
        fro.add(a, 0);
        cross.add(a * at, U64 * fabsl(a * at));
        rows[i].add(fabsl(a), 0); cols[j].add(fabsl(a), 0);
        if (i == j) { tra.add(a, 0); t1.add(C1[(size_t)i * d + i], 0); t2.add(C2[(size_t)i * d + i], 0); }
    }
    for (int i = 0; i < d; ++i) { const ld g = (ld)mu1[i] - (ld)mu2[i]; mean.add(g * g, 4 * U64 * g * g); }
    h.fro2 = fro.e; h.b_fro2 = fro.bound(); h.trA2 = cross.e; h.b_trA2 = cross.bound(); h.trA = tra.e; h.b_trA = tra.bound();
    h.tr1 = t1.e; h.b_tr1 = t1.bound(); h.tr2 = t2.e; h.b_tr2 = t2.bound(); h.mean = mean.e; h.b_mean = mean.bound();
    h.inf_norm = 0; h.one_norm = 0; h.b_inf = 0; h.b_one = 0;
    for (int i = 0; i < d; ++i) {
        h.row[i] = rows[i].e; h.b_row[i] = rows[i].bound(); h.col[i] = cols[i].e; h.b_col[i] = cols[i].bound();
        h.inf_norm = std::max(h.inf_norm, h.row[i]); h.b_inf = std::max(h.b_inf, h.b_row[i]);
        h.one_norm = std::max(h.one_norm, h.col[i]); h.b_one = std::max(h.b_one, h.b_col[i]);
    }
    auto finite = [](ld v) { return v == v && fabsl(v) <= (ld)1.7976931348623157e308; };
    h.bad = !(finite(h.fro2) && finite(h.tr1) && finite(h.tr2) && finite(h.mean));
    if (h.bad) return h;
    const ld fro_n = sqrtl(h.fro2), b_fro = (h.fro2 > 0) ? h.b_fro2 / (2 * fro_n) + 2 * U64 * fro_n : 0;
    const ld u = std::min(fro_n, std::min(h.inf_norm, h.one_norm)), b_u = std::max(b_fro, std::max(h.b_inf, h.b_one));
    if (!(u > 0)) { h.zero = true; h.c = 1.0; return h; }
    const ld lo = u / 2.5L, b_lo = b_u / 2.5L + 2 * U64 * lo;
    ld w = 0, b_w = 0;
    if (!clear_of(h.trA, 0, h.b_trA, 0)) h.drifted = true;
    if (h.trA > 0) {
        w = h.trA2 / h.trA;
        b_w = (h.b_trA2 + fabsl(w) * h.b_trA) / (h.trA - h.b_trA) + 2 * U64 * fabsl(w);
    }
    h.branch = 0; h.c = lo; h.b_c = b_lo;
    if (h.trA > 0) {
        if (!clear_of(w, lo, b_w, b_lo) || (d > 1 && !clear_of(w, u, b_w, b_u))) h.drifted = true;       // (d = 1: make_A)
        if (w > lo && w <= u) { h.branch = 1; h.c = w; h.b_c = b_w; }
    }
    if (h.trA > 0 && h.trA2 > 0) {
        h.pr = h.trA * h.trA / h.trA2;
        const ld q1 = h.trA * h.trA, q2 = 0.25L * d * h.trA2, q3 = 0.25L * d * h.fro2;
        const ld bq1 = 2 * fabsl(h.trA) * h.b_trA + 4 * U64 * q1;
        if (!clear_of(q1, q2, bq1, 0.25L * d * h.b_trA2 + 4 * U64 * q2) || !clear_of(q1, q3, bq1, 0.25L * d * h.b_fro2 + 4 * U64 * q3)) h.drifted = true;
        h.scaled = allow_scaled && q1 < q2;
        h.hopeless = q1 < q3;
        if (h.scaled) { h.branch = 2; h.c = u; h.b_c = b_u; }
    } else {
        if (h.trA > 0 && !clear_of(h.trA2, 0, h.b_trA2, 0)) h.drifted = true;
        h.hopeless = h.trA * h.trA < 0.25L * d * h.fro2;
    }
    return h;
}

static void stats_case(int d, const std::vector<int>& kinds, bool allow_scaled, bool with_s32, bool do_stats, bool do_sched, uint64_t seed) {
    const int B = (int)kinds.size();
    const int64_t dd = (int64_t)d * d;
    const int nb = (int)stat_blocks(d);
    const size_t sd = stat_doubles(d);
    Rng rng(seed * 1000003 + d);
    std::vector<double> A((size_t)B * dd), C1((size_t)B * dd), C2((size_t)B * dd), mu1((size_t)B * d), mu2((size_t)B * d);
    std::vector<NsState> st(B);
    std::vector<Ns32State> s32(B);
    const int mid = (B == 3) ? 1 : -1;                    // B = 3: the middle problem is done before the launches
    for (int b = 0; b < B; ++b) {
        make_A(kinds[b], d, rng, &A[(size_t)b * dd]);
        for (int64_t e = 0; e < dd; ++e) { C1[(size_t)b * dd + e] = rng.gauss(); C2[(size_t)b * dd + e] = rng.gauss() * 3.0; }
        for (int i = 0; i < d; ++i) { mu1[(size_t)b * d + i] = rng.gauss(); mu2[(size_t)b * d + i] = rng.gauss(); }
        if (kinds[b] == NAN_C1) C1[(size_t)b * dd + (size_t)(d / 2) * d + d / 2] = NAN;
        if (kinds[b] == INF_MU) mu2[(size_t)b * d + d - 1] = INFINITY;
        st[b] = cleared_state();
        if (b == mid) st[b].done = 1;
        memset(&s32[b], 0xEE, sizeof(Ns32State));
    }
    double *dA = dupload(A), *dC1 = dupload(C1), *dC2 = dupload(C2), *dm1 = dupload(mu1), *dm2 = dupload(mu2);
    double* dstats = dalloc<double>((size_t)B * sd);
    NsState* dst = dupload(st);
    Ns32State* ds32 = dupload(s32);
    hipLaunchKernelGGL(ns_tilestats, dim3(nb, nb, B), dim3(256), 0, 0, dA, d, dC1, dd, dC2, dd, dstats, dst);
    if (with_s32 && B != 1) { printf("stats_case: the low-precision state belongs to a launch of one problem\n"); exit(1); }
    hipLaunchKernelGGL(ns_prepare, dim3(B), dim3(256), 0, 0, dstats, d, nb, dm1, (int64_t)d, dm2, (int64_t)d, -1, dst, 0,
                       with_s32 ? ds32 : (Ns32State*)nullptr, allow_scaled ? 1 : 0);
    dsync();
    const std::vector<double> hstats = d2h(dstats, (size_t)B * sd);
    const std::vector<NsState> got = d2h(dst, B);
    const std::vector<Ns32State> got32 = d2h(ds32, B);

    for (int b = 0; b < B; ++b) {
        const std::string tag = std::string(do_stats ? "stats " : "schedule ") + kind_name(kinds[b]) + " d=" + std::to_string(d) + " b=" + std::to_string(b) + "/" +
                                std::to_string(B) + (allow_scaled ? "" : " allow_scaled=0") + (with_s32 ? " +s32" : "");
        const double* S = &hstats[(size_t)b * sd];
        if (b == mid) {
            if (do_stats) {
                report_count(tag + " done before: statistics written (bytes)", (double)touched(S, sd * sizeof(double)));
                report_count(tag + " done before: state bytes changed", (double)(memcmp(&got[b], &st[b], sizeof(NsState)) != 0));
            }
            continue;
        }
        const HostRule h = host_rule(&A[(size_t)b * dd], &C1[(size_t)b * dd], &C2[(size_t)b * dd], &mu1[(size_t)b * d], &mu2[(size_t)b * d], d, allow_scaled);
        const NsState& g = got[b];
        if (h.drifted) { report_count(tag + ": CASE DRIFTED (the host's branch is within 4 bounds of a threshold)", 1.0); continue; }
        {
            // the branch each operand is MADE for, at the sizes where it is meant to hold: a change to make_A or the seeds that loses one fails here
            const int want = (kinds[b] == FLAT) ? 1 : (kinds[b] == DECAY && d >= 31 && allow_scaled) ? 2 : (kinds[b] == NONNORMAL && d >= 31) ? 0 : -1;
            static const char* wn[] = {"U / 2.5", "tr(A^2) / tr A", "U with scaled steps"};
            if (want >= 0) report_count(tag + ": the host's branch of the scale rule is not the one this operand is for (" + wn[want] + ")", (double)(h.bad || h.zero || h.branch != want));
            if (kinds[b] == DECAY && !allow_scaled) report_count(tag + ": scaled although allow_scaled = 0", (double)(h.branch == 2 || h.scaled));
        }
        if (do_stats) {
            // ---- tile partials of ns_tilestats
            const double *rowabs = S, *colabs = S + (size_t)nb * d, *scal = S + 2 * (size_t)nb * d;
            if (!h.bad) {
                ld sums[5] = {0, 0, 0, 0, 0};
                for (int t = 0; t < nb * nb; ++t) for (int q = 0; q < 5; ++q) sums[q] += scal[(size_t)kStatScal * t + q];
                report_ratio(tag + " |A|_F^2", ratio_of(fabsl(sums[0] - h.fro2), h.b_fro2));
                report_ratio(tag + " sum a_ij a_ji", ratio_of(fabsl(sums[1] - h.trA2), h.b_trA2));
                report_ratio(tag + " tr A", ratio_of(fabsl(sums[2] - h.trA), h.b_trA));
                report_ratio(tag + " tr C1 (tiles)", ratio_of(fabsl(sums[3] - h.tr1), h.b_tr1));
                report_ratio(tag + " tr C2 (tiles)", ratio_of(fabsl(sums[4] - h.tr2), h.b_tr2));
                double mr = 0, mc = 0;
                for (int i = 0; i < d; ++i) {
                    ld rs = 0, cs = 0;
                    for (int k = 0; k < nb; ++k) { rs += rowabs[(size_t)k * d + i]; cs += colabs[(size_t)k * d + i]; }
                    upd(mr, ratio_of(fabsl(rs - h.row[i]), h.b_row[i])); upd(mc, ratio_of(fabsl(cs - h.col[i]), h.b_col[i]));
                }
                report_ratio(tag + " row sums of |A| (max over rows)", mr);
                report_ratio(tag + " column sums of |A| (max over columns)", mc);
            }
            size_t spare = 0;
            for (int t = 0; t < nb * nb; ++t) spare += touched(scal + (size_t)kStatScal * t + 5, 3 * sizeof(double));
            report_count(tag + " spare words of the tile records written (bytes)", (double)spare);
            // ---- the armed state
            if (h.bad) {
                report_count(tag + ": nonfinite, done, finished not all 1", (double)!(g.nonfinite == 1 && g.done == 1 && g.finished == 1));
            } else if (h.zero) {
                report_count(tag + ": not (done, finished, conv = 1, final_iter = 0, c = 1, nonfinite = 0)",
                             (double)!(g.done == 1 && g.finished == 1 && g.conv == 1 && g.final_iter == 0 && g.c == 1.0 && g.nonfinite == 0));
            } else {
                static const char* bn[] = {"U / 2.5", "tr(A^2) / tr A", "U (scaled)"};
                report_ratio(tag + " c, branch " + bn[h.branch], ratio_of(fabsl((ld)g.c - h.c), h.b_c));
                report_ratio(tag + " tr C1", ratio_of(fabsl((ld)g.tr1 - h.tr1), h.b_tr1));
                report_ratio(tag + " tr C2", ratio_of(fabsl((ld)g.tr2 - h.tr2), h.b_tr2));
                report_ratio(tag + " mean term", ratio_of(fabsl((ld)g.mean_term - h.mean), h.b_mean));
                const bool armed = g.done == 0 && g.finished == 0 && g.nonfinite == 0 && g.conv == 0 && g.final_iter == -1 && g.res_last == 0.0 &&
                                   g.tr_last == 0.0 && g.res_min == 1e300 && g.tr_safe == 0.0 && g.has_safe == 0 && g.upd_skip[0] == 0 && g.upd_skip[1] == 0;
                report_count(tag + ": state not armed as documented", (double)!armed);
            }
            report_count(tag + ": res[] / tr[] history written by the set-up (bytes)", (double)(touched(g.res, sizeof(g.res)) + touched(g.tr, sizeof(g.tr))));
            if (with_s32) {
                const Ns32State& q = got32[b];
                const bool off = h.bad || h.zero || h.hopeless;
                const bool reset = q.ok == 0 && q.final_iter == -1 && q.skip_corr == 1 && q.decided_at == -1 && q.strict == 0 && q.grew == 0 && q.res[0] == 1e300;
                const bool flags = off ? (q.done == 1 && q.finished == 1 && q.failed == 1 && q.upd_skip[0] == 1 && q.upd_skip[1] == 1)
                                       : (q.done == 0 && q.finished == 0 && q.failed == 0 && q.upd_skip[0] == 0 && q.upd_skip[1] == 0);
                report_count(tag + (off ? ": low-precision leg not switched off ((tr A)^2 < d/4 |A|_F^2, bad or zero)" : ": low-precision leg not left on"),
                             (double)!(reset && flags));
            }
        }
        if (do_sched && !h.bad) {
            double ones = 0;
            if (!h.scaled || h.zero) {
                for (int k = 0; k < kMaxIter; ++k) ones += !same_bits(g.mu[k], 1.0);
                report_count(tag + " not scaled: mu[k] that are not exactly 1", ones);
                continue;
            }
            const double m0 = g.mu[0], q = 3.0 / (m0 * m0);
            const double l0 = (-1.0 + std::sqrt(1.0 - 4.0 * (1.0 - q))) / 2.0;
            const double dl = 8 * U64 * q / (1.0 + 2.0 * l0) + 128 * U64 * l0;       // (+ 8 u per step of the device's recurrence, 16 steps at most)
            report_count(tag + " l0 = " + std::to_string(l0) + " outside [1e-5, 0.5]", (double)!(l0 + dl >= 1e-5 && l0 - dl <= 0.5));
            const double p = host_p((double)h.pr, d), lh_raw = std::exp(-0.5 * p * std::log((double)d)) / 3.0, lh = clamp_l0(lh_raw);
            const double bl = l0_rel_bound(p, d) * lh_raw + dl;
            printf("    (participation ratio %.4f of %d, p = %.6f, host l0 = %.6e, device l0 = %.6e, relative bound %.2e)\n", (double)h.pr, d, p, lh, l0, bl / lh);
            report_ratio(tag + " l0 against the float64 bisection", std::fabs(l0 - lh) / bl);
            double mlo[kMaxIter], mhi[kMaxIter];
            const int nlo = host_schedule(std::fmax(l0 - dl, 0.0), mlo), nhi = host_schedule(l0 + dl, mhi);
            if (nlo != nhi) { report_count(tag + ": CASE DRIFTED (l crosses 0.9 within the uncertainty of l0)", 1.0); continue; }
            double worst = 0, tail = 0;
            for (int k = 0; k < nlo; ++k) {
                const double a = std::fmin(mlo[k], mhi[k]) * (1 - 8 * U64), z = std::fmax(mlo[k], mhi[k]) * (1 + 8 * U64);
                upd(worst, std::fabs(g.mu[k] - 0.5 * (a + z)) / (0.5 * (z - a)));
            }
            for (int k = nlo; k < kMaxIter; ++k) tail += !same_bits(g.mu[k], 1.0);
            report_ratio(tag + " mu[1.." + std::to_string(nlo - 1) + "] between the recurrences from l0 -+ dl", worst);
            report_count(tag + " mu[k] after the last scaled step that are not exactly 1", tail);
        }
    }
    free_all();
}

static void section_stats(bool do_stats, bool do_sched) {
    printf("== %s\n", do_stats ? "stats: ns_tilestats + ns_prepare" : "schedule: mu[k] of ns_prepare");
    const int dims[] = {1, 2, 31, 32, 33, 64, 65, 100, 130};
    uint64_t seed = 1;
    for (int d : dims) {
        for (int k = FLAT; k <= NOISE; ++k) {
            stats_case(d, {k}, true, true, do_stats, do_sched, ++seed);          // (the low-precision state is ONE problem's: B = 1 only)
            stats_case(d, {k, (k + 1) % 4, (k + 2) % 4}, true, false, do_stats, do_sched, ++seed);
        }
        stats_case(d, {DECAY, FLAT, DECAY}, false, false, do_stats, do_sched, ++seed);            // allow_scaled = 0
    }
    if (do_stats)
        for (int d : {33, 64})
            for (int k = ZERO; k <= OVERFLOW_A; ++k) {
                stats_case(d, {k}, true, true, true, false, ++seed);
                stats_case(d, {FLAT, k, k}, true, false, true, false, ++seed);
            }
}

// ================================================================================================ first
static void first_case(int d, double mu0, uint64_t seed) {
    const int B = 3;
    const int64_t dd = (int64_t)d * d, stride = dd + 5;
    const int nslots = (int)cdiv(dd, 256), pstride = nslots + 7;
    Rng rng(seed * 7919 + d);
    std::vector<double> A((size_t)B * dd);
    for (double& v : A) v = rng.gauss();
    std::vector<NsState> st(B);
    for (int b = 0; b < B; ++b) { st[b] = armed_state(b == 0 ? 2.7 : 0.37 + 0.011 * d); st[b].mu[0] = (b == 2) ? mu0 : (mu0 == 1.0 ? 1.0 : 1.0 + 0.5 * (mu0 - 1.0)); }
    st[1].done = 1;
    double* dA = dupload(A);
    NsState* dst = dupload(st);
    double *dY = dalloc<double>((size_t)B * stride), *dT = dalloc<double>((size_t)B * stride), *dZ = dalloc<double>((size_t)B * stride);
    double* dP = dalloc<double>((size_t)B * pstride);
    hipLaunchKernelGGL(ns_first, dim3(nslots, B), dim3(256), 0, 0, dA, d, dst, dY, dT, dZ, stride, dP, pstride);
    dsync();
    const std::vector<double> Y = d2h(dY, (size_t)B * stride), T = d2h(dT, (size_t)B * stride), Z = d2h(dZ, (size_t)B * stride), P = d2h(dP, (size_t)B * pstride);
    const std::vector<NsState> after = d2h(dst, B);
    for (int b = 0; b < B; ++b) {
        const std::string tag = "first d=" + std::to_string(d) + " b=" + std::to_string(b) + " mu=" + std::to_string(st[b].mu[0]);
        size_t pad = touched(&Y[(size_t)b * stride + dd], 5 * 8) + touched(&T[(size_t)b * stride + dd], 5 * 8) + touched(&Z[(size_t)b * stride + dd], 5 * 8);
        report_count(tag + " padding behind Y0 / T / Z1 written (bytes)", (double)pad);
        report_count(tag + " state bytes changed", (double)(memcmp(&after[b], &st[b], sizeof(NsState)) != 0));
        if (b == 1) {
            report_count(tag + " done: outputs written (bytes)", (double)(touched(&Y[(size_t)b * stride], dd * 8) + touched(&T[(size_t)b * stride], dd * 8) +
                                                                         touched(&Z[(size_t)b * stride], dd * 8) + touched(&P[(size_t)b * pstride], (size_t)pstride * 8)));
            continue;
        }
        const ld c = st[b].c, m = st[b].mu[0], m3 = m * m * m, g = 1.5L * m - 0.5L * m3;
        double ry = 0, rt = 0, diff = 0;
        SqAcc acc;
        for (int r = 0; r < d; ++r) for (int q = 0; q < d; ++q) {
            const size_t e = (size_t)b * stride + (size_t)r * d + q;
            const ld a = A[(size_t)b * dd + (size_t)r * d + q], yx = a / c, y = Y[e];
            upd(ry, ratio_of(fabsl(y - yx), 2.01L * U64 * fabsl(yx)));
            const ld dg = (r == q) ? 1.0L : 0.0L, tx = 1.5L * m * dg - 0.5L * m3 * y, t = T[e];
            upd(rt, ratio_of(fabsl(t - tx), U64 * fabsl(tx) + 3.1L * U64 * fabsl(0.5L * m3 * y) + U64 * 1.5L * m * dg));
            diff += !same_bits(T[e], Z[e]);
            const ld eh = t - g * dg;
            acc.add(eh, U64 * fabsl(eh) + dg * (U64 * fabsl(g) + U64 * m3));
        }
        report_ratio(tag + " Y0 = A / c", ry);
        report_ratio(tag + " T0 from the device's Y0", rt);
        report_count(tag + " elements with T0 != Z1 bitwise", diff);
        ld s = 0;
        for (int i = 0; i < nslots; ++i) s += P[(size_t)b * pstride + i];
        report_ratio(tag + " partial slots add up to |T0 - (1.5 mu - 0.5 mu^3) I|_F^2", ratio_of(fabsl(s - acc.e), acc.bound()));
        report_count(tag + " slots past the grid written (bytes)", (double)touched(&P[(size_t)b * pstride + nslots], 7 * 8));
    }
    free_all();
}
static void section_first() {
    printf("== first: ns_first\n");
    uint64_t seed = 100;
    for (int d : {1, 33, 100, 130}) for (double mu0 : {1.0, 1.37}) first_case(d, mu0, ++seed);
}

// ================================================================================================ check
__global__ __launch_bounds__(256) void check_kernel(NsCheckArgs a) {
    __shared__ double red[4];
    ns_check_block(a, (int64_t)blockIdx.x, red);
}

static const double NF = INFINITY;            // "the residual left the floats": an infinite partial sum
struct Expect { int done, finished, conv, final_iter, skip0, skip1, nonfinite; double tr_last; };
struct Step { double res, tr, mu; Expect e; };
struct Row { const char* name; const char* rule; int max_iter; double tol_res; std::vector<Step> steps; };

// d = 4, tol_tr = 1e-13.  res = the residual ||I - Z Y||_F the check must arrive at (the partials hold (mu^3 res / 2)^2 in three slots);
// tr = trace of the diagonal Y handed to the check (NaN: a NaN on its diagonal).  Expect = the state after that check.
static std::vector<Row> check_table() {
    const double t40 = 0x1p-40, q = 0x1p-21;      // q: 3/4 q^2 + 1/4 q^3 = 0.75 * 2^-42 (1 + 2^-21 / 3) <= 2^-40
    std::vector<Row> R;
    R.push_back({"tolerance reached", "res <= a.tol_res: conv = 1, finish; Y_k is the answer; the next launches are switched off, this word by the next check", 64, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {0x1p-4, 2.5, 1.0, {0, 0, 0, 1, 0, 0, 0, 2.5}},
                  {0x1p-45, 2.75, 1.0, {1, 1, 1, 2, 0, 1, 0, 2.75}}}});
    R.push_back({"predicted finish", "bound <= a.tol_res: done = 1, conv = 1, res_last = bound, upd_skip[(k + 1) & 1] = 1; the next check closes the problem with trace(Y_{k+1})", 64, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {q, 2.5, 1.0, {1, 0, 1, 1, 1, 0, 0, 2.5}},
                  {99.0, 2.625, 1.0, {1, 1, 1, 2, 1, 1, 0, 2.625}}}});           // (res of the closing step: partials the check must not read)
    R.push_back({"stalled: not before k = 2", "stalled = k >= 2 && |tr - tr_prev| <= tol_tr |tr| && |res - res_prev| <= 1e-9 res", 64, t40,
                 {{0.5, 3.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 3.0}},
                  {0.5, 3.0, 1.0, {0, 0, 0, 1, 0, 0, 0, 3.0}},                   // both still at k = 1: goes on
                  {0.5, 3.0, 1.0, {1, 1, 2, 2, 0, 1, 0, 3.0}}}});
    R.push_back({"stalled: not when only the trace pauses", "both must stand still (the trace alone can pause by coincidence)", 64, t40,
                 {{0.5, 3.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 3.0}},
                  {0.25, 3.0, 1.0, {0, 0, 0, 1, 0, 0, 0, 3.0}},
                  {0.125, 3.0, 1.0, {0, 0, 0, 2, 0, 0, 0, 3.0}},                 // trace still, residual halves: goes on
                  {0.125, 3.0, 1.0, {1, 1, 2, 3, 1, 0, 0, 3.0}}}});
    R.push_back({"runaway", "trace quiet (two increments <= 1e-9 |tr|) while the residual has GROWN twice in a row: tr_last = tr_prev, conv = 2", 64, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {0.25, 3.0, 1.0, {0, 0, 0, 1, 0, 0, 0, 3.0}},
                  {0.375, 3.0, 1.0, {0, 0, 0, 2, 0, 0, 0, 3.0}},
                  {0.5, 3.0 + 0x1p-40, 1.0, {1, 1, 2, 3, 1, 0, 0, 3.0}}}});
    R.push_back({"explode, the safe trace returned", "k >= 4, the residual quadruples: the trace of the last iterate whose residual was within 1.5x of the smallest seen, "
                 "provided the trace of the previous iterate still agrees with it to 1e-6", 64, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {0.25, 2.5, 1.0, {0, 0, 0, 1, 0, 0, 0, 2.5}},
                  {0.125, 3.0, 1.0, {0, 0, 0, 2, 0, 0, 0, 3.0}},                 // smallest residual: tr_safe = 3
                  {0.25, 3.0 + 0x1p-22, 1.0, {0, 0, 0, 3, 0, 0, 0, 3.0 + 0x1p-22}},   // 2x the smallest: not safe; trace 8e-8 off
                  {1.25, 7.0, 1.0, {1, 1, 2, 4, 0, 1, 0, 3.0}}}});                // 5x the previous residual
    R.push_back({"explode refused: goes non-finite", "a product with genuinely negative eigenvalues diverges in the trace as well: that stays an error", 64, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {0.25, 2.5, 1.0, {0, 0, 0, 1, 0, 0, 0, 2.5}},
                  {0.125, 3.0, 1.0, {0, 0, 0, 2, 0, 0, 0, 3.0}},
                  {0.25, 3.5, 1.0, {0, 0, 0, 3, 0, 0, 0, 3.5}},                  // the trace has moved by a sixth
                  {NF, 7.0, 1.0, {1, 1, 0, 3, 0, 1, 1, 3.5}}}});
    R.push_back({"max_iter", "k + 1 >= a.max_iter: conv = 0, finish", 3, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {0.25, 2.5, 1.0, {0, 0, 0, 1, 0, 0, 0, 2.5}},
                  {0.125, 2.75, 1.0, {1, 1, 0, 2, 0, 1, 0, 2.75}}}});
    R.push_back({"non-finite residual", "!finite: nonfinite = 1, finish; the last finite iterate stays in tr_last / final_iter", 64, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {NF, 2.5, 1.0, {1, 1, 0, 0, 1, 0, 1, 2.0}}}});
    R.push_back({"non-finite trace on the predicted closing check", "st->done: finite = (tr == tr) && !isinf(tr); if (!finite) nonfinite = 1", 64, t40,
                 {{0.5, 2.0, 1.0, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {q, 2.5, 1.0, {1, 0, 1, 1, 1, 0, 0, 2.5}},
                  {99.0, NAN, 1.0, {1, 1, 1, 2, 1, 1, 1, NAN}}}});
    // mu_1 = 1.5 (mu^3 = 3.375, exact): the partials hold (3.375 res / 2)^2; with tol = 2^-44, res = 2^-45 is inside the tolerance and
    // 3.375 * 2^-45 is not -- without the division the check would predict instead of closing
    R.push_back({"residual divided by mu_k^3", "res = 2 sqrt(sumsq) / (mu_k^3): with a scaled step the partials hold (T - (1.5 mu - 0.5 mu^3) I)^2", 64, 0x1p-44,
                 {{0.5, 2.0, 1.5, {0, 0, 0, 0, 0, 0, 0, 2.0}},
                  {0x1p-45, 2.5, 1.5, {1, 1, 1, 1, 1, 0, 0, 2.5}}}});
    return R;
}

static bool state_matches(const NsState& s, const Expect& e) {
    const bool tr_ok = (e.tr_last != e.tr_last) ? (s.tr_last != s.tr_last) : same_bits(s.tr_last, e.tr_last);
    return s.done == e.done && s.finished == e.finished && s.conv == e.conv && s.final_iter == e.final_iter && s.upd_skip[0] == e.skip0 &&
           s.upd_skip[1] == e.skip1 && s.nonfinite == e.nonfinite && tr_ok;
}

static void section_check() {
    printf("== check: ns_check_block\n");
    const int d = 4, B = 3, nslots = 3, pstride = 5;
    const int64_t stride = 16 + 3;
    for (const Row& row : check_table()) {
        printf("  -- %s   [%s]\n", row.name, row.rule);
        // problem 1 runs the row; problems 0 and 2 hold other data (a finished neighbour and a running one) that must not leak
        std::vector<NsState> st(B);
        for (int b = 0; b < B; ++b) { st[b] = armed_state(1.0); for (size_t k = 0; k < row.steps.size(); ++k) st[b].mu[k] = (b == 1) ? row.steps[k].mu : 1.0; }
        st[0].done = 1; st[0].finished = 1; st[0].conv = 1; st[0].final_iter = 0; st[0].tr_last = 42.0;
        NsState* dst = dupload(st);
        double* dP = dalloc<double>((size_t)B * pstride);
        double* dY = dalloc<double>((size_t)B * stride);
        bool closed = false;
        NsState before1 = st[1];
        for (size_t k = 0; k < row.steps.size() + 2; ++k) {
            const bool extra = k >= row.steps.size();              // two more checks on the closed problem: "already finished"
            const Step& s = row.steps[extra ? row.steps.size() - 1 : k];
            std::vector<double> P((size_t)B * pstride), Y((size_t)B * stride);
            memset(P.data(), 0xEE, P.size() * 8); memset(Y.data(), 0xEE, Y.size() * 8);
            for (int b = 0; b < B; ++b) {
                const double h = (b == 1) ? s.mu * s.mu * s.mu * s.res / 2.0 : 0.75, sq = h * h, tr = (b == 1) ? s.tr : 1.0 + (double)k;
                P[(size_t)b * pstride + 0] = sq / 2; P[(size_t)b * pstride + 1] = sq / 4; P[(size_t)b * pstride + 2] = sq / 4;       // slots 3, 4: poison
                for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) Y[(size_t)b * stride + i * d + j] = (i == j) ? tr / 4 : 1e30 * (i + 1);
            }
            CK(hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice));
            CK(hipMemcpy(dY, Y.data(), Y.size() * 8, hipMemcpyHostToDevice));
            NsCheckArgs a;
            a.k = (int)k; a.max_iter = row.max_iter; a.st_all = dst; a.partials_all = dP; a.nslots = nslots; a.pstride = pstride; a.Yall = dY; a.stride = stride;
            a.d = d; a.tol_res = row.tol_res; a.tol_tr = 1e-13;
            hipLaunchKernelGGL(check_kernel, dim3(B), dim3(256), 0, 0, a);
            dsync();
            const std::vector<NsState> got = d2h(dst, B);
            const std::string tag = std::string("check '") + row.name + "' k=" + std::to_string(k);
            if (!extra) {
                const bool ok = state_matches(got[1], s.e);
                if (!ok) printf("    got done %d finished %d conv %d final_iter %d upd_skip %d %d nonfinite %d tr_last %.17g res[k] %.17g\n", got[1].done, got[1].finished,
                                got[1].conv, got[1].final_iter, got[1].upd_skip[0], got[1].upd_skip[1], got[1].nonfinite, got[1].tr_last, got[1].res[k]);
                report_count(tag + ": state differs from the table", (double)!ok);
                if (!closed) {
                    // the history: this check's residual (bit for bit: dyadic operands) and trace; a closing check of a predicted finish
                    // records the bound it was predicted with
                    const bool predicted_close = k > 0 && row.steps[k - 1].e.done && !row.steps[k - 1].e.finished;
                    const double rp = predicted_close ? row.steps[k - 1].res : 0.0, want_bound = 0.75 * rp * rp + 0.25 * rp * rp * rp;
                    const bool res_ok = predicted_close ? std::fabs(got[1].res[k] - want_bound) <= 4 * U64 * want_bound && same_bits(got[1].res_last, got[1].res[k])
                                                        : same_bits(got[1].res[k], s.res);
                    const bool tr_ok = (s.tr != s.tr) ? (got[1].tr[k] != got[1].tr[k]) : same_bits(got[1].tr[k], s.tr);
                    report_count(tag + ": res[k] / tr[k] not the values handed in", (double)!(res_ok && tr_ok));
                }
                closed = got[1].finished != 0;
            } else {
                // already finished: only the NEXT upd_skip word is written
                NsState want = before1;
                want.upd_skip[(k + 1) & 1] = 1;
                report_count(tag + " (already finished): anything but upd_skip[(k + 1) & 1] = 1 changed", (double)(memcmp(&got[1], &want, sizeof(NsState)) != 0));
            }
            // the neighbours: 0 was finished from the start (only its skip words may be set), 2 runs on its own data
            NsState w0 = st[0]; w0.upd_skip[0] = got[0].upd_skip[0]; w0.upd_skip[1] = got[0].upd_skip[1];
            report_count(tag + ": finished neighbour changed beyond its upd_skip words", (double)(memcmp(&got[0], &w0, sizeof(NsState)) != 0 || got[0].upd_skip[(k + 1) & 1] != 1));
            before1 = got[1];
        }
        report_count(std::string("check '") + row.name + "': the row did not close the problem", (double)!closed);
        free_all();
    }
}

// ================================================================================================ run
struct RunProblem { bool nonfinite; int conv, iters; bool loose; double exact, bound; };
struct RunFile { int d = 0, B = 0; std::vector<RunProblem> pb; std::vector<double> cov1, cov2; bool shared = false; };

static bool read_run_file(const char* path, RunFile& f) {
    FILE* fp = fopen(path, "rb");
    if (!fp) { printf("cannot open %s\n", path); return false; }
    std::vector<double> v;
    double buf[4096]; size_t n;
    while ((n = fread(buf, 8, 4096, fp)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(fp);
    if (v.size() < 3 || v[0] != 20250.0) { printf("%s: not a problem file\n", path); return false; }
    f.d = (int)v[1]; f.B = (int)v[2];
    const size_t dd = (size_t)f.d * f.d, need = 3 + (size_t)f.B * 6 + 2 * (size_t)f.B * dd;
    if (f.d < 1 || f.d > 1024 || f.B < 1 || f.B > 32 || v.size() != need) { printf("%s: bad sizes\n", path); return false; }
    for (int b = 0; b < f.B; ++b) {
        const double* q = &v[3 + (size_t)b * 6];
        f.pb.push_back({q[0] != 0.0, (int)q[1], (int)q[2], q[3] != 0.0, q[4], q[5]});
    }
    f.cov1.assign(v.begin() + 3 + f.B * 6, v.begin() + 3 + f.B * 6 + f.B * dd);
    f.cov2.assign(v.begin() + 3 + f.B * 6 + f.B * dd, v.end());
    f.shared = true;
    for (int b = 1; b < f.B; ++b) if (memcmp(&f.cov1[(size_t)b * dd], &f.cov1[0], dd * 8) != 0) f.shared = false;
    return true;
}

struct RunResult { std::vector<NsState> st; };
enum RunMode { PLAIN, SHARED, REUSE };

// one call of run_ns on problems [b0, b0 + n) of the file
static RunResult run_once(const RunFile& f, int b0, int n, RunMode mode, int first_chunk, Workspace& ws, const double* dc1, const double* dc2, const double* dmu) {
    const int d = f.d;
    const int64_t dd = (int64_t)d * d;
    if (ws.small.reserve(ns_small_bytes(d, n)) != FAD_OK) { printf("%s\n", err_buf()); exit(2); }
    CK(hipMemset(ws.small.p, 0xEE, ns_small_bytes(d, n)));
    NsState* dstates = static_cast<NsState*>(ws.small.p);
    enqueue_clear_states(dstates, n, 0);
    NsProblem pb{d, n, dc1 + (mode == SHARED ? 0 : b0 * dd), mode == SHARED ? 0 : dd, dc2 + b0 * dd, dd, dmu, 0, dmu, 0, -1};
    if (mode == REUSE) {
        // what the low-precision attempt leaves behind: A = C1 C2 in the first matrix of ws.mats, its statistics, the armed state
        if (ws.mats.reserve((size_t)(6 * dd * n) * sizeof(double)) != FAD_OK) { printf("%s\n", err_buf()); exit(2); }
        double* A = static_cast<double*>(ws.mats.p);
        double* tilestats = reinterpret_cast<double*>(dstates + n) + (size_t)n * ns_pstride(d);
        GemmType g{pb.cov1, pb.s_cov1, pb.cov2, pb.s_cov2, A, dd, 1.0, 0.0, 0.0, nullptr};
        if (gemm_f64_launch(d, &g, 1, n, &dstates[0].done, kStateInts, 0, 0) < 0) { printf("%s\n", err_buf()); exit(2); }
        const unsigned nb = (unsigned)stat_blocks(d);
        hipLaunchKernelGGL(ns_tilestats, dim3(nb, nb, (unsigned)n), dim3(256), 0, 0, A, d, pb.cov1, pb.s_cov1, pb.cov2, pb.s_cov2, tilestats, dstates);
        hipLaunchKernelGGL(ns_prepare, dim3((unsigned)n), dim3(256), 0, 0, tilestats, d, (int)nb, pb.mu1, pb.s_mu1, pb.mu2, pb.s_mu2, -1, dstates, 0, (Ns32State*)nullptr, 1);
    }
    NsState* hs = nullptr;
    const int rc = run_ns(pb, 0, 0.0, 0, 0, ws, &hs, mode == REUSE, nullptr, first_chunk);
    if (rc != FAD_OK) { printf("run_ns failed: %s\n", err_buf()); exit(2); }
    dsync();
    RunResult r; r.st.assign(hs, hs + n);
    return r;
}

static void check_against_file(const std::string& tag, const RunFile& f, int b, const NsState& s) {
    const RunProblem& p = f.pb[b];
    if (p.nonfinite) { report_count(tag + ": nonfinite / finished not set", (double)!(s.nonfinite == 1 && s.finished == 1)); return; }
    report_count(tag + ": stop code " + std::to_string(s.conv) + ", the emulation's " + std::to_string(p.conv), (double)(s.conv != p.conv || s.nonfinite != 0 || s.finished != 1));
    report_count(tag + ": " + std::to_string(s.final_iter + 1) + " iterations, the emulation's " + std::to_string(p.iters) + (p.loose ? " (may differ by one)" : ""),
                 (double)(std::abs(s.final_iter + 1 - p.iters) > (p.loose ? 1 : 0)));
    const double v = std::sqrt(s.c) * s.tr_last;
    if (p.bound > 0) report_ratio(tag + " sqrt(c) tr_last against the eigenvalue value", std::fabs(v - p.exact) / p.bound);
    else report_count(tag + ": value not exactly " + std::to_string(p.exact), (double)(v != p.exact));
}
static double state_diffs(const NsState& a, const NsState& b) {
    return (double)!(a.conv == b.conv && a.final_iter == b.final_iter && a.nonfinite == b.nonfinite && a.finished == b.finished &&
                     (a.nonfinite || (same_bits(a.tr_last, b.tr_last) && same_bits(a.c, b.c))));
}

static void section_run(const char* path) {
    printf("== run: run_ns on %s\n", path);
    RunFile f;
    if (!read_run_file(path, f)) { ++g_fail; return; }
    const int d = f.d, B = f.B;
    std::vector<double> zero(d, 0.0);
    const double *dc1 = dupload(f.cov1), *dc2 = dupload(f.cov2), *dmu = dupload(zero);
    static Pool pool;                                  // the thread's history of single-pair calls (f64_iters)
    Workspace& ws = pool.slot[0];
    ws.pool = &pool;
    const std::string head = "run d=" + std::to_string(d) + " B=" + std::to_string(B);
    const RunResult batch = run_once(f, 0, B, PLAIN, 0, ws, dc1, dc2, dmu);
    for (int b = 0; b < B; ++b) {
        const NsState& s = batch.st[b];
        printf("    problem %d: c %.6e conv %d final_iter %d nonfinite %d\n      res:", b, s.c, s.conv, s.final_iter, s.nonfinite);
        for (int k = 0; k <= s.final_iter && k < kMaxIter; ++k) printf(" %.3e", s.res[k]);
        printf("\n      tr: ");
        for (int k = 0; k <= s.final_iter && k < kMaxIter; ++k) printf(" %.15g", s.tr[k]);
        printf("\n");
        check_against_file(head + " batch, problem " + std::to_string(b), f, b, s);
    }
    if (f.shared) {
        const RunResult sh = run_once(f, 0, B, SHARED, 0, ws, dc1, dc2, dmu);
        for (int b = 0; b < B; ++b) report_count(head + " shared first covariance (stride 0), problem " + std::to_string(b) + ": differs from the strided batch", state_diffs(sh.st[b], batch.st[b]));
    }
    for (int chunk : {1, 2, 4, 7, 8}) {          // (4 and 8 end a chunk on check 7 and 3: where a 9- and a 5-iteration problem predict their finish)
        const RunResult r = run_once(f, 0, B, PLAIN, chunk, ws, dc1, dc2, dmu);
        for (int b = 0; b < B; ++b) report_count(head + " first_chunk=" + std::to_string(chunk) + ", problem " + std::to_string(b) + ": differs from the default chunking", state_diffs(r.st[b], batch.st[b]));
    }
    {
        const RunResult r = run_once(f, 0, B, REUSE, 0, ws, dc1, dc2, dmu);
        for (int b = 0; b < B; ++b) report_count(head + " reuse_prepared, problem " + std::to_string(b) + ": differs from the batch", state_diffs(r.st[b], batch.st[b]));
    }
    // every problem alone (B = 1 sizes its first chunk by what the previous one needed), forwards and backwards
    std::vector<NsState> single(B);
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < B; ++i) {
            const int b = pass ? B - 1 - i : i;
            const RunResult r = run_once(f, b, 1, PLAIN, 0, ws, dc1, dc2, dmu);
            const std::string tag = head + " alone, problem " + std::to_string(b) + (pass ? " (reverse order)" : "");
            if (!pass) {
                single[b] = r.st[0];
                check_against_file(tag, f, b, r.st[0]);
                const RunProblem& p = f.pb[b];
                // (another batch size may pick another GEMM tile: the same codes, the value within the same tolerance)
                const bool codes = r.st[0].conv == batch.st[b].conv && r.st[0].nonfinite == batch.st[b].nonfinite &&
                                   std::abs(r.st[0].final_iter - batch.st[b].final_iter) <= (p.loose ? 1 : 0);
                report_count(tag + ": codes differ from the batch's", (double)!codes);
                if (!p.nonfinite && p.bound > 0)
                    report_ratio(tag + " against the batch's value", std::fabs(std::sqrt(r.st[0].c) * r.st[0].tr_last - std::sqrt(batch.st[b].c) * batch.st[b].tr_last) / p.bound);
            } else {
                report_count(tag + ": differs from the same problem after another predecessor", state_diffs(r.st[0], single[b]));
            }
        }
    pool.release_all();
    ws.pool = nullptr;
    free_all();
}

int main(int argc, char** argv) {
    int dev_count = 0;
    CK(hipGetDeviceCount(&dev_count));
    CK(hipSetDevice(0));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    g_num_cus = prop.multiProcessorCount;
    printf("device: %s, %d CUs\n", prop.gcnArchName, g_num_cus);
    bool any = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        any = true;
        if (a == "stats") section_stats(true, false);
        else if (a == "schedule") section_stats(false, true);
        else if (a == "first") section_first();
        else if (a == "check") section_check();
        else if (a == "run") { if (i + 1 >= argc) { printf("run needs a problem file\n"); return 1; } section_run(argv[++i]); }
        else { printf("unknown section %s\n", a.c_str()); return 1; }
    }
    if (!any) { section_stats(true, false); section_stats(false, true); section_first(); section_check(); }
    printf("%d checks, %d failed, largest err / bound %.3f\n", g_checks, g_fail, g_max_ratio);
    if (g_fail) { printf("FAILED\n"); return 1; }
    printf("all checks passed\n");
    return 0;
}
