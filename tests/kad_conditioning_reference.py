"""Inputs and host references for the conditioning tests of the KAD family (test plumbing, not product; numpy and scipy only).

The kernels of csrc/kad.hip start a float32 accumulator at h_i + h_j = -(|x_i|^2 + |y_j|^2) / 2 and add the dot product on the MFMAs, so
the rounding error of d^2 scales with |x|^2 + |y|^2, not with d^2: what decides the accuracy of a kernel value is
kappa = (|x|^2 + |y|^2) / (2 sigma^2).  This module makes rows with a large kappa and says what float32 allows there:

  offset_int_rows   integer rows far from the origin, for which every float32 quantity of the kernels is exact in any summation order;
  offset_gauss      the Gaussian sets of test_gpu_kad.py moved by a common offset;
  pow2_rows         Gaussian values on a grid of 2^-3, exact in fp16, bf16 and fp32, to be scaled by powers of two;
  kappa             the label and the scale of the tolerances;
  bracket_means     float64 lower and upper values of the kernel means when every d^2 may be off by tau (|a|^2 + |b|^2): a hard bound;
  chain32_means     a float32 emulation of the documented chain, vectorised over all pairs: what float32 costs at that kappa;
  conditioning_constant   A = max over the Gaussian cases of (chain32 error of a mean / that mean) / kappa, per dtype."""
import functools

import numpy as np
from scipy.spatial.distance import cdist, pdist

TAU = 1.3e-5                       # the float32 d^2 margin of test_gpu_prdc.py / DESIGN.md 4.8, relative to |a|^2 + |b|^2
MEANS = ("kxx_mean", "kyy_mean", "kxy_mean")
STEP = {"fp16": 16, "bf16": 16, "fp32": 2}          # K of the MFMA instructions of chunk_mfma

EXACT_SHAPES = [(127, 128, 17), (129, 300, 128), (300, 129, 1024), (130, 129, 1280)]          # n, m, d
EXACT_CASES = [(n, m, d, 40) for n, m, d in EXACT_SHAPES] + [(127, 128, 17, 200)]              # n, m, d, off
GAUSS_CASES = [(d, off) for off in (4, 16) for d in (17, 128, 512)]                            # n = 255, m = 257
GAUSS_N, GAUSS_M = 255, 257
SONG_CUTS = (0, 1, 3, 130, 257)                     # the second Gaussian set cut into songs of 1, 2, 127 and 127 rows
PRDC_OFFSET = 2
PRDC_CASES = [(1100, 900, 128, 5), (777, 1301, 512, 3)]                                        # n, m, d, k
PRDC_CAP = 0.02                    # widest bracket of each of the four PRDC values at PRDC_OFFSET (0.005 at offset 0)
SCALES = [("fp16", -14), ("fp16", 9), ("bf16", -40), ("bf16", 40), ("fp32", -50), ("fp32", 50)]   # (dtype, e): rows scaled by 2^e
OVERFLOW_EXP, UNDERFLOW_EXP = 70, -80              # |x|^2 overflows / underflows float32 at these scales


# ------------------------------------------------------------------------------------------------------------------- dtypes
def round_to(a, dt):
    """a (float32 values) rounded to fp16 / bf16 / fp32 and returned as float32 (bf16: round to nearest even on the upper 16 bits)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == "fp16":
        return a.astype(np.float16).astype(np.float32)
    if dt == "bf16":
        u = a.view(np.uint32)
        return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    assert dt == "fp32", dt
    return a


# --------------------------------------------------------------------------------------------------------------------- rows
def exact_condition(d, off):
    """True when integer rows in [-3, 3] + off of length d keep every float32 quantity of the kernels exact: the values are exact in
    bf16 (off + 3 <= 256), and |x|^2 <= 2^22, so that the norms, h = -|x|^2 / 2 (half-integers), h_i + h_j and every partial sum of the
    chain are half-integers below 2^23 in magnitude."""
    return off + 3 <= 256 and d * (off + 3) ** 2 <= 2 ** 22


def offset_int_rows(rng, n, d, off, dups):
    """Integer rows in [-3, 3] + off (float32) with row j a copy of row i for every (i, j) of dups, as _int_rows of test_gpu_prdc.py."""
    assert exact_condition(d, off), (d, off)
    a = (rng.integers(-3, 4, size=(n, d)) + off).astype(np.float32)
    for i, j in dups:
        if i < n and j < n:
            a[j] = a[i]
    return a


def exact_sets(n, m, d, off):
    """The two sets of an exact case: duplicates inside each set and one y row on top of an x row."""
    rng = np.random.default_rng(n * 7 + m * 3 + d + off)
    x = offset_int_rows(rng, n, d, off, [(0, 1), (3, n - 1), (2, n // 2)])
    y = offset_int_rows(rng, m, d, off, [(1, 0), (4, m - 2)])
    y[5] = x[4]
    return x, y


def offset_gauss(n, m, d, off, seed, shift):
    """The _sets rows of test_gpu_kad.py (float32) with off added to every element of both sets."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * (1.0 + 0.1 * shift) + 0.3 * shift).astype(np.float32)
    return x + np.float32(off), y + np.float32(off)


def gauss_sets(d, off, dt):
    """The Gaussian case (d, off) in dtype dt, as float32 values."""
    x, y = offset_gauss(GAUSS_N, GAUSS_M, d, off, seed=d + off, shift=1)
    return round_to(x, dt), round_to(y, dt)


def prdc_gauss(n, m, d, seed):
    """_gauss of test_gpu_prdc.py: y scaled and shifted by amounts that shrink with D, so the sets overlap about as much at every D."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * (1.0 + 0.1 * (128 / d) ** 0.5) + 0.05 * (128 / d) ** 0.25).astype(np.float32)
    return x, y


def pow2_rows(n, m, d, seed):
    """Gaussian values rounded to multiples of 2^-3 and clipped to |v| <= 8 (7 significant bits: exact in fp16, bf16 and fp32)."""
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(rng.standard_normal((n, d)) * 8.0) / 8.0, -8.0, 8.0).astype(np.float32)
    y = np.clip(np.round((rng.standard_normal((m, d)) * 1.1 + 0.3) * 8.0) / 8.0, -8.0, 8.0).astype(np.float32)
    return x, y


# ---------------------------------------------------------------------------------------------------------------- float64
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def kappa(x, y, sigma):
    """The mean over the x-x pairs of (|a|^2 + |b|^2) / (2 sigma^2), which is mean |x_i|^2 / sigma^2 (y: the other set of the case,
    not used: one kappa labels a case)."""
    x = _f64(x)
    return float((x * x).sum(1).mean() / (sigma * sigma))


def max_pair_norms(x):
    """max over the pairs i != j of |x_i|^2 + |x_j|^2"""
    s = np.sort((_f64(x) ** 2).sum(1))
    return float(s[-1] + s[-2])


def _mean_of(k, same):
    if same:
        k = k.copy()
        np.fill_diagonal(k, 0.0)
        n = k.shape[0]
        return float(k.sum() / (n * (n - 1)))
    return float(k.mean())


def _pairs(x, y):
    return (("kxx_mean", x, x, True), ("kyy_mean", y, y, True), ("kxy_mean", x, y, False))


def means64(x, y, sigma):
    """The float64 kernel means and MMD^2 (kad_reference.kad at a given sigma)."""
    x, y = _f64(x), _f64(y)
    out = {name: _mean_of(np.exp(-cdist(a, b, "sqeuclidean") / (2.0 * sigma * sigma)), same) for name, a, b, same in _pairs(x, y)}
    out["mmd2"] = out["kxx_mean"] + out["kyy_mean"] - 2.0 * out["kxy_mean"]
    return out


def bracket_means(x, y, sigma, tau):
    """-> {name: (lo, hi)} for kxx_mean, kyy_mean, kxy_mean and mmd2 in float64, every pair's d^2 moved by -+ tau (|a|^2 + |b|^2) and
    clamped at 0.  No kernel whose float32 d^2 is within tau of float64 can leave it."""
    x, y = _f64(x), _f64(y)
    g = 1.0 / (2.0 * sigma * sigma)
    out = {}
    for name, a, b, same in _pairs(x, y):
        d2 = cdist(a, b, "sqeuclidean")
        e = tau * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])
        out[name] = (_mean_of(np.exp(-g * (d2 + e)), same), _mean_of(np.exp(-g * np.maximum(d2 - e, 0.0)), same))
    out["mmd2"] = (out["kxx_mean"][0] + out["kyy_mean"][0] - 2.0 * out["kxy_mean"][1],
                   out["kxx_mean"][1] + out["kyy_mean"][1] - 2.0 * out["kxy_mean"][0])
    return out


def inside(value, lo_hi):
    """lo <= value <= hi, with the slack of a float64 sum taken in another order (1e-13 relative)."""
    lo, hi = lo_hi
    slack = 1e-13 * max(abs(lo), abs(hi))
    return lo - slack <= value <= hi + slack


# ------------------------------------------------------------------------------------------------------ the float32 chain
def h32(a):
    """h = -|row|^2 / 2 as kad_pack_kernel sums it: lane l takes the columns l, l + 64, ... with one fused multiply-add each, then
    the 64 lanes meet in a butterfly (xor 32, 16, ..., 1), everything rounded to float32."""
    a = _f64(a)
    n, d = a.shape
    dp = -(-d // 64) * 64
    pad = np.zeros((n, dp))
    pad[:, :d] = a
    s = np.zeros((n, 64), dtype=np.float32)
    for c in range(0, dp, 64):
        s = (pad[:, c:c + 64] ** 2 + s.astype(np.float64)).astype(np.float32)        # fmaf: one rounding
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lanes ^ off]).astype(np.float32)
    return (np.float32(-0.5) * s[:, 0]).astype(np.float32)


def _column_order(d, step):
    """The order in which chunk_mfma feeds the columns: consecutive blocks of 16 for the 16-bit MFMAs; for float32 rows the step e of
    a group of 8 columns takes the columns e and e + 4 (lane half h holds k = 8 q + 4 h + e)."""
    cols = np.arange(-(-d // 8) * 8)
    if step == 2:
        cols = cols.reshape(-1, 2, 4).transpose(0, 2, 1).reshape(-1)
    return cols


def chain32_acc(a, b, step):
    """The accumulator of every pair at the end of the chain, float32 [n, m]: acc = fl32(h_i + h_j), then acc = fl32(acc + block dot)
    for the blocks of `step` columns in the kernel's order, each block dot taken in float64 and rounded once."""
    a, b = _f64(a), _f64(b)
    d = a.shape[1]
    cols = _column_order(d, step)
    pa = np.zeros((a.shape[0], cols.size))
    pb = np.zeros((b.shape[0], cols.size))
    pa[:, :d], pb[:, :d] = a, b
    pa, pb = pa[:, cols], pb[:, cols]
    acc = (h32(a)[:, None] + h32(b)[None, :]).astype(np.float32)
    for c in range(0, cols.size, step):
        acc = (acc.astype(np.float64) + pa[:, c:c + step] @ pb[:, c:c + step].T).astype(np.float32)
    return acc


def chain32_d2(a, b, step):
    """d^2 = -2 acc of the float32 chain, as float64 (not clamped)."""
    return -2.0 * chain32_acc(a, b, step).astype(np.float64)


def chain32_means(x, y, sigma, step):
    """The kernel means and MMD^2 from the float32 chain, k = exp(min(acc, 0) / sigma^2) and the sums in float64."""
    out = {name: _mean_of(np.exp(np.minimum(chain32_acc(a, b, step).astype(np.float64), 0.0) / (sigma * sigma)), same)
           for name, a, b, same in _pairs(x, y)}
    out["mmd2"] = out["kxx_mean"] + out["kyy_mean"] - 2.0 * out["kxy_mean"]
    return out


def mean_errors(got, want):
    """Relative error of each mean, and of mmd2 against the scale kxx + kyy + 2 kxy."""
    err = {k: abs(got[k] - want[k]) / abs(want[k]) for k in MEANS}
    err["mmd2"] = abs(got["mmd2"] - want["mmd2"]) / (want["kxx_mean"] + want["kyy_mean"] + 2.0 * want["kxy_mean"])
    return err


@functools.lru_cache(maxsize=None)
def gauss_case(d, off, dt):
    """Everything the host and GPU tests need of one Gaussian case, computed once: the rows (float32 values of dtype dt), the float64
    median distance sigma, kappa, the float64 means, the chain32 means and their errors, and the bracket at TAU."""
    x, y = gauss_sets(d, off, dt)
    sigma = float(np.median(pdist(_f64(x))))
    want = means64(x, y, sigma)
    chain = chain32_means(x, y, sigma, STEP[dt])
    return {"x": x, "y": y, "sigma": sigma, "kappa": kappa(x, y, sigma), "want": want, "chain": chain,
            "chain_err": mean_errors(chain, want), "bracket": bracket_means(x, y, sigma, TAU)}


@functools.lru_cache(maxsize=None)
def song_case(d, off, dt):
    """The songs of a Gaussian case (y cut at SONG_CUTS) against its x: per song of two rows or more the float64 means, the chain32
    errors and the bracket at TAU."""
    c = gauss_case(d, off, dt)
    out = []
    for s in range(len(SONG_CUTS) - 1):
        ys = c["y"][SONG_CUTS[s]:SONG_CUTS[s + 1]]
        if len(ys) < 2:
            out.append(None)
            continue
        want = means64(c["x"], ys, c["sigma"])
        out.append({"want": want, "chain_err": mean_errors(chain32_means(c["x"], ys, c["sigma"], STEP[dt]), want),
                    "bracket": bracket_means(c["x"], ys, c["sigma"], TAU)})
    return out


@functools.lru_cache(maxsize=None)
def conditioning_constant(dt):
    """A = max over the Gaussian cases of (chain32 error of a mean / that mean) / kappa: the reference's own estimate of what the
    float32 chain costs per unit of kappa, for rows of dtype dt."""
    return max(max(gauss_case(d, off, dt)["chain_err"][k] for k in MEANS) / gauss_case(d, off, dt)["kappa"] for d, off in GAUSS_CASES)


def song_chain_constant(dt, s):
    """max over the Gaussian cases of (chain32 error of song s's Kyy or Kxy / that mean) / kappa"""
    return max(max(song_case(d, off, dt)[s]["chain_err"][k] for k in ("kyy_mean", "kxy_mean")) / gauss_case(d, off, dt)["kappa"]
               for d, off in GAUSS_CASES)


@functools.lru_cache(maxsize=None)
def song_constants(dt):
    """The constant that bounds each song of SONG_CUTS: None for the song of one row (no Kyy); the set-level A for every song whose Kyy
    is an average over many pairs; for the song of two rows alone, song_chain_constant.  Its Kyy is one pair, whose float32 error no
    average reduces, and chain32 itself leaves MEAN_RTOL + 4 A kappa there (fp16, d = 512, offset 16: 2.8e-5 against 1.6e-5), so the
    set-level A cannot be asked of a correct kernel on that song."""
    out = []
    for s in range(len(SONG_CUTS) - 1):
        rows = SONG_CUTS[s + 1] - SONG_CUTS[s]
        out.append(None if rows < 2 else song_chain_constant(dt, s) if rows == 2 else conditioning_constant(dt))
    return tuple(out)
