"""float64 numpy reference of the polynomial-kernel distance (fad_kid, fad_kid_subsets), for the KID tests (test
plumbing, not product), on the same 16-bit / float32 values the kernels read, upcast:

  k(a, b) = (gamma a.b + coef0)^degree, gamma and coef0 as their float32 roundings (gamma None: fl32(1 / D)), as the library uses them
  Sxx, Syy over i != j; Sxy over every pair (its diagonal included in a subset);  means = S / (n (n - 1)), S / (n m)
  MMD^2 = Kxx + Kyy - 2 Kxy

kid_full and kid_subsets are that definition.  chain32_poly_means is a host emulation of the kernels' float32 chain: the accumulator
starts at 0 and takes one rounding per MFMA K block in chunk_mfma's column order (kad_conditioning_reference._column_order), the epilogue is
a float32 fma and degree - 1 float32 multiplies, every lane sums its 64 values of a 128 x 128 tile in float32 in the kernels' order
(bi, bj, g), and everything from there is float64.  A_poly (poly_constant) is what that chain costs, per dtype, at the shapes of the GPU
cases: the GPU tolerances are built from it."""
import functools

import numpy as np

import kad_conditioning_reference as CR

MEANS = ("kxx_mean", "kyy_mean", "kxy_mean")
STEP = CR.STEP
DTYPES = ("fp16", "bf16", "fp32")

# the Gaussian GPU cases: n = 255, m = 257 (two row blocks with a ragged edge each), every D x offset x degree
GAUSS_N, GAUSS_M = 255, 257
GAUSS_CASES = [(d, off, degree) for d in (1, 17, 128, 512) for off in (0, 4) for degree in (2, 3)]
MEAN_FLOOR = 4e-7                   # the floor of the GPU tolerance, relative to mean |k| of the block (MEAN_RTOL of the Gaussian kernel)

# the exact GPU cases: rows in {-1, 0, 1}, D = 16, gamma = 1 / 16, coef0 = 1, degree 3
EXACT_N, EXACT_M, EXACT_D, EXACT_LD = 301, 333, 16, 24
EXACT_SIZES = (2, 127, 128, 129, 300)
EXACT_SUBSETS = (1, 3, 17)
EXACT_FULL = ((2, 3), (255, 257))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def params32(d, gamma=None, coef0=1.0):
    """(gamma, coef0) as float64 values of the float32 numbers the library uses"""
    g = np.float32(1.0 / d) if gamma is None or gamma <= 0 else np.float32(gamma)
    return float(g), float(np.float32(coef0))


def kmat(a, b, degree, gamma, coef0):
    return (gamma * (_f64(a) @ _f64(b).T) + coef0) ** degree


def _block(a, b, same, degree, gamma, coef0):
    """-> (sum of k, sum of |k|, pairs) over i != j (same) or over every pair"""
    k = kmat(a, b, degree, gamma, coef0)
    if same:
        k = k.copy()
        np.fill_diagonal(k, 0.0)
        return float(k.sum()), float(np.abs(k).sum()), k.shape[0] * (k.shape[0] - 1)
    return float(k.sum()), float(np.abs(k).sum()), k.shape[0] * k.shape[1]


def kid_full(x, y, degree=3, gamma=None, coef0=1.0):
    """-> dict: the three means, mmd2, the three sums (sxx, syy, sxy), the means of |k| per block (abs_*) and gamma, coef0 as used"""
    g, c = params32(np.shape(x)[1], gamma, coef0)
    out = {"gamma": g, "coef0": c, "degree": degree}
    for name, a, b, same in CR._pairs(x, y):
        s, sa, cnt = _block(a, b, same, degree, g, c)
        out[name] = s / cnt
        out["s" + name[1:3]] = s
        out["abs_" + name] = sa / cnt
    out["mmd2"] = out["kxx_mean"] + out["kyy_mean"] - 2.0 * out["kxy_mean"]
    return out


def kid_subsets(x, y, index_x, index_y, degree=3, gamma=None, coef0=1.0):
    """-> float64 [S, 3]: Sxx, Syy (i != j) and Sxy (all s^2 pairs) of subset q = (x[index_x[q]], y[index_y[q]])"""
    x, y = _f64(x), _f64(y)
    index_x, index_y = np.asarray(index_x), np.asarray(index_y)
    out = np.zeros((index_x.shape[0], 3))
    for q in range(index_x.shape[0]):
        r = kid_full(x[index_x[q]], y[index_y[q]], degree, gamma, coef0)
        out[q] = r["sxx"], r["syy"], r["sxy"]
    return out


def subset_stats(sums, s):
    """sums [S, 3] -> (terms [S, 3] the three means, mmd2 [S], mean, population std), as fad_kid_subsets forms them"""
    sums = _f64(sums)
    terms = np.stack([sums[:, 0] / (s * (s - 1.0)), sums[:, 1] / (s * (s - 1.0)), sums[:, 2] / (float(s) * float(s))], axis=1)
    mmd2 = terms[:, 0] + terms[:, 1] - 2.0 * terms[:, 2]
    return terms, mmd2, float(mmd2.mean()), float(mmd2.std())


# ------------------------------------------------------------------------------------------------- the float32 emulation
def chain32_dot(a, b, step):
    """The accumulator of every pair at the end of the MFMA chain, float32 [n, m]: 0, then acc = fl32(acc + block dot) for the blocks
    of `step` columns in the kernel's order, each block dot taken in float64 and rounded once (CR.chain32_acc without h)."""
    a, b = _f64(a), _f64(b)
    d = a.shape[1]
    cols = CR._column_order(d, step)
    pa, pb = np.zeros((a.shape[0], cols.size)), np.zeros((b.shape[0], cols.size))
    pa[:, :d], pb[:, :d] = a, b
    pa, pb = pa[:, cols], pb[:, cols]
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for c in range(0, cols.size, step):
        acc = (acc.astype(np.float64) + pa[:, c:c + step] @ pb[:, c:c + step].T).astype(np.float32)
    return acc


def epilogue32_poly(acc, degree, gamma, coef0):
    """u = fl32(fma(acc, gamma, coef0)) -- the product is exact in float64, one rounding -- and k = u^degree by degree - 1 float32
    multiplies -> float32"""
    u = (np.asarray(acc, dtype=np.float32).astype(np.float64) * gamma + coef0).astype(np.float32)
    k = u
    for _ in range(degree - 1):
        k = (k * u).astype(np.float32)
    return k


def lane_sums32(k):
    """The float64 sum of a float32 matrix of kernel values (dropped pairs already 0) taken as the kernels take it: every lane of every
    wave adds its 64 values of a 128 x 128 tile in float32 in the order (bi, bj, g) -- rows bi * 32 + (g & 3) + 8 (g >> 2) + 4 (lane >> 5)
    and column bj * 32 + (lane & 31) of the wave's 64 x 64 -- and the lanes' sums meet in float64."""
    k = np.asarray(k, dtype=np.float32)
    R, Cn = -(-k.shape[0] // 64) * 64, -(-k.shape[1] // 64) * 64
    pad = np.zeros((R, Cn), dtype=np.float32)
    pad[:k.shape[0], :k.shape[1]] = k
    w = pad.reshape(R // 64, 64, Cn // 64, 64)
    s = np.zeros((R // 64, 2, Cn // 64, 32), dtype=np.float32)
    for bi in range(2):
        for bj in range(2):
            for g in range(16):
                r = bi * 32 + (g & 3) + 8 * (g >> 2)
                s = s + w[:, [r, r + 4], :, bj * 32:bj * 32 + 32]              # float32 + float32: one rounding
    return float(s.astype(np.float64).sum())


def chain32_poly_means(x, y, step, degree=3, gamma=None, coef0=1.0):
    """The three means and MMD^2 from the float32 chain: chain32_dot, epilogue32_poly, lane_sums32 (the triangles as the kernels walk
    them: the pairs j > i, twice), float64 from there."""
    g, c = params32(np.shape(x)[1], gamma, coef0)
    out = {}
    for name, a, b, same in CR._pairs(x, y):
        k = epilogue32_poly(chain32_dot(a, b, step), degree, g, c)
        if same:
            n = k.shape[0]
            out[name] = 2.0 * lane_sums32(np.triu(k, 1)) / (n * (n - 1.0))
        else:
            out[name] = lane_sums32(k) / (float(k.shape[0]) * k.shape[1])
    out["mmd2"] = out["kxx_mean"] + out["kyy_mean"] - 2.0 * out["kxy_mean"]
    return out


def mean_errors(got, want):
    """Error of each mean relative to the mean of |k| over its block, and of mmd2 relative to |Kxx| + |Kyy| + 2 |Kxy| (means of |k|)."""
    err = {k: abs(got[k] - want[k]) / want["abs_" + k] for k in MEANS}
    err["mmd2"] = abs(got["mmd2"] - want["mmd2"]) / (want["abs_kxx_mean"] + want["abs_kyy_mean"] + 2.0 * want["abs_kxy_mean"])
    return err


def gauss_rows(d, off, dt):
    """The rows of the Gaussian case (d, off) in dtype dt, as float32 values: CR.offset_gauss (zero-mean rows, or all elements moved by
    off: post-ReLU-like), rounded to dt."""
    x, y = CR.offset_gauss(GAUSS_N, GAUSS_M, d, off, seed=1000 + d + off, shift=1)
    return CR.round_to(x, dt), CR.round_to(y, dt)


@functools.lru_cache(maxsize=None)
def gauss_case(d, off, degree, dt):
    """One Gaussian case, computed once: the rows, the float64 reference, the chain32 means and their errors."""
    x, y = gauss_rows(d, off, dt)
    want = kid_full(x, y, degree)
    chain = chain32_poly_means(x, y, STEP[dt], degree)
    return {"x": x, "y": y, "want": want, "chain": chain, "chain_err": mean_errors(chain, want)}


@functools.lru_cache(maxsize=None)
def poly_constant(dt):
    """A_poly: the worst error of a chain32 mean over the mean of |k| of its block, over the Gaussian cases, for rows of dtype dt."""
    return max(max(gauss_case(d, off, degree, dt)["chain_err"][k] for k in MEANS) for d, off, degree in GAUSS_CASES)


def gpu_tolerance(dt):
    """max(4e-7, 4 A_poly): the GPU bound on a mean, relative to mean |k| of its block; the factor 4 over the emulation is the margin
    DESIGN.md 4.6 uses for the same chain."""
    return max(MEAN_FLOOR, 4.0 * poly_constant(dt))


# ------------------------------------------------------------------------------------------------------ the exact fixture
def exact_rows(n=EXACT_N, m=EXACT_M, d=EXACT_D, seed=16):
    """Rows in {-1, 0, 1} (float32; exact in every dtype).  With gamma = 1 / 16 and coef0 = 1 at D = 16, u = 1 + S / 16 is a multiple of
    2^-4 in [0, 2] and u^3 a multiple of 2^-12 in [0, 8]: 64 of them sum exactly in float32, and every float64 sum is exact."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-1, 2, size=(n, d)).astype(np.float32), rng.integers(-1, 2, size=(m, d)).astype(np.float32))


def exact_indices(n, m, subsets, s, seed):
    """subsets x s row numbers without repeats inside a subset, int32, for x and for y"""
    rng = np.random.default_rng(seed)
    ix = np.stack([rng.choice(n, s, replace=False) for _ in range(subsets)]).astype(np.int32)
    iy = np.stack([rng.choice(m, s, replace=False) for _ in range(subsets)]).astype(np.int32)
    return ix, iy
