"""float64 numpy reference of the KAD family with a kernel argument, for the kernel tests (test plumbing, not product).

With t = |a - b|^2 / (2 sigma^2), one bandwidth convention for the three kernels (gamma = 1 / (2 sigma^2), no eps):

  gaussian  k = exp(-t)            iq  k = 1 / (1 + t)            imq  k = 1 / sqrt(1 + t)

and everything else as the Gaussian references state it: the set-level means and MMD^2 of kad_reference.py, the per-song form (one
sigma, the baseline's Kxx), the uncertainty definitions of kad_uncertainty_reference.py and the permutation statistics of
kad_permutation_reference.py.  chain32_means is the float32 emulation of kad_conditioning_reference.py with the kernels' epilogue:
u = fl32(fma(acc, -c, 1)), w = max(u, 1), k = fl32(1 / w) or fl32(1 / sqrt(w)), c = fl32(1 / sigma^2)."""
import numpy as np
from scipy.spatial.distance import cdist, pdist

import kad_conditioning_reference as CR

KERNELS = ("gaussian", "iq", "imq")


def kernel_of_t(t, kernel):
    """k(t) in float64, t = d^2 / (2 sigma^2) >= 0"""
    t = np.asarray(t, dtype=np.float64)
    if kernel == "gaussian":
        return np.exp(-t)
    if kernel == "iq":
        return 1.0 / (1.0 + t)
    if kernel == "imq":
        return 1.0 / np.sqrt(1.0 + t)
    raise ValueError(f"unknown kernel {kernel!r}")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def kmat(a, b, sigma, kernel):
    return kernel_of_t(cdist(_f64(a), _f64(b), "sqeuclidean") / (2.0 * sigma * sigma), kernel)


def _mean(k, same):
    if same:
        k = k.copy()
        np.fill_diagonal(k, 0.0)
        n = k.shape[0]
        return float(k.sum() / (n * (n - 1)))
    return float(k.sum() / (k.shape[0] * k.shape[1]))


def median_distance(x):
    return float(np.median(pdist(_f64(x))))


# ------------------------------------------------------------------------------------------------------------- set level
def kad(x, y, sigma=None, kernel="gaussian"):
    x, y = _f64(x), _f64(y)
    if sigma is None:
        sigma = median_distance(x)
    kxx, kyy, kxy = _mean(kmat(x, x, sigma, kernel), True), _mean(kmat(y, y, sigma, kernel), True), _mean(kmat(x, y, sigma, kernel), False)
    return {"mmd2": kxx + kyy - 2.0 * kxy, "kxx_mean": kxx, "kyy_mean": kyy, "kxy_mean": kxy, "bandwidth": sigma}


# -------------------------------------------------------------------------------------------------------------- per song
def kad_individual(x, songs, sigma=None, kernel="gaussian"):
    """-> (kxx_mean, sigma, list per song: None for a song of fewer than 2 rows, else its kad dict with the baseline's kxx)"""
    x = _f64(x)
    if sigma is None:
        sigma = median_distance(x)
    kxx = _mean(kmat(x, x, sigma, kernel), True)
    out = []
    for y in songs:
        y = _f64(y)
        if len(y) < 2:
            out.append(None)
            continue
        kyy, kxy = _mean(kmat(y, y, sigma, kernel), True), _mean(kmat(x, y, sigma, kernel), False)
        out.append({"mmd2": kxx + kyy - 2.0 * kxy, "kxx_mean": kxx, "kyy_mean": kyy, "kxy_mean": kxy, "bandwidth": sigma})
    return kxx, sigma, out


# ----------------------------------------------------------------------------------------------------------- uncertainty
def uncertainty(x, ys, sigma=None, kernel="gaussian"):
    x = _f64(x)
    ys = [_f64(y) for y in ys]
    if sigma is None:
        sigma = median_distance(x)
    n, S = x.shape[0], len(ys)
    kxx = kmat(x, x, sigma, kernel)
    np.fill_diagonal(kxx, 0.0)
    rxx = kxx.sum(1)
    mxx = rxx / (n - 1)
    a, b, out = np.zeros((S, n)), [], []
    for s, y in enumerate(ys):
        m = y.shape[0]
        kyy = kmat(y, y, sigma, kernel)
        np.fill_diagonal(kyy, 0.0)
        kxy = kmat(x, y, sigma, kernel)
        a[s] = mxx - kxy.sum(1) / m
        b.append(kyy.sum(1) / (m - 1) - kxy.sum(0) / n)
        out.append({"mmd2": a[s].mean() + b[s].mean(), "kxx_mean": rxx.sum() / (n * (n - 1)), "kyy_mean": kyy.sum() / (m * (m - 1)),
                    "kxy_mean": kxy.sum() / (n * m)})
    ac = a - a.mean(1, keepdims=True)
    cov = 4.0 / (n * (n - 1)) * (ac @ ac.T)
    for s, y in enumerate(ys):
        m = y.shape[0]
        cov[s, s] += 4.0 / (m * (m - 1)) * float(((b[s] - b[s].mean()) ** 2).sum())
    return {"sets": out, "cov": cov, "stderr": np.sqrt(np.diag(cov)), "proj_x": a, "proj_y": b, "bandwidth": sigma}


# ----------------------------------------------------------------------------------------------------------- permutation
def statistics(x, y, u, sigma=None, kernel="gaussian"):
    """t for every labelling row of u (bool / 0-1 [L, N]) -> float64 [L]; sigma defaults to the median pairwise distance of Z"""
    z = np.concatenate([_f64(x), _f64(y)])
    n, m = len(x), len(y)
    if sigma is None:
        sigma = float(np.median(pdist(z)))
    k = kmat(z, z, sigma, kernel)
    np.fill_diagonal(k, 0.0)
    u = np.asarray(u, dtype=np.float64)
    assert np.all(u.sum(1) == n), "every labelling needs exactly n ones"
    r = k.sum(1)
    T = r.sum()
    q = np.einsum("li,li->l", u @ k, u)
    R = u @ r
    sxx, sxy, syy = q, R - q, T - 2.0 * R + q
    return sxx / (n * (n - 1.0)) + syy / (m * (m - 1.0)) - 2.0 * sxy / (n * m)


# ------------------------------------------------------------------------------------------------- the float32 emulation
def epilogue32(acc, sigma, kernel):
    """The kernels' float32 epilogue on a float32 accumulator S' = -d^2 / 2 -> k as float64 values of float32 numbers."""
    acc = np.asarray(acc, dtype=np.float32)
    if kernel == "gaussian":                                      # CR.chain32_means: exp of the clamped accumulator
        return np.exp(np.minimum(acc.astype(np.float64), 0.0) / (sigma * sigma))
    c = np.float32(1.0 / (sigma * sigma))
    u = (1.0 - acc.astype(np.float64) * np.float64(c)).astype(np.float32)          # fma: the product is exact in float64, one rounding
    w = np.maximum(u, np.float32(1.0)).astype(np.float64)
    k = 1.0 / w if kernel == "iq" else 1.0 / np.sqrt(w)
    return k.astype(np.float32).astype(np.float64)


def chain32_means(x, y, sigma, step, kernel):
    """The kernel means and MMD^2 from the float32 chain of CR.chain32_acc and epilogue32, the sums in float64."""
    out = {name: CR._mean_of(epilogue32(CR.chain32_acc(a, b, step), sigma, kernel), same) for name, a, b, same in CR._pairs(x, y)}
    out["mmd2"] = out["kxx_mean"] + out["kyy_mean"] - 2.0 * out["kxy_mean"]
    return out
