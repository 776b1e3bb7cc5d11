"""float64 numpy reference of the KAD standard errors (fad_kad_uncertainty) for the uncertainty tests (test plumbing, not product),
from the full kernel matrices, the definitions of include/fad_hip.h verbatim:

  mxx(i) = sum_{j != i} k(x_i, x_j) / (n - 1)           mxs(i) = sum_l k(x_i, y^s_l) / m_s
  mss(l) = sum_{l' != l} k(y^s_l, y^s_l') / (m_s - 1)    msx(l) = sum_i k(x_i, y^s_l) / n
  a^s_i = mxx(i) - mxs(i),  b^s_l = mss(l) - msx(l),  MMD^2_s = mean a^s + mean b^s
  cov[s][t] = 4 / (n (n - 1)) sum_i (a^s_i - mean a^s)(a^t_i - mean a^t) + [s = t] 4 / (m_s (m_s - 1)) sum_l (b^s_l - mean b^s)^2"""
import numpy as np
from scipy.spatial.distance import cdist, pdist


def _k(a, b, sigma):
    return np.exp(-cdist(a, b, "sqeuclidean") / (2.0 * sigma * sigma))


def uncertainty(x, ys, sigma=None):
    x = np.asarray(x, dtype=np.float64)
    ys = [np.asarray(y, dtype=np.float64) for y in ys]
    if sigma is None:
        sigma = float(np.median(pdist(x)))
    n, S = x.shape[0], len(ys)
    kxx = _k(x, x, sigma)
    np.fill_diagonal(kxx, 0.0)
    rxx = kxx.sum(1)
    mxx = rxx / (n - 1)
    a, b, out = np.zeros((S, n)), [], []
    for s, y in enumerate(ys):
        m = y.shape[0]
        kyy = _k(y, y, sigma)
        np.fill_diagonal(kyy, 0.0)
        kxy = _k(x, y, sigma)
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
