"""float64 numpy reference of the KAD permutation test for the tests (test plumbing, not product).

Z = [x; y] pooled (N = n + m rows), K' = exp(-|z_i - z_j|^2 / (2 sigma^2)) with a zero diagonal, r = K'1, T = 1'r.  For a 0/1
labelling u with n ones: q = u'K'u, R = u'r, Sxx = q, Sxy = R - q, Syy = T - 2R + q and
t(u) = Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m).  sigma defaults to the median pairwise distance of Z."""
import numpy as np
from scipy.spatial.distance import cdist, pdist


def pooled(x, y):
    return np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])


def median_distance_pooled(x, y):
    return float(np.median(pdist(pooled(x, y))))


def kernel(z, sigma):
    k = np.exp(-cdist(z, z, "sqeuclidean") / (2.0 * sigma * sigma))
    np.fill_diagonal(k, 0.0)
    return k


def statistics(x, y, u, sigma=None):
    """t for every labelling row of u (bool / 0-1 [L, N]) -> float64 [L]"""
    z = pooled(x, y)
    n, m = len(x), len(y)
    if sigma is None:
        sigma = median_distance_pooled(x, y)
    k = kernel(z, sigma)
    u = np.asarray(u, dtype=np.float64)
    assert np.all(u.sum(1) == n), "every labelling needs exactly n ones"
    r = k.sum(1)
    T = r.sum()
    q = np.einsum("li,li->l", u @ k, u)
    R = u @ r
    sxx, sxy, syy = q, R - q, T - 2.0 * R + q
    return sxx / (n * (n - 1.0)) + syy / (m * (m - 1.0)) - 2.0 * sxy / (n * m)


def observed_labelling(n, m):
    u = np.zeros((1, n + m), dtype=bool)
    u[0, :n] = True
    return u


def random_labellings(n, m, count, rng):
    u = np.zeros((count, n + m), dtype=bool)
    for p in range(count):
        u[p, rng.permutation(n + m)[:n]] = True
    return u


def p_value(t0, null):
    null = np.asarray(null, dtype=np.float64)
    return (1.0 + np.count_nonzero(null >= t0)) / (len(null) + 1.0)


def unpack(words, N):
    """packed words [P, ceil(N / 32)] (bit i & 31 of word i >> 5 is row i) -> bool [P, N]"""
    w = np.ascontiguousarray(np.asarray(words).view(np.uint32))
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :N].astype(bool)
