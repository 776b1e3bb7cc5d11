"""float64 numpy reference of the Kernel Audio Distance for the KAD tests (test plumbing, not product).

k(a, b) = exp(-|a - b|^2 / (2 sigma^2)); MMD^2 = Kxx + Kyy - 2 Kxy with the diagonal excluded by index from Kxx and Kyy;
sigma defaults to np.median(scipy.spatial.distance.pdist(x))."""
import numpy as np
from scipy.spatial.distance import cdist, pdist


def median_distance(x):
    return float(np.median(pdist(np.asarray(x, dtype=np.float64))))


def _kmean(a, b, sigma, same):
    d2 = cdist(a, b, "sqeuclidean")
    k = np.exp(-d2 / (2.0 * sigma * sigma))
    if same:
        np.fill_diagonal(k, 0.0)
        n = a.shape[0]
        return float(k.sum() / (n * (n - 1)))
    return float(k.sum() / (a.shape[0] * b.shape[0]))


def kad(x, y, sigma=None):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if sigma is None:
        sigma = median_distance(x)
    kxx, kyy, kxy = _kmean(x, x, sigma, True), _kmean(y, y, sigma, True), _kmean(x, y, sigma, False)
    return {"mmd2": kxx + kyy - 2.0 * kxy, "kxx_mean": kxx, "kyy_mean": kyy, "kxy_mean": kxy, "bandwidth": sigma}
