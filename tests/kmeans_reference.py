"""float64 numpy reference of Lloyd's k-means as fad_kmeans defines it (include/fad_hip.h), for the k-means and MAUVE
tests (test plumbing, not product).

assign(x, c):  every row takes the centroid with the smallest key (d^2, index): float64 squared distances, equal d^2 to the smaller
               index.
update(x, labels, c):  c_k = float32(float64 sum of the rows of cluster k / count_k); a cluster without rows keeps its centroid.
lloyd(x, init, max_iter):  for t = 1 .. max_iter: A_t = A(C_{t-1}); if t > 1 and A_t == A_{t-1} stop, converged; else C_t = M(A_t).
               When the loop runs out (and for max_iter = 0) the labels are one more assignment against the last centroids."""
import numpy as np


def dist2(x, c):
    """-> [N, K] float64 squared distances, as a sum of squared differences (no cancellation)."""
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    for k in range(c.shape[0]):
        out[:, k] = ((x - c[k]) ** 2).sum(1)
    return out


def assign(x, c):
    """-> (labels [N] int64, d2 [N] float64 of the chosen centroid, all d2 [N, K])."""
    d2 = dist2(x, c)
    labels = d2.argmin(1)                                  # the first minimum: equal d^2 go to the smaller index
    return labels, d2[np.arange(d2.shape[0]), labels], d2


def update(x, labels, c):
    """-> (centroids [K, D] float32, counts [K] int64)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.array(c, dtype=np.float32, copy=True)
    k = out.shape[0]
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    for j in np.flatnonzero(counts):
        out[j] = (x[labels == j].sum(0) / counts[j]).astype(np.float32)
    return out, counts


def lloyd(x, init, max_iter):
    """-> dict of centroids (float32), labels, dist2, counts, inertia, inertia_trace, iterations, converged, empty_clusters"""
    c = np.array(init, dtype=np.float32, copy=True)
    trace, prev, labels, d2 = [], None, None, None
    converged, iterations = 0, 0
    for t in range(1, max_iter + 1):
        labels, d2, _ = assign(x, c)
        trace.append(d2.sum())
        iterations = t
        if prev is not None and np.array_equal(labels, prev):
            converged = 1
            break
        c, _ = update(x, labels, c)
        prev = labels
    if not converged:
        labels, d2, _ = assign(x, c)
        trace.append(d2.sum())
    counts = np.bincount(labels, minlength=c.shape[0]).astype(np.int64)
    return {"centroids": c, "labels": labels, "dist2": d2, "counts": counts, "inertia": trace[-1], "inertia_trace": np.array(trace),
            "iterations": iterations, "converged": converged, "empty_clusters": int((counts == 0).sum())}


def seed_rows(n_rows, clusters, seed, restart):
    """The rows restart `restart` draws its init from: K distinct pooled rows, ascending."""
    return np.sort(np.random.default_rng([seed, restart]).choice(n_rows, clusters, replace=False))
