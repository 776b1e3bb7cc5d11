"""float64 numpy reference of the nearest baseline rows and authenticity for the nearest-neighbour tests (test plumbing, not product).

nearest(x, y, k): for every row y_j the k rows of x in ascending order of (d^2, i) -- scipy cdist, then np.lexsort per column;
r1^2(i) = prdc_reference.radii2(x, 1) (self excluded by index); y_j is copied when d^2(y_j, x_nn(j)) <= r1^2(nn(j)).
The bracket form takes a margin tau: a float32 d^2 may lie tau (|x_i|^2 + |y_j|^2) from the float64 one, so a row i is a valid
l-th neighbour of y_j when at most l - 1 rows are surely nearer and the row is not surely farther than the k-th; a copied decision
within the margins of both sides may fall either way."""
import importlib.util
from pathlib import Path

import numpy as np
from scipy.spatial.distance import cdist

_spec = importlib.util.spec_from_file_location("prdc_reference", Path(__file__).resolve().parent / "prdc_reference.py")
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)


def nearest(x, y, k=1):
    """-> (index [m, k] int64, dist2 [m, k] float64) in ascending (d^2, i)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    d2 = cdist(y, x, "sqeuclidean")
    n = x.shape[0]
    idx = np.empty((y.shape[0], k), np.int64)
    for j in range(y.shape[0]):
        idx[j] = np.lexsort((np.arange(n), d2[j]))[:k]
    return idx, np.take_along_axis(d2, idx, 1)


def authenticity(x, y):
    """-> dict of index [m], dist2 [m], nn_radius2 [m], copied_rows [m], copied and authenticity (k = 1)."""
    idx, d2 = nearest(x, y, 1)
    r1, _ = P.radii2(x, 1)
    nn_r2 = r1[idx[:, 0]]
    rows = d2[:, 0] <= nn_r2
    return {"index": idx[:, 0], "dist2": d2[:, 0], "nn_radius2": nn_r2, "copied_rows": rows, "copied": int(rows.sum()),
            "authenticity": 1.0 - float(rows.sum()) / y.shape[0]}


def bracket(x, y, k, tau):
    """-> dict of the float64 d2 [m, n], its margins tau (|x_i|^2 + |y_j|^2) [m, n], r1^2 [n] with its margin [n], and copied_lo /
    copied_hi: the fewest and most rows of y whose copied decision can come out true when every d^2 may be off by its margin (the
    nearest row itself may be any row within the margin of the closest)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    sx, sy = (x ** 2).sum(1), (y ** 2).sum(1)
    d2 = cdist(y, x, "sqeuclidean")
    marg = tau * (sy[:, None] + sx[None, :])
    r1, nn1 = P.radii2(x, 1)
    re = P.radius_margin(x, nn1, tau)
    best = nearest(x, y, 1)[0][:, 0]
    cand = d2 - marg < (d2 + marg).min(1)[:, None]                      # rows that may come out nearest (a tie goes by index)
    cand[np.arange(y.shape[0]), best] = True
    sure = (d2 + marg <= r1[None, :] - re[None, :]) | ~cand              # copied for sure if this row is the one returned
    maybe = (d2 - marg <= r1[None, :] + re[None, :]) & cand
    return {"d2": d2, "margin": marg, "r1": r1, "r1_margin": re,
            "copied_lo": int(sure.all(1).sum()), "copied_hi": int(maybe.any(1).sum())}


def valid_knn(idx, d2_got, br, k):
    """True where row idx[j, l] may be y_j's l-th neighbour within the bracket: its d^2 within the margin of the returned value, and
    the returned list ascending, holding k distinct rows, none of which is surely farther than some row left out."""
    d2, marg = br["d2"], br["margin"]
    m = idx.shape[0]
    ok = np.ones(m, bool)
    for j in range(m):
        row = idx[j]
        if len(set(row.tolist())) != k or (np.diff(d2_got[j]) < 0).any():
            ok[j] = False
            continue
        lo, hi = d2[j] - marg[j], d2[j] + marg[j]
        if not (np.abs(d2_got[j].astype(np.float64) - d2[j, row]) <= marg[j, row]).all():
            ok[j] = False
            continue
        out = np.ones(d2.shape[1], bool)
        out[row] = False
        # every row left out must not be surely nearer than the farthest row kept
        if out.any() and lo[row].max() > hi[out].min():
            ok[j] = False
    return ok
