"""float64 numpy reference of precision, recall, density and coverage for the PRDC tests (test plumbing, not product).

r2(i) = the k-th smallest squared distance from row i to the OTHER rows of its set (scipy cdist, the diagonal set to +inf, then
np.partition); P1(i, j) = d2(x_i, y_j) < r2_x(i), P2(i, j) = d2(x_i, y_j) < r2_y(j), all strict:
    precision = mean_j any_i P1     recall = mean_i any_j P2     density = sum P1 / (k m)     coverage = mean_i any_j P1
The bracket form takes a margin tau: every decision whose d2 lies within tau (|x_i|^2 + |y_j|^2) plus the radius's own margin
tau (|row|^2 + |k-th neighbour|^2) of its threshold may fall either way, and it returns the lowest and highest count or flag each
per-row output can take."""
import numpy as np
from scipy.spatial.distance import cdist


def radii2(a, k):
    """-> (r2 [n], index of the k-th neighbour [n]) within one set, self excluded by index."""
    a = np.asarray(a, dtype=np.float64)
    d2 = cdist(a, a, "sqeuclidean")
    np.fill_diagonal(d2, np.inf)
    nn = np.argpartition(d2, k - 1, axis=1)[:, k - 1]
    return d2[np.arange(a.shape[0]), nn], nn


def _totals(balls_y, recalled, covered, k):
    m, n = balls_y.shape[0], recalled.shape[0]
    return {"precision": float((balls_y > 0).sum() / m), "recall": float(recalled.sum() / n),
            "density": float(balls_y.sum() / (k * m)), "coverage": float(covered.sum() / n)}


def prdc(x, y, k=5):
    """-> dict of the four values and the per-row radius2_x, radius2_y, balls_y, flags_x (bit 0 recalled, bit 1 covered)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    r2x, _ = radii2(x, k)
    r2y, _ = radii2(y, k)
    d2 = cdist(x, y, "sqeuclidean")
    p1 = d2 < r2x[:, None]
    p2 = d2 < r2y[None, :]
    balls = p1.sum(0).astype(np.int64)
    recalled, covered = p2.any(1), p1.any(1)
    out = _totals(balls, recalled, covered, k)
    out.update(radius2_x=r2x, radius2_y=r2y, balls_y=balls, flags_x=recalled.astype(np.int64) | (covered.astype(np.int64) << 1))
    return out


def radius_margin(a, nn, tau):
    """tau (|a_i|^2 + |a_nn(i)|^2): how far a float32 r2(i) may lie from the float64 one."""
    sq = (np.asarray(a, dtype=np.float64) ** 2).sum(1)
    return tau * (sq + sq[nn])


def bracket(x, y, k, tau):
    """-> dict with lo / hi arrays of balls_y, recalled_x, covered_x and lo / hi of the four values, for decisions within the margin of
    their thresholds going either way; also the float64 radii and their margins."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    r2x, nnx = radii2(x, k)
    r2y, nny = radii2(y, k)
    ex, ey = radius_margin(x, nnx, tau), radius_margin(y, nny, tau)
    sx, sy = (x ** 2).sum(1), (y ** 2).sum(1)
    d2 = cdist(x, y, "sqeuclidean")
    pair = tau * (sx[:, None] + sy[None, :])
    g1 = d2 - r2x[:, None]
    g2 = d2 - r2y[None, :]
    m1 = pair + ex[:, None]
    m2 = pair + ey[None, :]
    p1_lo, p1_hi = g1 < -m1, g1 < m1
    p2_lo, p2_hi = g2 < -m2, g2 < m2
    out = {"balls_lo": p1_lo.sum(0), "balls_hi": p1_hi.sum(0), "recalled_lo": p2_lo.any(1), "recalled_hi": p2_hi.any(1),
           "covered_lo": p1_lo.any(1), "covered_hi": p1_hi.any(1), "radius2_x": r2x, "radius2_y": r2y, "radius_margin_x": ex,
           "radius_margin_y": ey}
    lo = _totals(out["balls_lo"], out["recalled_lo"], out["covered_lo"], k)
    hi = _totals(out["balls_hi"], out["recalled_hi"], out["covered_hi"], k)
    out.update({f"{key}_lo": v for key, v in lo.items()})
    out.update({f"{key}_hi": v for key, v in hi.items()})
    return out
