"""float64 numpy reference of the leave-one-out k-NN two-sample test on the pooled rows (fad_nn_test) for the tests (test plumbing, not
product).

Z = [x; y] pooled, N = n + m.  graph(x, y, k): for every row j the k rows i != j in ascending order of (d^2, i) -- scipy cdist, the
diagonal at +inf, np.lexsort per row.  Under a 0/1 labelling u with n ones, row j is predicted baseline when more than k / 2 of
u[nn(j, .)] are 1 and correct when the prediction equals u[j]; counts() gives the correct rows with u[j] = 1 and with u[j] = 0 for
every labelling, p_values() the two tails on the integer totals, labelling 0 the observed one.  bracket() is nearest_reference's margin
form on the pooled rows with the self pair's margin made infinite, so that nearest_reference.valid_knn never asks for self."""
import importlib.util
from pathlib import Path

import numpy as np
from scipy.spatial.distance import cdist


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NR = _load("nearest_reference")
PR = _load("kad_permutation_reference")


def graph(x, y, k):
    """-> (index [N, k] int64, dist2 [N, k] float64): every pooled row's k nearest other pooled rows in ascending (d^2, i)."""
    z = PR.pooled(x, y)
    N = z.shape[0]
    d2 = cdist(z, z, "sqeuclidean")
    np.fill_diagonal(d2, np.inf)
    idx = np.empty((N, k), np.int64)
    for j in range(N):
        idx[j] = np.lexsort((np.arange(N), d2[j]))[:k]
    return idx, np.take_along_axis(d2, idx, 1)


def counts(index, u):
    """(correct_x [L], correct_y [L]) int64 for the labelling rows of u (bool [L, N]) on the graph ``index`` [N, k]."""
    index = np.asarray(index, dtype=np.int64)
    u = np.asarray(u, dtype=bool)
    k = index.shape[1]
    votes = u[:, index].sum(2)                                   # [L, N]: neighbours labelled 1
    correct = (2 * votes > k) == u
    return (correct & u).sum(1).astype(np.int64), (correct & ~u).sum(1).astype(np.int64)


def p_values(c):
    """c [L] integer totals, c[0] the observed one -> (p_value: upper tail, p_value_low: lower tail)"""
    c = np.asarray(c, dtype=np.int64)
    L = c.shape[0]
    return (1.0 + np.count_nonzero(c[1:] >= c[0])) / L, (1.0 + np.count_nonzero(c[1:] <= c[0])) / L


def results(index, n, m, u):
    """the whole result on a given graph: u [P, N] WITHOUT the observed labelling, which is put first here"""
    ua = np.concatenate([PR.observed_labelling(n, m), np.asarray(u, dtype=bool)])
    cx, cy = counts(index, ua)
    p, p_low = p_values(cx + cy)
    return {"accuracy": (cx[0] + cy[0]) / float(n + m), "accuracy_x": cx[0] / float(n), "accuracy_y": cy[0] / float(m), "p_value": p,
            "p_value_low": p_low, "correct_x": int(cx[0]), "correct_y": int(cy[0]), "null_correct_x": cx[1:], "null_correct_y": cy[1:]}


def reference(x, y, u, k):
    """graph and results in float64"""
    idx, d2 = graph(x, y, k)
    out = results(idx, len(x), len(y), u)
    out.update(index=idx, dist2=d2)
    return out


def bracket(x, y, tau):
    """nearest_reference's bracket of the pooled rows against themselves: d2 [N, N], margin tau (|z_i|^2 + |z_j|^2) with the self
    pair's margin infinite (self is never surely nearer than a returned row, and is never returned)."""
    z = PR.pooled(x, y)
    s = (z ** 2).sum(1)
    marg = tau * (s[:, None] + s[None, :])
    np.fill_diagonal(marg, np.inf)
    return {"d2": cdist(z, z, "sqeuclidean"), "margin": marg, "norms": s}


def valid_graph(index, dist2, br, k):
    """nearest_reference.valid_knn on the pooled rows, and no row its own neighbour -> bool [N]"""
    index = np.asarray(index, dtype=np.int64)
    ok = NR.valid_knn(index, dist2, br, k)
    return ok & (index != np.arange(index.shape[0])[:, None]).all(1)


# ---- a hand-written line: 4 baseline points at 0, 1, 2, 10 and 3 evaluation points at 3, 11, 12 (pooled rows 0 .. 6), with exact ties
# in distance (row 1: rows 0 and 2; row 2: rows 1 and 4; row 5: rows 3 and 6) that go to the smaller index.  The graphs, and the
# correct rows under the observed labelling and under 1010101, written out by hand.
LINE_X = np.array([[0.0], [1.0], [2.0], [10.0]], dtype=np.float32)
LINE_Y = np.array([[3.0], [11.0], [12.0]], dtype=np.float32)
LINE_U = np.array([[1, 0, 1, 0, 1, 0, 1]], dtype=bool)                            # one more labelling with 4 ones
LINE_GRAPH = {1: [[1], [0], [1], [5], [2], [3], [5]],
              3: [[1, 2, 4], [0, 2, 4], [1, 4, 0], [5, 6, 4], [2, 1, 0], [3, 6, 4], [5, 3, 4]]}
LINE_DIST2 = {1: [[1], [1], [1], [1], [1], [1], [1]],
              3: [[1, 4, 9], [1, 1, 4], [1, 1, 4], [1, 4, 49], [1, 4, 9], [1, 1, 64], [1, 4, 81]]}
# k -> ((correct_x, correct_y) observed, (correct_x, correct_y) under LINE_U)
LINE_COUNTS = {1: ((3, 1), (1, 2)), 3: ((3, 2), (3, 0))}


# ---- near copies: 200 evaluation rows, each a distinct baseline row plus 0.01 N(0, I), against the 300 baseline rows, D = 16
NEAR_COPIES_SEED = 7


def near_copies_case(n=300, m=200, d=16, P=199, noise=0.01, seed=NEAR_COPIES_SEED):
    """-> x, y (float32), labellings u [P, N] (without the observed one)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    rows = rng.choice(n, size=m, replace=False)
    y = (x[rows] + noise * rng.standard_normal((m, d))).astype(np.float32)
    return x, y, PR.random_labellings(n, m, P, rng)
