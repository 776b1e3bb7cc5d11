"""The sliced 2-Wasserstein permutation test in numpy float64, restating the definition of DESIGN.md 4.20 and include/fad_hip.h
(fad_sliced_permutation_test) on top of tests/sliced_reference.py.

Z = [x; y] is projected once on the rounded directions (float64).  A labelling u (bool [N], exactly n ones; labelling 0 is the observed
one, the first n rows) gives per direction a = sort of the projections with u = 1, b = sort of those with u = 0, and
W_l(u) = S_l(a, b) / (n m q_l) by ``values_from_sorted`` -- plain, or ``ordered`` in the library's summation order.  T(u) and M(u) are
``statistics`` of the L values; p = (1 + #{T(u_p) >= T(u_0), p >= 1}) / (P + 1), and the same with M.
"""
import numpy as np

import sliced_reference as SR


def labellings(n, m, P, seed=0):
    """P random labellings of N = n + m rows with exactly n ones each -> bool [P x N] (numpy's generator, one permutation each)"""
    rng = np.random.default_rng([17, seed, n, m, P])
    u = np.zeros((P, n + m), dtype=bool)
    for p in range(P):
        u[p, rng.permutation(n + m)[:n]] = True
    return u


def with_observed(u, n):
    """[P x N] -> [P + 1 x N]: the observed labelling (the first n rows) in front"""
    obs = np.zeros((1, u.shape[1]), dtype=bool)
    obs[0, :n] = True
    return np.concatenate([obs, np.asarray(u, dtype=bool)])


def p_values(T, M):
    """T, M [P + 1], entry 0 the observed labelling -> (p_value, p_value_max): (1 + #{null >= observed}) / (P + 1), ties counted"""
    T, M = np.asarray(T, dtype=np.float64), np.asarray(M, dtype=np.float64)
    P = len(T) - 1
    return (1 + int(np.sum(T[1:] >= T[0]))) / (P + 1), (1 + int(np.sum(M[1:] >= M[0]))) / (P + 1)


def values_of_projections(pz, q, u_all, ordered=False):
    """W [NL x L] from the pooled projections pz [N x L] (any order of rows), q [L] and the labellings u_all [NL x N]"""
    out = np.zeros((len(u_all), len(q)))
    for p, u in enumerate(u_all):
        sa = np.sort(pz[u], axis=0).T.copy()
        sb = np.sort(pz[~u], axis=0).T.copy()
        out[p] = SR.values_from_sorted(sa, sb, q, ordered)
    return out


def null_statistics(pz, q, u_all):
    """(T, M) [NL] of the labellings u_all [NL x N] from the pooled projections pz [N x L]: the same definition, all directions of a
    labelling at once (the sums over the overlapping pairs in numpy's order along the first axis) -- for the tests of the statistic
    itself, which run thousands of labellings"""
    u_all = np.asarray(u_all, dtype=bool)
    n = int(u_all[0].sum())
    m = pz.shape[0] - n
    i, j, w = SR.overlap(n, m)
    wf, den = w.astype(np.float64)[:, None], float(n * m) * q
    T, M = np.zeros(len(u_all)), np.zeros(len(u_all))
    for p, u in enumerate(u_all):
        diff = np.sort(pz[u], axis=0)[i] - np.sort(pz[~u], axis=0)[j]
        W = (wf * (diff * diff)).sum(axis=0) / den
        T[p], M[p] = W.mean(), W.max()
    return T, M


def permutation_test(x, y, theta, dt, u, ordered=False):
    """The reference: x, y float32 values representable in ``dt``, theta float32 [L x D] (rounded here), u bool [P x N] -> dict with
    values [P + 1 x L] (row 0 the observed labelling), q, T and M [P + 1], null, null_max, the two p-values, the observed statistics and
    the pooled float64 projections pz [N x L]"""
    n = len(x)
    t = SR.round_to_dtype(theta, dt).astype(np.float64)
    q = SR.direction_norms(t)
    pz = np.concatenate([np.asarray(x, dtype=np.float64) @ t.T, np.asarray(y, dtype=np.float64) @ t.T])      # as SR.sliced projects each set
    u_all = with_observed(u, n)
    values = values_of_projections(pz, q, u_all, ordered)
    stats = [SR.statistics(v) for v in values]
    T, M = np.array([s[0] for s in stats]), np.array([s[2] for s in stats])
    p, pmax = p_values(T, M)
    return {"values": values, "q": q, "pz": pz, "T": T, "M": M, "null": T[1:], "null_max": M[1:], "p_value": p, "p_value_max": pmax,
            "sw2_squared": stats[0][0], "std_error": stats[0][1], "max_sliced": stats[0][2], "max_index": stats[0][3]}
