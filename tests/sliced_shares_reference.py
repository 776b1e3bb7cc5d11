"""Every row's share of the sliced 2-Wasserstein distance in numpy float64, restating the definition of DESIGN.md 4.19 and
include/fad_hip.h (fad_sliced_shares) on top of tests/sliced_reference.py.

Per direction l, a = the projections of x sorted ascending, b = those of y; rx[r] / ry[r] = the row at rank r, equal projections in
ascending row order (a stable argsort).  "Lead" is the larger set (x at n == m), A [na]; the other is B [nb]:
    lead element at rank i:   c(i) = sum_{j = j0 .. j1} w_ij (A_i - B_j)^2,  j0 = i nb // na, j1 = ((i + 1) nb - 1) // na, j ascending
    other element at rank j:  c(j) = sum_{i = i0 .. i1} w_ij (A_i - B_j)^2,  i0 = j na // nb, i1 = ((j + 1) na - 1) // nb, i ascending
    w_ij = min((i + 1) nb, (j + 1) na) - max(i nb, j na)
    t_l(row) = c / (float(n m) q_l);   share[row] = (sum_l t_l(row), l ascending, one running sum) / L.
``ordered=True`` walks these sums term by term as the library documents them; the plain order is numpy's (np.bincount over the
overlapping pairs of sliced_reference.overlap, i major).  Both sum the terms of one element in ascending partner order, so they agree
to the last bit: two independent spellings of one definition.
"""
import math

import numpy as np

import sliced_reference as SR

LCM_SIZES = ((1, 1), (7, 1), (6, 4), (33, 32), (128, 64), (257, 130), (300, 1), (3, 2), (5, 5))


def _lead_costs_ordered(a, b):
    """c per rank of the larger a [na] over its partners j ascending, and c per rank of b [nb] over its partners i ascending"""
    na, nb = len(a), len(b)
    i = np.arange(na, dtype=np.int64)
    lo, hi = i * nb, (i + 1) * nb
    j0, j1 = lo // na, (hi - 1) // na
    ca = np.zeros(na)
    for k in range(int((j1 - j0).max()) + 1):
        j = j0 + k
        live = j <= j1
        jc = np.minimum(j, nb - 1)
        w = np.minimum(hi, (jc + 1) * na) - np.maximum(lo, jc * na)
        diff = a - b[jc]
        ca = np.where(live, ca + w.astype(np.float64) * (diff * diff), ca)
    j = np.arange(nb, dtype=np.int64)
    lo, hi = j * na, (j + 1) * na
    i0, i1 = lo // nb, (hi - 1) // nb
    cb = np.zeros(nb)
    for k in range(int((i1 - i0).max()) + 1):
        i = i0 + k
        live = i <= i1
        ic = np.minimum(i, na - 1)
        w = np.minimum(hi, (ic + 1) * nb) - np.maximum(lo, ic * nb)
        diff = a[ic] - b
        cb = np.where(live, cb + w.astype(np.float64) * (diff * diff), cb)
    return ca, cb


def rank_costs(a, b, ordered=False):
    """-> (cx [n], cy [m]): the cost of every rank of a (x's side, ordered as given) and of b (y's side), float64.  a and b need not be
    monotone: the formulas only pair ranks."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if ordered:
        if len(b) > len(a):
            cb, ca = _lead_costs_ordered(b, a)
            return ca, cb
        return _lead_costs_ordered(a, b)
    i, j, w = SR.overlap(len(a), len(b))                                               # i major, j ascending within i (and i within j)
    diff = a[i] - b[j]
    term = w.astype(np.float64) * (diff * diff)
    return np.bincount(i, weights=term, minlength=len(a)), np.bincount(j, weights=term, minlength=len(b))


def shares_from_sorted(sa, sb, ix, iy, q, ordered=False):
    """share_x [n], share_y [m] from the projections along the ranks sa [L x n], sb [L x m], the rows at the ranks ix, iy and q [L]"""
    L, n = sa.shape
    m = sb.shape[1]
    acc_x, acc_y = np.zeros(n), np.zeros(m)
    for l in range(L):
        cx, cy = rank_costs(sa[l], sb[l], ordered)
        den = float(n * m) * q[l]
        tx, ty = np.zeros(n), np.zeros(m)
        tx[ix[l]] = cx / den
        ty[iy[l]] = cy / den
        acc_x, acc_y = acc_x + tx, acc_y + ty
    return acc_x / L, acc_y / L


def projections(rows, theta, dt):
    """float64 projections [L x n] of the rows on theta rounded to ``dt``, and q"""
    t = SR.round_to_dtype(theta, dt).astype(np.float64)
    return (np.asarray(rows, dtype=np.float64) @ t.T).T.copy(), SR.direction_norms(t)


def stable_order(p):
    """the rows at the ranks of every direction: a stable argsort (equal projections in ascending row order; -0 == +0 here)"""
    return np.argsort(p, axis=1, kind="stable")


def shares(x, y, theta, dt, ordered=False):
    """The free reference: float64 projections, their own stable argsort -> dict of share_x, share_y, index_x, index_y, q"""
    px, q = projections(x, theta, dt)
    py, _ = projections(y, theta, dt)
    ix, iy = stable_order(px), stable_order(py)
    sx, sy = shares_from_sorted(np.take_along_axis(px, ix, 1), np.take_along_axis(py, iy, 1), ix, iy, q, ordered)
    return {"share_x": sx, "share_y": sy, "index_x": ix, "index_y": iy, "q": q}


def replicated_costs(a, b):
    """(cx, cy) of SORTED a [n], b [m] through replication to lcm(n, m): element i of a stands for lcm / n equal points, matched in
    order with b's; every replicated pair weighs gcd (n m / lcm), and an element's cost is the sum over its own points"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n, m = len(a), len(b)
    g = math.gcd(n, m)
    sq = (np.repeat(a, m // g) - np.repeat(b, n // g)) ** 2 * g
    return sq.reshape(n, m // g).sum(axis=1), sq.reshape(m, n // g).sum(axis=1)


def share_bound(px_along, py_along, q, dx, dy):
    """The bound on |share - float64 share along the same order| per row of x and of y.  A device difference is d = d* + e with d* the
    float64 difference of the same pair and |e| <= delta' = delta_x + delta_y (projection_bound, per direction), so
    |d^2 - d*^2| <= 2 |d*| delta' + delta'^2 per term; weighted by w_ij, summed over the element's partners, divided by n m q_l and
    averaged over l.  -> (bound per RANK-aligned array [L x n], [L x m]): the caller scatters them to rows with the same indices."""
    L, n = px_along.shape
    m = py_along.shape[1]
    i, j, w = SR.overlap(n, m)
    bx, by = np.zeros((L, n)), np.zeros((L, m))
    for l in range(L):
        dd = dx[l] + dy[l]
        term = w.astype(np.float64) * (2.0 * np.abs(px_along[l][i] - py_along[l][j]) * dd + dd * dd) / (float(n * m) * q[l])
        bx[l] = np.bincount(i, weights=term, minlength=n)
        by[l] = np.bincount(j, weights=term, minlength=m)
    return bx, by


def sequential_sum(v):
    """a plain running float64 sum in index order"""
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1])
