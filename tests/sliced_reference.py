"""The sliced 2-Wasserstein distance in numpy float64, restating the definition of DESIGN.md 4.17 and include/fad_hip.h
(fad_sliced_wasserstein), with the inputs, the rounding of the directions and the error bounds the GPU tests use.

Per direction l, with theta_l rounded to the rows' dtype, q_l = sum_d theta_ld^2 (float64, index order), a = sort(x theta_l),
b = sort(y theta_l):
    W_l = S_l / (n m q_l),   S_l = sum over overlapping (i, j) of w_ij (a_(i) - b_(j))^2,
    w_ij = min((i + 1) m, (j + 1) n) - max(i m, j n) > 0,
the integral of the squared difference of the two step quantile functions.  ``ordered=True`` sums S_l in the order the library documents
(per element of the larger set over its j ascending; blocks of 256 elements by a halving tree; blocks in index order): the same IEEE
operations in the same order, so the same bits whatever the values.  The plain order is numpy's.
"""
import math

import numpy as np

DTYPES = ("fp16", "bf16", "fp32")
U32 = 2.0 ** -23           # one ulp of float32 at 1: the matrix cores' summation inside a k step is not plain round-to-nearest
BLOCK = 256


def round_to_dtype(a, dt):
    """float32 values rounded to nearest even in ``dt`` -> float32 (numpy for float16, torch on the CPU for bfloat16)"""
    a = np.asarray(a, dtype=np.float32)
    if dt == "fp16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float32)
    if dt == "bf16":
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()
    return a.copy()


def direction_norms(theta_rounded):
    """q_l = sum_d theta_ld^2 in float64, summed in index order"""
    t = np.asarray(theta_rounded, dtype=np.float64)
    q = np.zeros(len(t))
    for c in range(t.shape[1]):
        q = q + t[:, c] * t[:, c]
    return q


def overlap(n, m):
    """-> (i, j, w): every overlapping pair of the sorted x (n) and y (m) and its exact integer weight, i major"""
    i = np.arange(n, dtype=np.int64)
    j0, j1 = (i * m) // n, ((i + 1) * m - 1) // n
    cnt = j1 - j0 + 1
    ii = np.repeat(i, cnt)
    jj = np.arange(cnt.sum(), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(j0, cnt)
    w = np.minimum((ii + 1) * m, (jj + 1) * n) - np.maximum(ii * m, jj * n)
    return ii, jj, w


def match_sum(a, b):
    """S of one direction from the SORTED a [n], b [m], float64, numpy's summation order"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    i, j, w = overlap(len(a), len(b))
    diff = a[i] - b[j]
    return float(np.sum(w.astype(np.float64) * (diff * diff)))


def match_sum_ordered(a, b):
    """S of one direction from the SORTED a, b in the library's documented order (the larger set leads, a when the sizes are equal)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if len(b) > len(a):
        a, b = b, a
    na, nb = len(a), len(b)
    i = np.arange(na, dtype=np.int64)
    lo, hi = i * nb, (i + 1) * nb
    j0, j1 = lo // na, (hi - 1) // na
    s = np.zeros(na)
    for k in range(int((j1 - j0).max()) + 1):
        j = j0 + k
        live = j <= j1
        jc = np.minimum(j, nb - 1)
        w = np.minimum(hi, (jc + 1) * na) - np.maximum(lo, jc * na)
        diff = a - b[jc]
        s = np.where(live, s + w.astype(np.float64) * (diff * diff), s)
    blocks = -(-na // BLOCK)
    t = np.zeros(blocks * BLOCK)
    t[:na] = s
    t = t.reshape(blocks, BLOCK)
    width = BLOCK // 2
    while width:
        t[:, :width] = t[:, :width] + t[:, width:2 * width]
        width //= 2
    total = 0.0
    for v in t[:, 0]:
        total = total + float(v)
    return total


def values_from_sorted(sa, sb, q, ordered=False):
    """W_l from the sorted projections sa [L x n], sb [L x m] and q [L]"""
    n, m = sa.shape[1], sb.shape[1]
    f = match_sum_ordered if ordered else match_sum
    return np.array([f(sa[l], sb[l]) / (float(n * m) * q[l]) for l in range(len(q))])


def statistics(values):
    """-> (sw2_squared, std_error, max_sliced, max_index) as the library forms them: in index order"""
    L = len(values)
    s = 0.0
    for v in values:
        s = s + float(v)
    mean = s / L
    d2 = 0.0
    for v in values:
        dv = float(v) - mean
        d2 = d2 + dv * dv
    se = math.sqrt(d2 / (L - 1)) / math.sqrt(L) if L > 1 else float("nan")
    k = int(np.argmax(values))
    return mean, se, float(values[k]), k


def sliced(x, y, theta, dt, ordered=False):
    """The reference: x, y float32 values representable in ``dt``, theta float32 [L x D] (rounded here) -> dict with values, q, the
    float64 sorted projections and the statistics"""
    t = round_to_dtype(theta, dt).astype(np.float64)
    q = direction_norms(t)
    pa = np.sort(np.asarray(x, dtype=np.float64) @ t.T, axis=0).T.copy()
    pb = np.sort(np.asarray(y, dtype=np.float64) @ t.T, axis=0).T.copy()
    values = values_from_sorted(pa, pb, q, ordered)
    mean, se, mx, k = statistics(values)
    return {"values": values, "q": q, "sorted_x": pa, "sorted_y": pb, "sw2_squared": mean, "std_error": se, "max_sliced": mx,
            "max_index": k, "fad_scale": x.shape[1] * mean}


def replicated_sum(a, b):
    """S through replication to lcm(n, m): element i of a stands for lcm / n equal points -- the definition the overlap form shortens"""
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    n, m = len(a), len(b)
    g = math.gcd(n, m)
    ra, rb = np.repeat(a, m // g), np.repeat(b, n // g)
    return float(np.sum((ra - rb) ** 2)) * g             # each of the lcm points weighs n m / lcm = gcd


def projection_bound(rows, theta_rounded, dt):
    """delta [L]: the bound on the float32 error of one projection, gamma_k max_i sum_d |x_id theta_ld|, gamma_k = k u / (1 - k u),
    u = 2^-23, k = D for 16-bit rows (exact products), D + 1 for float32 rows.  Sorting is 1-Lipschitz in the sup norm, so the bound holds
    elementwise for the sorted projections."""
    D = rows.shape[1]
    k = D if dt in ("fp16", "bf16") else D + 1
    gamma = k * U32 / (1.0 - k * U32)
    mags = np.abs(np.asarray(rows, dtype=np.float64)) @ np.abs(np.asarray(theta_rounded, dtype=np.float64)).T
    return gamma * mags.max(axis=0)


def value_bound(w_ref, q, dx, dy):
    """|W_l - reference| <= (2 sqrt(W_ref q) delta' + delta'^2) / q, delta' = delta_x + delta_y (Cauchy-Schwarz on (u + e)^2 - u^2)"""
    dd = dx + dy
    return (2.0 * np.sqrt(w_ref * q) * dd + dd * dd) / q


def rows(n, m, d, dt, seed=0):
    """standard normal rows, y shifted and scaled a little, rounded to ``dt`` -> float32"""
    rng = np.random.default_rng([seed, n, m, d])
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (1.25 * rng.standard_normal((m, d)) + 0.5).astype(np.float32)
    return round_to_dtype(x, dt), round_to_dtype(y, dt)


def directions(L, d, seed=0):
    return np.random.default_rng([7, seed, L, d]).standard_normal((L, d)).astype(np.float32)


def exact_rows(n, m, d, seed=0):
    """rows (integers in [-8, 8]) x 2^e_i, one e_i in [-8, 8] per row: representable in all three dtypes, every projection on integer
    directions exact in float32"""
    rng = np.random.default_rng([11, seed, n, m, d])
    x = rng.integers(-8, 9, (n, d)).astype(np.float32) * np.exp2(rng.integers(-8, 9, (n, 1))).astype(np.float32)
    y = rng.integers(-8, 9, (m, d)).astype(np.float32) * np.exp2(rng.integers(-8, 9, (m, 1))).astype(np.float32)
    return x, y


def exact_directions(L, d, seed=0):
    """integers in [-8, 8], no zero direction"""
    t = np.random.default_rng([13, seed, L, d]).integers(-8, 9, (L, d)).astype(np.float32)
    t[np.all(t == 0, axis=1), 0] = 1.0
    return t
