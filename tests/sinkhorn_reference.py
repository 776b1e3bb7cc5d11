"""The Sinkhorn divergence in numpy float64, restating the definition of DESIGN.md 4.16 and include/fad_hip.h (fad_sinkhorn) with the
cost matrix materialised -- small shapes only.  Shared by tests/test_sinkhorn_host.py (self-checks, no GPU) and
tests/test_gpu_sinkhorn.py (the GPU entry against it).

    C_ij = |x_i - y_j|^2 / 2,  f = 0, g = 0, then L times   f_i <- -eps (LSE_j((g_j - C_ij) / eps) - log m)
                                                           g_j <- -eps (LSE_i((f_i - C_ij) / eps) - log n)      (g takes the new f)
    OT = mean(f) + mean(g);   marginal_error = mean_i |exp((f_i - f'_i) / eps) - 1| with f' one more f step, not adopted
    S = OT(x, y) - OT(x, x) / 2 - OT(y, y) / 2;   F = f - (f^xx + g^xx) / 2,  G = g - (f^yy + g^yy) / 2
"""
import functools

import numpy as np
from scipy.spatial.distance import pdist
from scipy.special import logsumexp

DTYPES = ("fp16", "bf16", "fp32")
SHAPES = ((300, 200, 37), (129, 127, 128), (128, 128, 64), (1, 1, 5), (257, 130, 64))
BLUR_FACTOR = 0.25


def round_to(a, dt):
    """float32 values rounded to dtype dt (round to nearest even), as float32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == "fp16":
        return a.astype(np.float16).astype(np.float32)
    if dt == "bf16":
        u = a.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)
    return a


@functools.lru_cache(maxsize=None)
def rows(n, m, d, dt, seed=0):
    """standard normal rows rounded to dt -> (x [n, d], y [m, d]) float32 (read-only)"""
    rng = np.random.default_rng([seed, n, m, d])
    x = round_to(rng.standard_normal((n, d)), dt)
    y = round_to(rng.standard_normal((m, d)), dt)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def cost(x, y):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    return 0.5 * ((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=-1)


def median_distance(x):
    return float(np.median(pdist(np.asarray(x, dtype=np.float64))))


def f_step(C, g, eps):
    return -eps * (logsumexp((g[None, :] - C) / eps, axis=1) - np.log(C.shape[1]))


def g_step(C, f, eps):
    return -eps * (logsumexp((f[:, None] - C) / eps, axis=0) - np.log(C.shape[0]))


def plan_mass(C, f, g, eps):
    """sum_ij exp((f_i + g_j - C_ij) / eps) / (n m): the total mass of the transport plan"""
    return float(np.exp(logsumexp((f[:, None] + g[None, :] - C) / eps) - np.log(C.size)))


def ot(C, eps, iterations, check=None):
    """-> dict f, g, value, marginal_error of one problem; check(f, g) is called after every g step"""
    n, m = C.shape
    f, g = np.zeros(n), np.zeros(m)
    for _ in range(iterations):
        f = f_step(C, g, eps)
        g = g_step(C, f, eps)
        if check is not None:
            check(f, g)
    f2 = f_step(C, g, eps)
    return {"f": f, "g": g, "value": float(f.mean() + g.mean()), "marginal_error": float(np.abs(np.expm1((f - f2) / eps)).mean())}


def sinkhorn(x, y, eps, iterations):
    """-> dict: divergence, ot_xy, ot_xx, ot_yy, marginal_error / _xx / _yy, f, g, pot_x (F), pot_y (G), epsilon"""
    xy, xx, yy = ot(cost(x, y), eps, iterations), ot(cost(x, x), eps, iterations), ot(cost(y, y), eps, iterations)
    return {"divergence": xy["value"] - 0.5 * xx["value"] - 0.5 * yy["value"], "ot_xy": xy["value"], "ot_xx": xx["value"],
            "ot_yy": yy["value"], "marginal_error": xy["marginal_error"], "marginal_error_xx": xx["marginal_error"],
            "marginal_error_yy": yy["marginal_error"], "f": xy["f"], "g": xy["g"], "pot_x": xy["f"] - 0.5 * (xx["f"] + xx["g"]),
            "pot_y": xy["g"] - 0.5 * (yy["f"] + yy["g"]), "epsilon": float(eps)}


def unit(x, y, eps):
    """U = 2^-24 (max |x_i|^2 + max |y_j|^2) + 2^-24 eps log(max(n, m)): the float32 formation error of C plus that of exp / log"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    return 2.0 ** -24 * ((x * x).sum(axis=1).max() + (y * y).sum(axis=1).max()) + 2.0 ** -24 * eps * np.log(max(len(x), len(y)))
