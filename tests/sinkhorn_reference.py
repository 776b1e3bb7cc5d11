"""The Sinkhorn divergence in numpy float64, restating the definition of DESIGN.md 4.16 and include/fad_hip.h (fad_sinkhorn) with the
cost matrix materialised -- small shapes only.  Shared by tests/test_sinkhorn_host.py (self-checks, no GPU),
tests/test_gpu_sinkhorn.py and tests/test_gpu_sinkhorn_edges.py (the GPU entry against it).  Beside it, for the edge tests:
sinkhorn_blocked (the same definition in torch float64 with C recomputed per block of rows, for sizes whose C does not fit),
sinkhorn_chain32 (a float32 emulation of the arithmetic DESIGN.md 4.16 documents: what float32 costs on a case, the source of the
edge tests' bounds) and cross_plan (the unit map of csrc/kad_song_tiles.h restated).

    C_ij = |x_i - y_j|^2 / 2,  f = 0, g = 0, then L times   f_i <- -eps (LSE_j((g_j - C_ij) / eps) - log m)
                                                           g_j <- -eps (LSE_i((f_i - C_ij) / eps) - log n)      (g takes the new f)
    OT = mean(f) + mean(g);   marginal_error = mean_i |exp((f_i - f'_i) / eps) - 1| with f' one more f step, not adopted
    S = OT(x, y) - OT(x, x) / 2 - OT(y, y) / 2;   F = f - (f^xx + g^xx) / 2,  G = g - (f^yy + g^yy) / 2
"""
import functools

import numpy as np
from scipy.spatial.distance import pdist
from scipy.special import logsumexp

from kad_conditioning_reference import STEP, _column_order, h32

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
    return _assemble(ot(cost(x, y), eps, iterations), ot(cost(x, x), eps, iterations), ot(cost(y, y), eps, iterations), eps)


def unit(x, y, eps):
    """U = 2^-24 (max |x_i|^2 + max |y_j|^2) + 2^-24 eps log(max(n, m)): the float32 formation error of C plus that of exp / log"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    return 2.0 ** -24 * ((x * x).sum(axis=1).max() + (y * y).sum(axis=1).max()) + 2.0 ** -24 * eps * np.log(max(len(x), len(y)))


# ------------------------------------------------------------------------------------------------------------ edge rows
@functools.lru_cache(maxsize=None)
def edge_rows(n, m, d, dt, off=0.0, sep=0.0):
    """the rows of rows() with `off` added to every element of both sets and `sep` more to y, rounded to dt AFTER the addition, so that
    the reference and the GPU see the same values -> (x, y) float32 (read-only)"""
    x, y = rows(n, m, d, dt)
    x = round_to(x + np.float32(off), dt)
    y = round_to(y + np.float32(off) + np.float32(sep), dt)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


# -------------------------------------------------------------------------------------------------------- the unit map
TILE = 128
CROSS_UNITS = 8192                  # kad::kCrossUnits
LAUNCH_BUDGET = 1 << 30             # kad::kLaunchBudget, the default
SOFTMIN_EPILOGUE = 192              # kad::kSoftminEpilogue


def cross_plan(n_rows, n_cols, depth=64, f32=False):
    """-> (TI, TJ, rr, NR) of one half-step that reduces n_rows rows into n_cols columns: kad::cross_rows_per_unit and
    kad::cross_ranges of csrc/kad_song_tiles.h at the default launch budget (softmin_plan of csrc/kad.hip; `depth` is the packed row
    length in elements, which the default budget makes irrelevant below about 10^4 row blocks).  Unit u = R * TJ + J walks the row
    blocks [R * rr, min(TI, (R + 1) * rr)) of column block J."""
    TI, TJ = -(-n_rows // TILE), -(-n_cols // TILE)
    per_launch = max(64, LAUNCH_BUDGET // ((16 * depth if f32 else depth) + SOFTMIN_EPILOGUE))
    nr = max(1, min(TI, -(-CROSS_UNITS // TJ)))
    rr = min(-(-TI // nr), per_launch)
    return TI, TJ, rr, -(-TI // rr)


# ------------------------------------------------------------------------------------------- float64, C never stored whole
def _blocked_step(a, b, p, eps, block):
    """torch float64: q_i = -eps (LSE_j((p_j - C_ij) / eps) - log(len(b))) for the rows i of a, a block of rows of a at a time"""
    import math

    import torch
    nb = (b * b).sum(dim=1)
    out = torch.empty(len(a), dtype=torch.float64, device=a.device)
    for i0 in range(0, len(a), block):
        ab = a[i0:i0 + block]
        Cm = 0.5 * ((ab * ab).sum(dim=1)[:, None] + nb[None, :]) - ab @ b.T
        out[i0:i0 + block] = -eps * (torch.logsumexp((p[None, :] - Cm) / eps, dim=1) - math.log(len(b)))
    return out


def _blocked_ot(a, b, eps, iterations, block):
    import torch
    f = torch.zeros(len(a), dtype=torch.float64, device=a.device)
    g = torch.zeros(len(b), dtype=torch.float64, device=a.device)
    for _ in range(iterations):
        f = _blocked_step(a, b, g, eps, block)
        g = _blocked_step(b, a, f, eps, block)
    f2 = _blocked_step(a, b, g, eps, block)
    return {"f": f.cpu().numpy(), "g": g.cpu().numpy(), "value": float(f.mean() + g.mean()),
            "marginal_error": float(torch.expm1((f - f2) / eps).abs().mean())}


def _assemble(xy, xx, yy, eps):
    return {"divergence": xy["value"] - 0.5 * xx["value"] - 0.5 * yy["value"], "ot_xy": xy["value"], "ot_xx": xx["value"],
            "ot_yy": yy["value"], "marginal_error": xy["marginal_error"], "marginal_error_xx": xx["marginal_error"],
            "marginal_error_yy": yy["marginal_error"], "f": xy["f"], "g": xy["g"], "pot_x": xy["f"] - 0.5 * (xx["f"] + xx["g"]),
            "pot_y": xy["g"] - 0.5 * (yy["f"] + yy["g"]), "epsilon": float(eps)}


def sinkhorn_blocked(x, y, eps, iterations, device, block=2048):
    """sinkhorn() in torch float64 on `device`, C = (|a|^2 + |b|^2) / 2 - a.b recomputed per block of `block` rows at every half-step and
    never stored whole: the reference for sizes whose cost matrix does not fit.  -> the dict of sinkhorn(), numpy float64."""
    import torch
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64), device=device)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64), device=device)
    return _assemble(_blocked_ot(xt, yt, eps, iterations, block), _blocked_ot(xt, xt, eps, iterations, block),
                     _blocked_ot(yt, yt, eps, iterations, block), eps)


# ---------------------------------------------------------------------------------------------- the float32 emulation
# Rows of a 128-row block in the order one lane of sinkhorn_cols_kernel holds them: group (wm, h) -- wave row wm, lane half h -- has
# the rows 64 wm + 32 bi + 8 (g >> 2) + 4 h + (g & 3), summed in the order (bi, g).  [4 groups, 32]
_LANE_ROWS = np.array([[64 * wm + 32 * bi + 8 * (g >> 2) + 4 * h + (g & 3) for bi in range(2) for g in range(16)]
                       for wm in range(2) for h in range(2)])


def _ref32(m):
    return np.where(np.isneginf(m), np.float32(0), m)


def _merge32(M, S, m2, s2, c):
    """lse_merge of csrc/kad.hip in float32: (M, S) merged with (m2, s2), in this order"""
    nm = np.maximum(M, m2)
    ref = _ref32(nm)
    return nm, S * np.exp2((M - ref) * c) + s2 * np.exp2((m2 - ref) * c)


def chain32_v(a, b, ha, hb, step):
    """kad_conditioning_reference.chain32_acc with the two h vectors given: acc = fl32(ha_i + hb_j), then one float32 rounding per block
    of `step` columns in the kernel's order, each block dot taken in float64 -> v [rows of a, rows of b] float32"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = a.shape[1]
    cols = _column_order(d, step)
    pa = np.zeros((a.shape[0], cols.size))
    pb = np.zeros((b.shape[0], cols.size))
    pa[:, :d], pb[:, :d] = a, b
    pa, pb = pa[:, cols], pb[:, cols]
    acc = ha[:, None] + hb[None, :]
    assert acc.dtype == np.float32
    for c0 in range(0, cols.size, step):
        acc = (acc.astype(np.float64) + pa[:, c0:c0 + step] @ pb[:, c0:c0 + step].T).astype(np.float32)
    return acc


def softmin32(v, c32, eps):
    """The soft-min epilogue of DESIGN.md 4.16 on v [rows, columns] float32 -> the columns' potentials, float64:
    per tile and group of 32 rows the maximum and the float32 sum of exp2(fl32(fl32(v - M) c)) against it, merged into the group's running
    state over the row blocks of a unit (cross_plan), the four groups merged in float32 (lane halves, then waves), the units in float64."""
    n_rows, n_cols = v.shape
    TI, _, rr, NR = cross_plan(n_rows, n_cols)
    pad = np.full((TI * TILE, n_cols), -np.inf, dtype=np.float32)
    pad[:n_rows] = v
    t = pad.reshape(TI, TILE, n_cols)[:, _LANE_ROWS, :]                            # [TI, 4, 32, columns]
    tm = t.max(axis=2)
    ref = _ref32(tm)
    ts = np.zeros_like(tm)
    for k in range(32):
        ts = ts + np.exp2((t[:, :, k, :] - ref) * c32)
    assert ts.dtype == np.float32
    M64 = np.full(n_cols, -np.inf)
    S64 = np.zeros(n_cols)
    for R in range(NR):
        M = np.full((4, n_cols), -np.inf, dtype=np.float32)
        S = np.zeros((4, n_cols), dtype=np.float32)
        for I in range(R * rr, min(TI, (R + 1) * rr)):
            M, S = _merge32(M, S, tm[I], ts[I], c32)
        Mw, Sw = _merge32(M[0::2], S[0::2], M[1::2], S[1::2], c32)                  # lane halves: [2 waves, columns]
        Mu, Su = _merge32(Mw[0], Sw[0], Mw[1], Sw[1], c32)
        m2 = Mu.astype(np.float64)
        nm = np.maximum(M64, m2)
        ref64 = np.where(np.isneginf(nm), 0.0, nm)
        S64 = S64 * np.exp2((M64 - ref64) * float(c32)) + Su.astype(np.float64) * np.exp2((m2 - ref64) * float(c32))
        M64 = nm
    return -(M64 + eps * np.log(S64)) + eps * np.log(n_rows)


def _chain32_ot(a, b, eps, iterations, step):
    """one problem: f over the rows of b for every row of a, g the other way; the potential rides in the row operand's h vector"""
    c32 = np.float32(1.4426950408889634 / eps)
    ha0, hb0 = h32(a), h32(b)

    def half(rows_, cols_, h_rows, h_cols, p):
        hp = h_rows if p is None else h_rows + p.astype(np.float32)
        return softmin32(chain32_v(rows_, cols_, hp, h_cols, step), c32, eps)
    f = g = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(iterations):
            f = half(b, a, hb0, ha0, g)
            g = half(a, b, ha0, hb0, f)
        f2 = half(b, a, hb0, ha0, g)
    return {"f": f, "g": g, "value": float(f.mean() + g.mean()), "marginal_error": float(np.abs(np.expm1((f - f2) / eps)).mean())}


def sinkhorn_chain32(x, y, eps, iterations, dt):
    """A float32 emulation of what DESIGN.md 4.16 documents, on the CPU -> the dict of sinkhorn().  v_ij by chain32_v with
    ha = fl32(h32(rows) + fl32(p)) and hb = h32(columns); then softmin32; the potential in float64.  It models the SIZES of the errors
    (the rounding of h + p, the accumulation over D, the float32 exponent and sums), not the kernel's bits: exp2 here is numpy's, and
    the MFMA's order inside a block of STEP[dt] columns is not known.
    Compare f, g of (x, y), F, G, the three OT terms and S against float64, NOT f and g of the self problems one by one: there the
    diagonal pair dominates, so f_i - g_i is nearly free and drifts with L (40 U in this emulation where f + g stays within 1 U)."""
    step = STEP[dt]
    return _assemble(_chain32_ot(x, y, eps, iterations, step), _chain32_ot(x, x, eps, iterations, step),
                     _chain32_ot(y, y, eps, iterations, step), eps)


POTS = ("f", "g", "pot_x", "pot_y")
TERMS = ("ot_xy", "ot_xx", "ot_yy", "divergence")


def ratios(got, want, U):
    """error / U of the four potentials (the worst row) and of the four terms"""
    out = {k: float(np.abs(got[k] - want[k]).max()) / U for k in POTS}
    out.update({k: abs(got[k] - want[k]) / U for k in TERMS})
    return out
