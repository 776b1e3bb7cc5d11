"""float64 numpy reference of the aggregated KAD permutation test for the tests (test plumbing, not product).

t is [B, L]: the statistic of bandwidth b under labelling j, labelling 0 the observed one (L = P + 1).
    p_b(j) = #{i : t_b(i) >= t_b(j)} / L,   p_values[b] = p_b(0),   m(j) = min_b p_b(j),   p_aggregated = #{j : m(j) <= m(0)} / L
-- the single-step min-p correction on the same labellings, uniform weights.  Counts are compared as integers.  The statistics come
from kad_permutation_reference.statistics, one bandwidth at a time.  Also the data of the calibration and power checks, so that the
host test (float64 alone) and the GPU test draw the same sets."""
import importlib.util
from pathlib import Path

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PR = _load("kad_permutation_reference")


def counts(t):
    """ge[b, j] = #{i : t[b, i] >= t[b, j]} (int64 [B, L])"""
    t = np.asarray(t, dtype=np.float64)
    return np.stack([(row[:, None] >= row[None, :]).sum(0) for row in t]).astype(np.int64)


def aggregate(t):
    """-> (p_values [B], p_aggregated)"""
    ge = counts(t)
    L = ge.shape[1]
    least = ge.min(0)
    return ge[:, 0] / float(L), float(np.count_nonzero(least <= least[0])) / float(L)


def statistics(x, y, u, sigmas):
    """t [B, L] for the labelling rows of u (the observed one is NOT added) at every sigma"""
    return np.stack([PR.statistics(x, y, u, float(s)) for s in sigmas])


def with_observed(n, m, u):
    return np.concatenate([PR.observed_labelling(n, m), np.asarray(u, dtype=bool)])


# ---- the "blobs" pair (Gretton et al. 2012): a 3 x 3 grid of unit Gaussians at spacing 10 against the same grid with within-blob
# correlation 0.8 -- the difference lives far below the median distance, where a median-sigma test is blind
BLOBS_LADDER = tuple(2.0 ** e for e in range(-5, 2))         # 1/32 .. 2 of the pooled median
BLOBS_SEED = 2                                               # checked on the CPU in float64 (test_kad_aggregate_host.py)


def blobs(n, m, rng, spacing=10.0, rho=0.8):
    cx = rng.integers(0, 3, size=(n, 2)) * spacing
    cy = rng.integers(0, 3, size=(m, 2)) * spacing
    x = cx + rng.standard_normal((n, 2))
    a = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
    y = cy + rng.standard_normal((m, 2)) @ a.T
    return x, y


def blobs_case(seed=BLOBS_SEED, n=400, m=400, P=199):
    """-> x, y (float32 values), labellings u [P, N] (without the observed one)"""
    rng = np.random.default_rng(seed)
    x, y = blobs(n, m, rng)
    u = PR.random_labellings(n, m, P, rng)
    return x.astype(np.float32), y.astype(np.float32), u


# ---- calibration: 100 null draws, both sets standard normal
CALIBRATION_FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0)
CALIBRATION_SEED0 = 1000                                     # draws use the seeds 1000 .. 1099; checked on the CPU in float64
CALIBRATION_CAP = 12                                         # of 100 aggregates <= 0.05: P(Bin(100, 0.05) >= 13) ~ 0.002


def null_draw(s, n=150, m=150, d=16, P=199):
    rng = np.random.default_rng(CALIBRATION_SEED0 + s)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.standard_normal((m, d)).astype(np.float32)
    u = PR.random_labellings(n, m, P, rng)
    return x, y, u
