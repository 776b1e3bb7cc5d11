"""The sliced 2-Wasserstein bootstrap in numpy float64, restating the definition of DESIGN.md 4.21 and include/fad_hip.h
(fad_sliced_bootstrap) on top of tests/sliced_reference.py.

A replicate is a pair of uint8 count vectors (cx [n], cy [m]); its sets are np.repeat(x, cx, axis=0) and np.repeat(y, cy, axis=0) -- rows in
ascending order, copies adjacent -- and its values are those of ``SR.sliced`` on them.  Replicate 0 is the sets as given (all ones).
The interval statistics are plain numpy on the replicates' means.
"""
import numpy as np

import sliced_reference as SR


def with_observed(counts):
    """[B x rows] -> [B + 1 x rows]: the all-ones replicate in front"""
    counts = np.asarray(counts, dtype=np.uint8)
    return np.concatenate([np.ones((1, counts.shape[1]), dtype=np.uint8), counts])


def row_counts(rows, B, seed=0, top=4):
    """B replicates of ``rows`` rows with counts 0 .. top - 1 at random, never all zero -> uint8 [B x rows] (for tests that give counts)"""
    rng = np.random.default_rng([19, seed, rows, B])
    c = rng.integers(0, top, (B, rows)).astype(np.uint8)
    c[c.sum(axis=1) == 0, 0] = 1
    return c


def bootstrap(x, y, theta, dt, cx, cy, ordered=False):
    """The reference: x, y float32 values representable in ``dt``, theta float32 [L x D] (rounded by SR.sliced), cx [B x n] and cy [B x m]
    -> dict with values [B + 1 x L] (row 0 the sets as given), totals [B + 1 x 2], boot and boot_max [B] and the observed statistics"""
    ax, ay = with_observed(cx), with_observed(cy)
    runs = [SR.sliced(np.repeat(x, ax[b], axis=0), np.repeat(y, ay[b], axis=0), theta, dt, ordered) for b in range(len(ax))]
    return {"values": np.array([r["values"] for r in runs]), "q": runs[0]["q"],
            "totals": np.array([[int(ax[b].sum()), int(ay[b].sum())] for b in range(len(ax))], dtype=np.int64),
            "boot": np.array([r["sw2_squared"] for r in runs[1:]]), "boot_max": np.array([r["max_sliced"] for r in runs[1:]]),
            "sw2_squared": runs[0]["sw2_squared"], "std_error": runs[0]["std_error"], "max_sliced": runs[0]["max_sliced"],
            "max_index": runs[0]["max_index"]}


def intervals(boot, observed, confidence=0.95):
    """-> dict of boot_mean, boot_std (ddof = 1), bias, ci_percentile and ci_basic of the replicates ``boot`` around ``observed``"""
    boot = np.asarray(boot, dtype=np.float64)
    lo, hi = np.quantile(boot, [(1 - confidence) / 2, (1 + confidence) / 2])
    return {"boot_mean": boot.mean(), "boot_std": boot.std(ddof=1), "bias": boot.mean() - observed, "ci_percentile": (lo, hi),
            "ci_basic": (2 * observed - hi, 2 * observed - lo)}


def difference(boot_i, boot_j, observed_i, observed_j, confidence=0.95):
    """-> dict of diff, diff_observed, ci_diff and prob_closer of two sets' replicates on one baseline"""
    diff = np.asarray(boot_i, dtype=np.float64) - np.asarray(boot_j, dtype=np.float64)
    lo, hi = np.quantile(diff, [(1 - confidence) / 2, (1 + confidence) / 2])
    return {"diff": diff, "diff_observed": observed_i - observed_j, "ci_diff": (lo, hi), "prob_closer": np.mean(diff < 0)}
