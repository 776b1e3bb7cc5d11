"""The sliced 2-Wasserstein distance between two sets of embedding rows (Rabin et al. 2011; Bonneel et al. 2015): both sets are projected
on L random directions, in one dimension optimal transport is sorting, so W_2^2 per direction is a match of the two step quantile
functions, and the L values are averaged.  A transport distance between the two EMPIRICAL sets, as the Sinkhorn divergence is, but with
no blur, no iterations and no convergence question, on all rows, in O((n + m) log) per direction; its Monte-Carlo error over the
directions has an honest estimate (``std_error``).  Everything runs in one GPU call (``fad_sliced_wasserstein``, include/fad_hip.h;
DESIGN.md 4.17): projections on the matrix cores, a segmented radix sort, the match in float64.

    python -m fadtk_amd.sliced <model> <baseline_dir> <eval_dir> [csv] [--projections 512] [--seed 0] [-w N] [--indiv | --shares]

The directions are ``sliced_directions(D, projections, seed)``: standard normal, NOT normalised (the library divides each direction's
value by its squared length).  ``fad_scale`` = D x ``sw2_squared`` reads beside FAD's mean term: a pure translation delta gives
E W_l = |delta|^2 / D.  The CSV gets one row per call under CSV_HEADER.  Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.

Per song (``--indiv``): every file of the evaluation directory alone against the baseline, all songs in one GPU call
(``fad_sliced_individual``), each with the bits ``calc_sliced_wasserstein(x, song)`` gives: the parameter-free per-song
ranking beside FAD's and KAD's.  The CSV (default ``sliced-individual-results.csv``) gets one row per file under INDIV_CSV_HEADER,
sorted by ``sw2_squared`` descending.

Per-row shares (``--shares``): where the set-level number comes from, on BOTH sides -- every row's share of ``sw2_squared``
(``fad_sliced_shares``, DESIGN.md 4.19: the sort carries the row index, the match keeps every element's cost), summed per file.  The CSV
(default ``sliced-shares.csv``) gets one row per file of both directories under SHARES_CSV_HEADER: ``share`` (the sum of the file's
rows' shares), ``fraction`` (of ``sw2_squared``) and ``lift`` (fraction / the file's fraction of its set's rows: 1 for a file that
carries the distance in proportion to its length); the baseline's files first, each side sorted by ``share`` descending.  A baseline
file with a high lift holds rows the evaluation set does not cover (mode dropping); an evaluation file with one holds rows far from
the baseline.

The two-sample permutation test (``calc_sliced_wasserstein_permutation_test``) and the bootstrap intervals
(``calc_sliced_wasserstein_bootstrap``, ``calc_sliced_wasserstein_bootstrap_compare``, ``bootstrap_counts``) have command
lines of their own: ``python -m fadtk_amd.sliced_permutation`` and ``python -m fadtk_amd.sliced_bootstrap``.
"""
from __future__ import annotations

import logging
import math
from argparse import ArgumentParser
from pathlib import Path
from typing import Optional

import numpy as np

from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,n,m,sw2_squared,sliced_w2,std_error,max_sliced,max_index,fad_scale,projections,seed\n"
INDIV_CSV_HEADER = "file,rows,sw2_squared,sliced_w2,std_error,fad_scale\n"
INDIV_CSV_NAME = "sliced-individual-results.csv"
SHARES_CSV_HEADER = "side,file,rows,share,fraction,lift\n"
SHARES_CSV_NAME = "sliced-shares.csv"
INDIV_BYTES = 4 << 30          # song rows per fad_sliced_individual call at most (a larger set is split: the same bits either way)
MAX_PROJECTIONS = 65536


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def _check(x, y):
    """the shapes, or a ValueError -- before any file is read or the native library is loaded -> (n, m, D)"""
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"sliced Wasserstein needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"sliced Wasserstein: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[1] < 1 or sx[1] > 2048:
        raise ValueError(f"sliced Wasserstein: D = {sx[1]} is outside 1 .. 2048")
    if sx[0] < 1 or sy[0] < 1:
        raise ValueError(f"sliced Wasserstein needs at least 1 row per set, got {sx[0]} and {sy[0]}")
    if sx[0] * sy[0] >= 2 ** 53:
        raise ValueError(f"sliced Wasserstein: n m = {sx[0]} x {sy[0]} is 2^53 or more")
    return int(sx[0]), int(sy[0]), int(sx[1])


def check_params(projections=512, seed=0):
    """-> (projections, seed), or a ValueError: projections not an integer in 1 .. 65536, seed not an integer >= 0."""
    if isinstance(projections, bool) or int(projections) != projections or not 1 <= int(projections) <= MAX_PROJECTIONS:
        raise ValueError(f"sliced Wasserstein: projections must be an integer in 1 .. {MAX_PROJECTIONS}, got {projections!r}")
    if isinstance(seed, bool) or int(seed) != seed or int(seed) < 0:
        raise ValueError(f"sliced Wasserstein: seed must be an integer >= 0, got {seed!r}")
    return int(projections), int(seed)


def sliced_directions(d: int, projections: int = 512, seed: int = 0) -> np.ndarray:
    """The directions of a call: ``np.random.default_rng(seed).standard_normal((projections, d)).astype(np.float32)``."""
    projections, seed = check_params(projections, seed)
    return np.random.default_rng(seed).standard_normal((projections, int(d))).astype(np.float32)


def _one_dtype(x, y):
    from . import hip
    if hip.K._is_torch(x) and hip.K._is_torch(y):
        if x.dtype != y.dtype:
            x, y = x.float(), y.float()
    elif not hip.K._is_torch(x) and not hip.K._is_torch(y):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
    return x, y


def calc_sliced_wasserstein(x, y, projections: int = 512, seed: int = 0, directions=None, per_direction: bool = False,
                            device: int = 0) -> dict:
    """The sliced 2-Wasserstein distance of y against the baseline x (``fad_sliced_wasserstein``) over ``directions`` [L x D] (float32,
    not normalised; None: ``sliced_directions(D, projections, seed)``).  numpy arrays or torch CUDA tensors of float16 / bfloat16 /
    float32; mixed dtypes go to float32.  -> dict: ``sw2_squared`` (the mean over the directions of W_l), ``sliced_w2`` (its square
    root), ``std_error`` (std(W_l, ddof = 1) / sqrt(L); NaN for one direction), ``max_sliced`` and ``max_index`` (the largest W_l and
    its direction), ``fad_scale`` (= D x sw2_squared), ``n``, ``m``, ``projections``, ``seed`` (None with directions of one's own) and,
    with ``per_direction``, the float64 array ``values`` [L]."""
    n, m, d = _check(x, y)
    if directions is None:
        directions = sliced_directions(d, projections, seed)
    else:
        from .hip import sliced_directions_array
        directions = sliced_directions_array(directions, d)
        seed = None
    from . import hip
    x, y = _one_dtype(x, y)
    res = hip.sliced_wasserstein(x, y, directions, device=device, values=per_direction)
    out = {"sw2_squared": res["sw2_squared"], "sliced_w2": math.sqrt(max(res["sw2_squared"], 0.0)), "std_error": res["std_error"],
           "max_sliced": res["max_sliced"], "max_index": res["max_index"], "fad_scale": d * res["sw2_squared"], "n": res["n"],
           "m": res["m"], "projections": res["projections"], "seed": seed}
    if per_direction:
        out["values"] = res["values"]
    return out


def calc_sliced_wasserstein_individual(x, songs, projections: int = 512, seed: int = 0, directions=None, per_direction: bool = False,
                                       device: int = 0, max_bytes: int = INDIV_BYTES) -> dict:
    """The sliced 2-Wasserstein distance of every song [m_s x D] alone against the baseline x, every song in one GPU call
    (``fad_sliced_individual``): song s gets the bits of ``calc_sliced_wasserstein(x, songs[s])`` with the same directions.  numpy arrays
    or torch CUDA tensors of float16 / bfloat16 / float32; mixed dtypes go to float32; a song without rows is allowed and gives NaN.
    -> dict of float64 arrays [S] ``sw2_squared``, ``sliced_w2``, ``std_error``, ``max_sliced``, ``max_index`` (-1 where there is
    none), ``fad_scale``, ``rows`` and ``status`` (0, FAD_ERR_TOO_FEW_ROWS or FAD_ERR_NOT_FINITE: NaN values), plus ``n``,
    ``projections``, ``seed`` (None with directions of one's own) and, with ``per_direction``, ``values`` [S x L].  Songs whose rows
    together exceed ``max_bytes`` go in several calls of whole songs: with the same directions that cannot change a bit."""
    sx = _shape_of(x)
    songs = list(songs)
    shapes = [_shape_of(y) for y in songs]
    if len(sx) != 2:
        raise ValueError(f"sliced Wasserstein needs a 2-D baseline, got shape {sx}")
    if sx[1] < 1 or sx[1] > 2048:
        raise ValueError(f"sliced Wasserstein: D = {sx[1]} is outside 1 .. 2048")
    if sx[0] < 1:
        raise ValueError(f"sliced Wasserstein needs at least 1 baseline row, got {sx[0]}")
    if not songs:
        raise ValueError("sliced Wasserstein per song needs at least 1 song")
    for sh in shapes:
        if len(sh) != 2 or (sh[0] > 0 and sh[1] != sx[1]):
            raise ValueError(f"sliced Wasserstein: a song of shape {sh} against a baseline of D = {sx[1]}")
        if sx[0] * sh[0] >= 2 ** 53:
            raise ValueError(f"sliced Wasserstein: n m = {sx[0]} x {sh[0]} is 2^53 or more")
    n, d = int(sx[0]), int(sx[1])
    if directions is None:
        directions = sliced_directions(d, projections, seed)
    else:
        from .hip import sliced_directions_array
        directions = sliced_directions_array(directions, d)
        seed = None
    from . import hip
    torch_in = hip.K._is_torch(x)
    if torch_in:
        import torch
        if len({x.dtype, *(y.dtype for y in songs)}) > 1:
            x, songs = x.float(), [y.float() for y in songs]
        cat = lambda parts: torch.cat(parts, 0) if parts else x[:0]                  # noqa: E731
    else:
        x = np.asarray(x)
        songs = [np.asarray(y) for y in songs]
        if len({x.dtype, *(y.dtype for y in songs)}) > 1:
            x, songs = x.astype(np.float32), [y.astype(np.float32) for y in songs]
        cat = lambda parts: np.concatenate(parts, 0) if parts else x[:0]             # noqa: E731
    row_bytes = max(1, d * (x.element_size() if torch_in else x.itemsize))
    S, L = len(songs), directions.shape[0]
    res = {k: np.full(S, np.nan) for k in ("sw2_squared", "std_error", "max_sliced")}
    res["max_index"] = np.full(S, -1.0)
    status = np.zeros(S)
    values = np.full((S, L), np.nan) if per_direction else None
    s0 = 0
    while s0 < S:                                 # batches of whole songs under the byte budget (at least one song each)
        s1, size = s0, 0
        while s1 < S and (s1 == s0 or size + shapes[s1][0] * row_bytes <= max_bytes):
            size += shapes[s1][0] * row_bytes
            s1 += 1
        part = [y.reshape(-1, d) if shapes[s0 + i][0] == 0 else y for i, y in enumerate(songs[s0:s1])]
        off = np.concatenate([[0], np.cumsum([shapes[s][0] for s in range(s0, s1)], dtype=np.int64)])
        r = hip.sliced_individual(x, cat(part), off, directions, device=device, values=per_direction)
        for k in res:
            res[k][s0:s1] = r[k]
        status[s0:s1] = r["status"]
        if per_direction:
            values[s0:s1] = r["values"]
        s0 = s1
    out = {"sw2_squared": res["sw2_squared"], "sliced_w2": np.sqrt(np.maximum(res["sw2_squared"], 0.0)), "std_error": res["std_error"],
           "max_sliced": res["max_sliced"], "max_index": res["max_index"], "fad_scale": d * res["sw2_squared"],
           "rows": np.array([float(sh[0]) for sh in shapes]), "status": status, "n": n, "projections": int(L), "seed": seed}
    if per_direction:
        out["values"] = values
    return out


def _check_offsets(offsets, rows: int, name: str) -> np.ndarray:
    """-> ``offsets`` as int64 [F + 1], or a ValueError: not 1-D, fewer than 2 entries, not starting at 0, decreasing, or not ending at
    ``rows``"""
    off = np.asarray(offsets)
    if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"sliced Wasserstein shares: {name} must be a 1-D sequence of F + 1 integer row indices, F >= 1")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != rows or np.any(np.diff(off) < 0):
        raise ValueError(f"sliced Wasserstein shares: {name} must start at 0, never decrease and end at the {rows} rows of its set")
    return off


def file_sums(share: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """-> float64 [F]: the sum of ``share[offsets[f]:offsets[f + 1]]`` per file (0 for a file without rows)"""
    return np.array([float(np.sum(share[offsets[f]:offsets[f + 1]])) for f in range(len(offsets) - 1)], dtype=np.float64)


def file_lift(file_share: np.ndarray, offsets: np.ndarray, sw2_squared: float) -> np.ndarray:
    """-> float64 [F]: (file share / sw2_squared) / (file rows / set rows); NaN for a file without rows or at sw2_squared == 0"""
    rows = np.diff(offsets).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (file_share / sw2_squared) / (rows / float(offsets[-1]))


def calc_sliced_wasserstein_shares(x, y, projections: int = 512, seed: int = 0, directions=None, x_offsets=None, y_offsets=None,
                                   device: int = 0) -> dict:
    """``calc_sliced_wasserstein`` of y against the baseline x (the same dict, the same bits) plus every row's share of ``sw2_squared``
    on both sides (``fad_sliced_shares``): the float64 arrays ``share_x`` [n] and ``share_y`` [m].  Each sums to ``sw2_squared`` up to
    rounding; n x ``share_x[i]`` is row i's mean squared one-dimensional displacement under the optimal one-dimensional matchings.
    Rows with equal projections are ranked by row index: shares are discontinuous at such ties.  Inputs, dtypes and ValueErrors as
    ``calc_sliced_wasserstein``.  With ``x_offsets`` [F + 1] (row f0 of file f is ``x_offsets[f]``; starts at 0, ends at n) the dict also
    has ``file_share_x`` [F] (the sum of the file's rows' shares) and ``file_lift_x`` = (file share / sw2_squared) / (file rows / n);
    ``y_offsets`` likewise gives ``file_share_y`` and ``file_lift_y``."""
    n, m, d = _check(x, y)
    if x_offsets is not None:
        x_offsets = _check_offsets(x_offsets, n, "x_offsets")
    if y_offsets is not None:
        y_offsets = _check_offsets(y_offsets, m, "y_offsets")
    if directions is None:
        directions = sliced_directions(d, projections, seed)
    else:
        from .hip import sliced_directions_array
        directions = sliced_directions_array(directions, d)
        seed = None
    from . import hip
    x, y = _one_dtype(x, y)
    res = hip.sliced_shares(x, y, directions, device=device)
    out = {"sw2_squared": res["sw2_squared"], "sliced_w2": math.sqrt(max(res["sw2_squared"], 0.0)), "std_error": res["std_error"],
           "max_sliced": res["max_sliced"], "max_index": res["max_index"], "fad_scale": d * res["sw2_squared"], "n": res["n"],
           "m": res["m"], "projections": res["projections"], "seed": seed, "share_x": res["share_x"], "share_y": res["share_y"]}
    for side, off in (("x", x_offsets), ("y", y_offsets)):
        if off is not None:
            out[f"file_share_{side}"] = file_sums(out[f"share_{side}"], off)
            out[f"file_lift_{side}"] = file_lift(out[f"file_share_{side}"], off, out["sw2_squared"])
    return out


MAX_PERMUTATIONS = 65536


def check_permutations(permutations) -> int:
    """-> permutations, or a ValueError: not an integer in 1 .. 65536."""
    if isinstance(permutations, bool) or int(permutations) != permutations or not 1 <= int(permutations) <= MAX_PERMUTATIONS:
        raise ValueError(f"sliced Wasserstein permutation test takes 1 .. {MAX_PERMUTATIONS} permutations, got {permutations!r}")
    return int(permutations)


def _check_labels(labels, N: int) -> None:
    """the shape of given labellings, or a ValueError -- before the native library is loaded: [P, N] 0/1 (bool / uint8) or
    [P, ceil(N / 32)] packed 32-bit words, P in 1 .. 65536"""
    if not hasattr(labels, "dtype"):
        labels = np.asarray(labels)
    sh = tuple(labels.shape)
    words = (N + 31) // 32
    kind = str(labels.dtype).replace("torch.", "")
    if len(sh) != 2:
        raise ValueError(f"sliced Wasserstein permutation test: labels must be 2-D, got shape {sh}")
    want = N if kind in ("bool", "uint8") else words
    if sh[1] != want:
        raise ValueError(f"sliced Wasserstein permutation test: labels of shape {sh} and dtype {kind}; 0/1 labels have N = {N} columns, "
                         f"packed 32-bit words ceil(N / 32) = {words}")
    check_permutations(sh[0])


def calc_sliced_wasserstein_permutation_test(x, y, permutations: int = 1000, projections: int = 512, seed: int = 0, directions=None,
                                             labels=None, return_labels: bool = False, per_labelling: bool = False,
                                             device: int = 0) -> dict:
    """Is y distinguishable from the baseline x at all?  The two-sample permutation test with the sliced 2-Wasserstein distance as its
    statistic (``fad_sliced_permutation_test``): no bandwidth, no pair pass.  The pooled rows are projected and sorted
    once per direction; each of ``permutations`` random relabellings that hold the sizes at n and m splits the sorted projections into
    its two sorted groups, and the statistic is recomputed -- all labellings in one GPU call.  Labellings come from
    ``kad.random_labellings`` (the same seed gives the KAD and k-NN tests' labellings) unless ``labels`` gives them (bool / uint8 [P, N]
    or packed words [P, ceil(N / 32)]); the directions as ``calc_sliced_wasserstein`` (``seed`` seeds both).  -> everything
    ``calc_sliced_wasserstein(x, y)`` returns, with its bits, plus ``p_value`` = (1 + #{null >= sw2_squared}) / (P + 1), ``p_value_max``
    (the same with the largest slice: sensitive to a difference that lives in few directions), ``null`` and ``null_max`` [P],
    ``permutations``, ``seed`` (None when labels or directions are given) and, on request, ``values`` [P + 1, L] (row 0 the observed
    labelling) and ``labels``."""
    n, m, d = _check(x, y)
    given = directions is not None or labels is not None
    if directions is None:
        directions = sliced_directions(d, projections, seed)
    else:
        from .hip import sliced_directions_array
        directions = sliced_directions_array(directions, d)
    if labels is None:
        permutations = check_permutations(permutations)
        from .kad import random_labellings
        labels = random_labellings(n, m, permutations, seed=seed, device=device)
    else:
        _check_labels(labels, n + m)
    from . import hip
    x, y = _one_dtype(x, y)
    res = hip.sliced_permutation_test(x, y, labels, directions, device=device, per_labelling=per_labelling)
    out = {"sw2_squared": res["sw2_squared"], "sliced_w2": math.sqrt(max(res["sw2_squared"], 0.0)), "std_error": res["std_error"],
           "max_sliced": res["max_sliced"], "max_index": res["max_index"], "fad_scale": d * res["sw2_squared"], "n": res["n"],
           "m": res["m"], "projections": res["projections"], "seed": None if given else seed, "p_value": res["p_value"],
           "p_value_max": res["p_value_max"], "null": res["null"], "null_max": res["null_max"], "permutations": int(res["permutations"])}
    if per_labelling:
        out["values"] = res["values"]
    if return_labels:
        out["labels"] = labels
    return out


MAX_REPLICATES = 65536


def check_bootstrap(replicates=1000, confidence=0.95):
    """-> (replicates, confidence), or a ValueError: replicates not an integer in 1 .. 65536, confidence not strictly between 0 and 1."""
    if isinstance(replicates, bool) or int(replicates) != replicates or not 1 <= int(replicates) <= MAX_REPLICATES:
        raise ValueError(f"sliced Wasserstein bootstrap takes 1 .. {MAX_REPLICATES} replicates, got {replicates!r}")
    if isinstance(confidence, bool) or not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"sliced Wasserstein bootstrap: confidence must lie strictly between 0 and 1, got {confidence!r}")
    return int(replicates), float(confidence)


def bootstrap_counts(sizes, replicates: int = 1000, seed: int = 0, stream: int = 0) -> np.ndarray:
    """The resamples of one set as row counts -> uint8 [replicates x rows].  ``sizes`` is the row count of every resampling unit:
    ``np.ones(n, int)`` resamples rows, ``np.diff(offsets)`` resamples files (all rows of a file move together, because the frames of
    one song are not independent).  Units without rows are left out of the pool.  With F units in the pool and
    ``rng = np.random.default_rng([seed, stream])``, for each replicate in order: the units' counts are
    ``np.bincount(rng.integers(0, F, size=F), minlength=F)`` and a row's count is its unit's.  A count above 255 is a ValueError.
    ``stream`` 0 is the baseline's, 1 + k the k-th evaluation set's: the baseline's resamples are the same whichever set they meet,
    which is what makes comparisons of sets paired."""
    sizes = np.asarray(sizes)
    if sizes.ndim != 1 or (sizes.size and not np.all(sizes == np.floor(sizes))) or np.any(sizes < 0):
        raise ValueError("sliced Wasserstein bootstrap: sizes must be a 1-D sequence of row counts >= 0")
    sizes = sizes.astype(np.int64)
    replicates, _ = check_bootstrap(replicates)
    _, seed = check_params(1, seed)
    if isinstance(stream, bool) or int(stream) != stream or int(stream) < 0:
        raise ValueError(f"sliced Wasserstein bootstrap: stream must be an integer >= 0, got {stream!r}")
    pool = np.flatnonzero(sizes > 0)
    F = int(pool.size)
    if F < 1:
        raise ValueError("sliced Wasserstein bootstrap: no resampling unit has a row")
    rng = np.random.default_rng([seed, int(stream)])
    out = np.zeros((replicates, int(sizes.sum())), dtype=np.uint8)
    for b in range(replicates):
        units = np.bincount(rng.integers(0, F, size=F), minlength=F)
        if units.max() > 255:
            raise ValueError(f"sliced Wasserstein bootstrap: replicate {b} draws one unit {int(units.max())} times (at most 255)")
        out[b] = np.repeat(units, sizes[pool]).astype(np.uint8)
    return out


def bootstrap_statistics(boot, observed: float, confidence: float = 0.95) -> dict:
    """The interval statistics of the replicates ``boot`` [B] around the plug-in value ``observed`` -> dict: ``boot_mean``, ``boot_std``
    (ddof = 1; NaN for one replicate), ``bias`` = boot_mean - observed, ``ci_percentile`` = np.quantile(boot, [(1 - c) / 2, (1 + c) / 2])
    and ``ci_basic`` = (2 observed - q_hi, 2 observed - q_lo), both as tuples of floats."""
    boot = np.asarray(boot, dtype=np.float64)
    _, c = check_bootstrap(1, confidence)
    lo, hi = (float(v) for v in np.quantile(boot, [(1 - c) / 2, (1 + c) / 2]))
    mean = float(np.mean(boot))
    return {"boot_mean": mean, "boot_std": float(np.std(boot, ddof=1)) if boot.size > 1 else float("nan"), "bias": mean - observed,
            "ci_percentile": (lo, hi), "ci_basic": (2 * observed - hi, 2 * observed - lo)}


def bootstrap_difference(boot_i, boot_j, observed_i: float, observed_j: float, confidence: float = 0.95) -> dict:
    """Two evaluation sets on one baseline, replicate by replicate (the baseline's resamples shared) -> dict: ``diff`` [B] =
    boot_i - boot_j, ``diff_observed``, ``ci_diff`` (the percentile interval of diff) and ``prob_closer`` (the share of replicates with
    diff < 0: set i closer to the baseline than set j)."""
    diff = np.asarray(boot_i, dtype=np.float64) - np.asarray(boot_j, dtype=np.float64)
    _, c = check_bootstrap(1, confidence)
    lo, hi = (float(v) for v in np.quantile(diff, [(1 - c) / 2, (1 + c) / 2]))
    return {"diff": diff, "diff_observed": observed_i - observed_j, "ci_diff": (lo, hi), "prob_closer": float(np.mean(diff < 0))}


def _bootstrap_side(counts, offsets, rows: int, name: str, replicates: int, seed: int, stream: int):
    """one side's counts and unit: given counts (uint8 [B x rows], checked), else drawn over the files of ``offsets`` or over the rows"""
    off = _check_offsets(offsets, rows, f"{name}_offsets") if offsets is not None else None
    unit = "row" if off is None else "file"
    if counts is not None:
        from .hip import sliced_bootstrap_counts_array
        return sliced_bootstrap_counts_array(counts, rows, f"counts_{name}"), unit
    return bootstrap_counts(np.ones(rows, dtype=np.int64) if off is None else np.diff(off), replicates, seed, stream), unit


def calc_sliced_wasserstein_bootstrap(x, y, replicates: int = 1000, confidence: float = 0.95, projections: int = 512, seed: int = 0,
                                      directions=None, x_offsets=None, y_offsets=None, counts_x=None, counts_y=None,
                                      per_replicate: bool = False, device: int = 0, y_stream: int = 1) -> dict:
    """How certain is the sliced 2-Wasserstein distance of y against the baseline x?  The bootstrap over the ROWS' sampling variability
    (``std_error`` is only the Monte-Carlo error over the directions): both sets are resampled with replacement ``replicates`` times and
    the distance is recomputed on every resample, all in one GPU call (``fad_sliced_bootstrap``, DESIGN.md 4.21: both sets are sorted
    once per direction and every resample expands the sorted arrays by its row counts).  With ``x_offsets`` / ``y_offsets`` [F + 1] whole
    files are resampled on that side, which is right when the frames of a song are not independent; without, rows.  Counts come from
    ``bootstrap_counts`` (stream 0 for x, ``y_stream`` for y) unless ``counts_x`` / ``counts_y`` (uint8 [B x rows]) give them, as
    ``labels`` does in the permutation test.
    -> everything ``calc_sliced_wasserstein(x, y)`` returns, with its bits, plus ``boot`` and ``boot_max`` [B] (each the bits of
    ``calc_sliced_wasserstein`` on ``np.repeat`` of the rows by the counts), ``boot_mean``, ``boot_std`` (ddof = 1), ``bias`` =
    boot_mean - sw2_squared, ``ci_percentile``, ``ci_basic``, ``replicates``, ``confidence``, ``unit`` (``unit_x``, ``unit_y``: "file"
    where offsets were given, else "row"; ``unit`` is "file" when either is) and ``seed`` (None when counts or directions are given);
    with ``per_replicate`` also ``values`` [B + 1, L], ``totals`` [B + 1, 2], ``counts_x`` and ``counts_y``.
    The plug-in SW2^2 is biased UPWARD: two samples of one distribution give a positive value of order 1/n + 1/m, and resampling adds
    that bias once more, so ``boot`` sits above ``sw2_squared`` as ``sw2_squared`` sits above the population value.  ``bias`` estimates
    it, ``ci_basic`` (reflected about the plug-in value) removes it to first order, ``ci_percentile`` does not and lies too high."""
    n, m, d = _check(x, y)
    replicates, confidence = check_bootstrap(replicates, confidence)
    given = directions is not None or counts_x is not None or counts_y is not None
    cx, unit_x = _bootstrap_side(counts_x, x_offsets, n, "x", replicates, seed, 0)
    cy, unit_y = _bootstrap_side(counts_y, y_offsets, m, "y", replicates, seed, y_stream)
    if cx.shape[0] != cy.shape[0]:
        raise ValueError(f"sliced Wasserstein bootstrap: counts_x has {cx.shape[0]} replicates, counts_y has {cy.shape[0]}")
    if directions is None:
        directions = sliced_directions(d, projections, seed)
    else:
        from .hip import sliced_directions_array
        directions = sliced_directions_array(directions, d)
    from . import hip
    x, y = _one_dtype(x, y)
    res = hip.sliced_bootstrap(x, y, cx, cy, directions, device=device, per_replicate=per_replicate)
    out = {"sw2_squared": res["sw2_squared"], "sliced_w2": math.sqrt(max(res["sw2_squared"], 0.0)), "std_error": res["std_error"],
           "max_sliced": res["max_sliced"], "max_index": res["max_index"], "fad_scale": d * res["sw2_squared"], "n": res["n"],
           "m": res["m"], "projections": res["projections"], "seed": None if given else seed, "boot": res["boot"],
           "boot_max": res["boot_max"], **bootstrap_statistics(res["boot"], res["sw2_squared"], confidence),
           "replicates": int(res["replicates"]), "confidence": confidence, "unit_x": unit_x, "unit_y": unit_y,
           "unit": "file" if "file" in (unit_x, unit_y) else "row"}
    if per_replicate:
        out.update(values=res["values"], totals=res["totals"], counts_x=cx, counts_y=cy)
    return out


def calc_sliced_wasserstein_bootstrap_compare(x, ys, replicates: int = 1000, confidence: float = 0.95, projections: int = 512,
                                              seed: int = 0, directions=None, x_offsets=None, ys_offsets=None,
                                              per_replicate: bool = False, device: int = 0) -> dict:
    """Is evaluation set A really closer to the baseline x than set B?  One ``calc_sliced_wasserstein_bootstrap`` per set of ``ys``, all
    with the same directions and the same resamples of the baseline (stream 0 of ``bootstrap_counts``; set k draws from stream 1 + k),
    so replicate b of every set meets the same resampled baseline and the comparison is paired.  ``ys_offsets``: None, or one offsets
    array (or None) per set.  -> dict: ``sets`` (the per-set dicts) and ``pairs`` {(i, j): dict for i < j} with ``diff`` [B] =
    boot_i - boot_j, ``diff_observed``, ``ci_diff`` (the percentile interval of diff) and ``prob_closer`` (the share of replicates in
    which set i is closer to the baseline than set j), plus ``replicates``, ``confidence`` and ``seed``.
    The upward bias of the plug-in SW2^2 (see ``calc_sliced_wasserstein_bootstrap``) largely cancels in the difference, because the
    baseline's part of it is shared; it does NOT cancel when the evaluation sets differ much in size (the 1/m terms differ): compare
    sets of similar size, or read ``bias`` of both."""
    ys = list(ys)
    if not ys:
        raise ValueError("sliced Wasserstein bootstrap compare needs at least 1 evaluation set")
    offs = list(ys_offsets) if ys_offsets is not None else [None] * len(ys)
    if len(offs) != len(ys):
        raise ValueError(f"sliced Wasserstein bootstrap compare: {len(ys)} sets, {len(offs)} offsets")
    replicates, confidence = check_bootstrap(replicates, confidence)
    shapes = [_check(x, y) for y in ys]                        # every set before any work
    n, d = shapes[0][0], shapes[0][2]
    own = directions is not None
    if own:
        from .hip import sliced_directions_array
        directions = sliced_directions_array(directions, d)
    else:
        directions = sliced_directions(d, projections, seed)
    cx, _ = _bootstrap_side(None, x_offsets, n, "x", replicates, seed, 0)
    sets = []
    for k, (y, off) in enumerate(zip(ys, offs)):
        r = calc_sliced_wasserstein_bootstrap(x, y, replicates=replicates, confidence=confidence, directions=directions,
                                              x_offsets=x_offsets, y_offsets=off, counts_x=cx, per_replicate=per_replicate,
                                              device=device, seed=seed, y_stream=1 + k)
        r["seed"] = None if own else seed
        sets.append(r)
    pairs = {(i, j): bootstrap_difference(sets[i]["boot"], sets[j]["boot"], sets[i]["sw2_squared"], sets[j]["sw2_squared"], confidence)
             for i in range(len(sets)) for j in range(i + 1, len(sets))}
    return {"sets": sets, "pairs": pairs, "replicates": replicates, "confidence": confidence, "seed": None if own else seed}


def check_csv(target: PathLike, header: str = CSV_HEADER) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not ``header`` (CSV_HEADER; INDIV_CSV_HEADER for the per-song file)."""
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline()
        if first.rstrip("\r\n") != header.rstrip("\n"):
            raise ValueError(f"{target} has the header {first.strip()!r}; a row of the sliced Wasserstein distance goes under "
                             f"{header.strip()!r}: write it to another file")


def indiv_csv_row(file, res: dict, s: int) -> str:
    """One CSV row (no line end) of song ``s`` of a calc_sliced_wasserstein_individual result under INDIV_CSV_HEADER."""
    return (f"{str(file).replace(',', '_')},{int(res['rows'][s])},{float(res['sw2_squared'][s])!r},{float(res['sliced_w2'][s])!r},"
            f"{float(res['std_error'][s])!r},{float(res['fad_scale'][s])!r}")


def write_indiv_csv(target: PathLike, files, res: dict) -> int:
    """The per-song CSV: INDIV_CSV_HEADER, then one row per file of ``files`` whose status is 0, sorted by ``sw2_squared`` descending
    (ties in the order of ``files``).  A file with another header is refused, untouched; one with this header is replaced.  -> the
    rows written."""
    check_csv(target, INDIV_CSV_HEADER)
    keep = [s for s in range(len(files)) if res["status"][s] == 0]
    keep.sort(key=lambda s: -res["sw2_squared"][s])
    target = Path(target)
    target.parent.mkdir(parents=True, exist_ok=True)
    target.write_text(INDIV_CSV_HEADER + "".join(indiv_csv_row(files[s], res, s) + "\n" for s in keep))
    return len(keep)


def write_shares_csv(target: PathLike, x_files, y_files, res: dict, x_offsets, y_offsets) -> int:
    """The per-file CSV of a calc_sliced_wasserstein_shares result with offsets: SHARES_CSV_HEADER, then one row per file -- the
    baseline's (``side`` = baseline) before the evaluation set's (eval), each side sorted by ``share`` descending (ties in the order of
    the files).  ``fraction`` = share / sw2_squared, ``lift`` as ``file_lift``.  A file with another header is refused, untouched; one
    with this header is replaced.  -> the rows written."""
    check_csv(target, SHARES_CSV_HEADER)
    lines = []
    for side, files, off, k in (("baseline", x_files, x_offsets, "x"), ("eval", y_files, y_offsets, "y")):
        share, lift = res[f"file_share_{k}"], res[f"file_lift_{k}"]
        with np.errstate(divide="ignore", invalid="ignore"):
            fraction = share / res["sw2_squared"]
        for f in sorted(range(len(files)), key=lambda f: -share[f]):
            lines.append(f"{side},{str(files[f]).replace(',', '_')},{int(off[f + 1] - off[f])},{float(share[f])!r},{float(fraction[f])!r},"
                         f"{float(lift[f])!r}\n")
    target = Path(target)
    target.parent.mkdir(parents=True, exist_ok=True)
    target.write_text(SHARES_CSV_HEADER + "".join(lines))
    return len(lines)


def append_csv(target: PathLike, row: str) -> None:
    """Append ``row`` (no line end) to the CSV ``target`` under CSV_HEADER (written when the file is new); a file with another header is
    refused, untouched (check_csv)."""
    check_csv(target)
    target = Path(target)
    target.parent.mkdir(parents=True, exist_ok=True)
    if not target.is_file():
        target.write_text(CSV_HEADER)
    with open(target, "a") as fh:
        fh.write(row + "\n")


def csv_row(model: str, baseline, eval_dir, res: dict) -> str:
    """One CSV row (no line end) of a calc_sliced_wasserstein result under CSV_HEADER."""
    return (f"{model},{baseline},{eval_dir},{res['n']},{res['m']},{res['sw2_squared']!r},{res['sliced_w2']!r},{res['std_error']!r},"
            f"{res['max_sliced']!r},{res['max_index']},{res['fad_scale']!r},{res['projections']},"
            f"{'' if res['seed'] is None else res['seed']}")


class SlicedWasserstein:
    """The sliced Wasserstein distance between two directories of audio, over the embedding caches FrechetAudioDistance writes and reads."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0, projections: int = 512, seed: int = 0):
        self.projections, self.seed = check_params(projections, seed)
        from .kad import KernelAudioDistance
        self.ml = ml
        self.device_index = device
        self.kad = KernelAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def score(self, baseline: PathLike, eval_dir: PathLike, per_direction: bool = False) -> dict:
        """calc_sliced_wasserstein of all rows of ``eval_dir`` against all rows of ``baseline``."""
        x, y = self.kad.load_rows(baseline), self.kad.load_rows(eval_dir)
        if x.dtype != y.dtype or x.dtype == np.float64:          # float64 caches and mixed dtypes go to float32
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_sliced_wasserstein(x, y, projections=self.projections, seed=self.seed, per_direction=per_direction,
                                       device=self.device_index)

    def score_permutation_test(self, baseline: PathLike, eval_dir: PathLike, permutations: int = 1000) -> dict:
        """calc_sliced_wasserstein_permutation_test of all rows of ``eval_dir`` against all rows of ``baseline``: the directions and the
        labellings both from this object's seed."""
        permutations = check_permutations(permutations)
        x, y = self.kad.load_rows(baseline), self.kad.load_rows(eval_dir)
        if x.dtype != y.dtype or x.dtype == np.float64:          # float64 caches and mixed dtypes go to float32
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_sliced_wasserstein_permutation_test(x, y, permutations=permutations, projections=self.projections, seed=self.seed,
                                                        device=self.device_index)

    def score_individual(self, baseline: PathLike, eval_dir: PathLike, csv: PathLike = INDIV_CSV_NAME) -> Path:
        """calc_sliced_wasserstein_individual of every file of ``eval_dir`` against all rows of ``baseline``, written to ``csv`` under
        INDIV_CSV_HEADER, sorted by ``sw2_squared`` descending.  Files whose embedding is missing, unreadable, of another D, empty or not
        finite are logged and dropped, as KAD's are.  A CSV with another header is refused before any work."""
        check_csv(csv, INDIV_CSV_HEADER)
        x = self.kad.load_rows(baseline)
        files = sorted(Path(eval_dir).glob("*.*"))
        keep = []
        for f in files:
            try:
                e = self.kad.fad.read_embedding_file(f)
            except Exception as err:      # noqa: BLE001
                log.error(f"An error occurred calculating the individual sliced Wasserstein distance using model {self.ml.name} on file {f}")
                log.error(err)
                continue
            if e.ndim != 2 or e.shape[1] != x.shape[1]:
                log.error(f"Embedding of {f} has shape {e.shape}; expected [*, {x.shape[1]}]")
            elif e.shape[0] < 1:
                log.error(f"Individual sliced Wasserstein distance of {f} dropped: no frames")
            else:
                keep.append((f, e))
        dts = {x.dtype, *(e.dtype for _, e in keep)}
        if len(dts) > 1 or np.float64 in dts:      # one dtype for the call; float64 caches are narrowed, as score() does
            x, keep = x.astype(np.float32), [(f, e.astype(np.float32)) for f, e in keep]
        csv = Path(csv)
        if not keep:
            write_indiv_csv(csv, [], {"status": [], "sw2_squared": []})
            return csv
        res = calc_sliced_wasserstein_individual(x, [e for _, e in keep], projections=self.projections, seed=self.seed,
                                                 device=self.device_index)
        for (f, _), st in zip(keep, res["status"]):
            if st != 0:
                log.error(f"An error occurred calculating the individual sliced Wasserstein distance using model {self.ml.name} on file "
                          f"{f} (status {int(st)}: {'no frames' if st == -6 else 'non-finite rows'})")
        write_indiv_csv(csv, [f for f, _ in keep], res)
        return csv


    def _embedding_files(self, directory: PathLike, d: Optional[int]) -> list:
        """-> [(file, embedding)] of ``directory`` in sorted order; a file whose embedding is missing, unreadable, not [* x d] (d None:
        the D of the first readable one) or empty is logged and dropped"""
        keep = []
        for f in sorted(Path(directory).glob("*.*")):
            try:
                e = self.kad.fad.read_embedding_file(f)
            except Exception as err:      # noqa: BLE001
                log.error(f"An error occurred calculating the sliced Wasserstein shares using model {self.ml.name} on file {f}")
                log.error(err)
                continue
            if e.ndim != 2 or (d is not None and e.shape[1] != d):
                log.error(f"Embedding of {f} has shape {e.shape}; expected [*, {'D' if d is None else d}]")
            elif e.shape[0] < 1:
                log.error(f"Sliced Wasserstein shares of {f} dropped: no frames")
            else:
                d = e.shape[1]
                keep.append((f, e))
        return keep

    def score_shares(self, baseline: PathLike, eval_dir: PathLike, csv: PathLike = SHARES_CSV_NAME) -> dict:
        """calc_sliced_wasserstein_shares of all rows of ``eval_dir`` against all rows of ``baseline`` with one offset per file, written
        to ``csv`` under SHARES_CSV_HEADER (write_shares_csv) -> the result, with ``x_files`` and ``y_files``.  Files are dropped and
        logged as score_individual drops them; a file with non-finite rows refuses the call, as it does ``score``.  A CSV with another
        header is refused before any work."""
        check_csv(csv, SHARES_CSV_HEADER)
        xs = self._embedding_files(baseline, None)
        if not xs:
            raise ValueError(f"sliced Wasserstein shares: no embedding rows under {baseline}")
        ys = self._embedding_files(eval_dir, xs[0][1].shape[1])
        if not ys:
            raise ValueError(f"sliced Wasserstein shares: no embedding rows under {eval_dir}")
        dts = {e.dtype for _, e in xs + ys}
        cast = (lambda e: e.astype(np.float32)) if len(dts) > 1 or np.float64 in dts else (lambda e: e)
        x, y = np.concatenate([cast(e) for _, e in xs]), np.concatenate([cast(e) for _, e in ys])
        xo = np.concatenate([[0], np.cumsum([len(e) for _, e in xs], dtype=np.int64)])
        yo = np.concatenate([[0], np.cumsum([len(e) for _, e in ys], dtype=np.int64)])
        res = calc_sliced_wasserstein_shares(x, y, projections=self.projections, seed=self.seed, x_offsets=xo, y_offsets=yo,
                                             device=self.device_index)
        res["x_files"], res["y_files"] = [f for f, _ in xs], [f for f, _ in ys]
        write_shares_csv(csv, res["x_files"], res["y_files"], res, xo, yo)
        return res

    def score_bootstrap(self, baseline: PathLike, eval_dirs, replicates: int = 1000, confidence: float = 0.95, rows: bool = False) -> dict:
        """calc_sliced_wasserstein_bootstrap_compare of all rows of every directory of ``eval_dirs`` against all rows of ``baseline`` ->
        its result, with ``x_files`` and, per set, ``files``.  Files are the resampling units (one offset per file, built as
        score_shares builds them) unless ``rows``.  Files are dropped and logged as score_shares drops them; a file with non-finite
        rows refuses the call.  The directions and the resamples both come from this object's seed."""
        replicates, confidence = check_bootstrap(replicates, confidence)
        eval_dirs = list(eval_dirs)
        if not eval_dirs:
            raise ValueError("sliced Wasserstein bootstrap needs at least 1 evaluation directory")
        xs = self._embedding_files(baseline, None)
        if not xs:
            raise ValueError(f"sliced Wasserstein bootstrap: no embedding rows under {baseline}")
        sets = []
        for e in eval_dirs:
            ys = self._embedding_files(e, xs[0][1].shape[1])
            if not ys:
                raise ValueError(f"sliced Wasserstein bootstrap: no embedding rows under {e}")
            sets.append(ys)
        dts = {e.dtype for _, e in xs + [fe for ys in sets for fe in ys]}
        cast = (lambda e: e.astype(np.float32)) if len(dts) > 1 or np.float64 in dts else (lambda e: e)
        offsets = lambda fs: np.concatenate([[0], np.cumsum([len(e) for _, e in fs], dtype=np.int64)])      # noqa: E731
        x = np.concatenate([cast(e) for _, e in xs])
        res = calc_sliced_wasserstein_bootstrap_compare(
            x, [np.concatenate([cast(e) for _, e in ys]) for ys in sets], replicates=replicates, confidence=confidence,
            projections=self.projections, seed=self.seed, x_offsets=None if rows else offsets(xs),
            ys_offsets=None if rows else [offsets(ys) for ys in sets], device=self.device_index)
        res["x_files"] = [f for f, _ in xs]
        for r, ys in zip(res["sets"], sets):
            r["files"] = [f for f, _ in ys]
        return res


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.sliced", description="Sliced 2-Wasserstein distance between the embedding rows of a "
                       "baseline and an evaluation directory of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help=f"append the result to this CSV; with --indiv or --shares: where the per-file rows go "
                   f"(default {INDIV_CSV_NAME} / {SHARES_CSV_NAME})")
    p.add_argument("--projections", type=int, default=512, help="random directions (default 512)")
    p.add_argument("--seed", type=int, default=0, help="seed of the directions (default 0)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    mode = p.add_mutually_exclusive_group()
    mode.add_argument("--indiv", action="store_true", help="one row per file of the eval directory")
    mode.add_argument("--shares", action="store_true", help=f"every file's share of the distance, both directories (default CSV "
                      f"{SHARES_CSV_NAME})")
    a = p.parse_args(argv)
    try:
        check_params(a.projections, a.seed)
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]
    if a.indiv or a.shares:
        a.csv = a.csv or (INDIV_CSV_NAME if a.indiv else SHARES_CSV_NAME)
    if a.csv:                                                           # before any work: a CSV with another header is refused
        check_csv(a.csv, INDIV_CSV_HEADER if a.indiv else SHARES_CSV_HEADER if a.shares else CSV_HEADER)

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    sw = SlicedWasserstein(model, audio_load_worker=a.workers, load_model=False, projections=a.projections, seed=a.seed)
    if a.indiv:
        csv = sw.score_individual(a.baseline, a.eval, a.csv)
        log.info(f"Individual sliced Wasserstein distances {model.name} of {a.eval} against {a.baseline} saved to {csv}")
        return
    if a.shares:
        res = sw.score_shares(a.baseline, a.eval, a.csv)
        log.info(f"Sliced Wasserstein shares {model.name} of {a.eval} against {a.baseline} (SW2^2 = {res['sw2_squared']}) saved to {a.csv}")
        return
    res = sw.score(a.baseline, a.eval)
    log.info(f"The sliced Wasserstein distance {model.name} between {a.baseline} and {a.eval} is: SW2^2 = {res['sw2_squared']} "
             f"+- {res['std_error']:.3g} over {res['projections']} directions (SW2 {res['sliced_w2']}, on FAD's scale {res['fad_scale']}, "
             f"largest slice {res['max_sliced']} at direction {res['max_index']})")
    print(f"{res['sw2_squared']!r}")
    if a.csv:
        append_csv(a.csv, csv_row(model.name, a.baseline, a.eval, res))
        log.info(f"Sliced Wasserstein distance appended to {a.csv}")


if __name__ == "__main__":
    main()
