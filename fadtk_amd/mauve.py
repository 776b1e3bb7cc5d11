"""MAUVE (Pillutla et al. 2021) and PRD curves (Sajjadi et al. 2018) between two sets of embedding rows: the baseline and the evaluation
rows are pooled and quantised into K cells by Lloyd's k-means, and the two cell histograms P (baseline) and Q (evaluation) are compared
-- along the divergence frontier (``mauve``, the area under it) and as a precision / recall curve (``f_beta``, ``f_beta_inv``), the
distribution-level partner of the k-NN precision and recall of ``fadtk_amd.prdc``.  The histograms themselves say which regions of the
baseline the evaluation set does not reach and where it piles up (``--cells``).

The k-means runs in one GPU call per restart (``fad_kmeans``, include/fad_hip.h): the assignment is the fused
nearest-row pass on the matrix cores, the update a deterministic float64 mean, the loop stays on the device.  Everything after the
histograms is float64 numpy on K numbers.

    python -m fadtk_amd.mauve <model> <baseline_dir> <eval_dir> [mauve.csv] [--clusters K] [--iterations 100] [--redo 5] [--seed 0]
                              [--scale 5] [--max-rows N] [--cells cells.csv] [-w N]

Seeding: restart r starts from K distinct pooled rows, ``np.random.default_rng([seed, r]).choice(N, K, replace=False)`` sorted
ascending; the restart with the smallest final inertia wins (ties: the smaller r).  ``--max-rows N`` thins each set as
``fadtk_amd.sinkhorn.subsample_rows`` does.  The CSV gets one row per call under CSV_HEADER; ``--cells`` writes one row per cell under
CELLS_CSV_HEADER, the cells the evaluation set misses first.  Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.
PCA and L2 normalisation before the quantisation are the caller's: pass reduced or normalised rows.
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
CSV_HEADER = ("model,baseline,eval,n,m,mauve,f_beta,f_beta_inv,clusters,inertia,iterations,converged,empty_clusters,redo,seed,scale,"
              "max_rows\n")
CELLS_CSV_HEADER = "cell,baseline_rows,eval_rows,p,q,log_ratio\n"
MAX_CLUSTERS = 65536
PRD_ANGLES = 1001
PRD_BETA = 8.0


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check_params(clusters=None, iterations=100, redo=5, seed=0, scale=5.0, points=25):
    """-> (clusters, iterations, redo, seed, scale, points), or a ValueError: clusters None or an integer in 1 .. 65536, iterations an
    integer >= 0, redo an integer >= 1, seed an integer >= 0, scale finite and > 0, points an integer >= 2."""
    if clusters is not None and (not _is_int(clusters) or not 1 <= int(clusters) <= MAX_CLUSTERS):
        raise ValueError(f"MAUVE: clusters must be an integer in 1 .. {MAX_CLUSTERS}, got {clusters!r}")
    if not _is_int(iterations) or int(iterations) < 0:
        raise ValueError(f"MAUVE: iterations must be an integer >= 0, got {iterations!r}")
    if not _is_int(redo) or int(redo) < 1:
        raise ValueError(f"MAUVE: redo must be an integer >= 1, got {redo!r}")
    if not _is_int(seed) or int(seed) < 0:
        raise ValueError(f"MAUVE: seed must be an integer >= 0, got {seed!r}")
    if isinstance(scale, bool) or not (float(scale) > 0 and math.isfinite(float(scale))):
        raise ValueError(f"MAUVE: scale must be finite and > 0, got {scale!r}")
    if not _is_int(points) or int(points) < 2:
        raise ValueError(f"MAUVE: points must be an integer >= 2, got {points!r}")
    return (None if clusters is None else int(clusters)), int(iterations), int(redo), int(seed), float(scale), int(points)


def default_clusters(n: int, m: int) -> int:
    """MAUVE's usual K: a tenth of the smaller set, at least 2, at most 65 536."""
    return min(MAX_CLUSTERS, max(2, min(int(n), int(m)) // 10))


def seed_rows(n_rows: int, clusters: int, seed: int = 0, restart: int = 0) -> np.ndarray:
    """The pooled rows restart ``restart`` takes as its init: ``np.random.default_rng([seed, restart]).choice(n_rows, clusters,
    replace=False)``, sorted ascending."""
    return np.sort(np.random.default_rng([int(seed), int(restart)]).choice(int(n_rows), int(clusters), replace=False))


def _check_sets(sets):
    """the shapes of 1 .. 8 row sets, or a ValueError -- before any file is read or the native library is loaded -> (rows per set, D)"""
    shapes = [_shape_of(s) for s in sets]
    if not 1 <= len(shapes) <= 8:
        raise ValueError(f"k-means takes 1 .. 8 row sets, got {len(shapes)}")
    for s in shapes:
        if len(s) != 2:
            raise ValueError(f"k-means needs 2-D row matrices, got shape {s}")
        if s[1] != shapes[0][1]:
            raise ValueError(f"k-means: the sets have different dimensions ({shapes[0][1]} and {s[1]})")
        if s[0] < 1:
            raise ValueError("k-means needs at least 1 row per set")
    if not 1 <= shapes[0][1] <= 2048:
        raise ValueError(f"k-means: D = {shapes[0][1]} is outside 1 .. 2048")
    return [int(s[0]) for s in shapes], int(shapes[0][1])


def _gather_rows(sets, rows: np.ndarray) -> np.ndarray:
    """the pooled rows ``rows`` (ascending) of ``sets`` as float32 [len(rows), D]"""
    out, start = [], 0
    for s in sets:
        n = int(s.shape[0])
        sel = rows[(rows >= start) & (rows < start + n)] - start
        if len(sel):
            part = s[sel]
            part = part.float().cpu().numpy() if type(part).__module__.split(".")[0] == "torch" else np.asarray(part, dtype=np.float32)
            out.append(part.astype(np.float32, copy=False))
        start += n
    return np.ascontiguousarray(np.concatenate(out, 0))


def calc_kmeans(x, clusters: int, iterations: int = 100, redo: int = 1, seed: int = 0, init=None, device: int = 0) -> dict:
    """Lloyd's k-means (``fad_kmeans``) of the rows ``x`` -- one frame matrix, or a list of up to 8 that are pooled in the given order
    without a copy; numpy arrays or torch tensors of one dtype (float16 / bfloat16 / float32) -- into ``clusters`` cells.  Restart r of
    ``redo`` starts from the pooled rows ``seed_rows(N, clusters, seed, r)`` cast to float32; the restart with the smallest final
    inertia wins, ties to the smaller r.  ``init`` [clusters, D] (float32) replaces the seeding (one run).  -> the dict of
    ``hip.kmeans`` (centroids, labels, counts, dist2, inertia, inertia_trace, iterations, converged, changed_last, empty_clusters, n, k)
    plus ``restart`` (the winner, None with ``init``) and ``inertias`` (every restart's final inertia)."""
    _, iterations, redo, seed, _, _ = check_params(clusters, iterations, redo, seed)
    if clusters is None:
        raise ValueError("k-means: clusters must be given")
    sets = [x] if hasattr(x, "shape") else list(x)
    rows, d = _check_sets(sets)
    N = sum(rows)
    if clusters > N:
        raise ValueError(f"k-means: clusters = {clusters} needs at least {clusters} pooled rows, got {N}")
    if init is not None:
        init = np.asarray(init, dtype=np.float32)
        if init.shape != (clusters, d):
            raise ValueError(f"k-means: init must be [{clusters}, {d}], got shape {init.shape}")
    from . import hip
    if init is not None:
        out = hip.kmeans(sets, init, iterations=iterations, device=device)
        out.update(restart=None, inertias=np.array([out["inertia"]]))
        return out
    best, inertias = None, []
    for r in range(redo):
        got = hip.kmeans(sets, _gather_rows(sets, seed_rows(N, clusters, seed, r)), iterations=iterations, device=device)
        inertias.append(got["inertia"])
        if best is None or got["inertia"] < best["inertia"]:
            best = got
            best["restart"] = r
    best["inertias"] = np.array(inertias)
    return best


def _kl(a: np.ndarray, b: np.ndarray) -> float:
    """KL(a || b) = sum over a_i > 0 of a_i ln(a_i / b_i)"""
    keep = a > 0
    with np.errstate(divide="ignore"):
        return float(np.sum(a[keep] * np.log(a[keep] / b[keep])))


def divergence_curve(p, q, scale: float = 5.0, points: int = 25) -> np.ndarray:
    """The divergence frontier of the histograms p and q -> [points + 2, 2]: (exp(-s KL(q || r)), exp(-s KL(p || r))) for
    r = lam p + (1 - lam) q, lam in linspace(1e-6, 1 - 1e-6, points), then (0, 1) and (1, 0).  1 - lam_i is taken as the grid's own
    mirror value lam_{points - 1 - i} (the same number up to rounding), so that swapping p and q gives the mirrored curve to the bit."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    out = []
    grid = np.linspace(1e-6, 1 - 1e-6, points)
    for lam, mirror in zip(grid, grid[::-1]):
        r = lam * p + mirror * q
        out.append((math.exp(-scale * _kl(q, r)), math.exp(-scale * _kl(p, r))))
    out += [(0.0, 1.0), (1.0, 0.0)]
    return np.array(out, dtype=np.float64)


def _area(xs: np.ndarray, ys: np.ndarray) -> float:
    """the trapezoid area of ys over xs sorted ascending (ties: ys ascending, so that swapping the two histograms walks the mirror
    image of the same polygon)"""
    order = np.lexsort((ys, xs))
    xs, ys = xs[order], ys[order]
    return float(np.sum(0.5 * (xs[1:] - xs[:-1]) * (ys[1:] + ys[:-1])))


def mauve_area(curve: np.ndarray) -> float:
    """The larger of the two trapezoid areas of a divergence curve: y over sorted x, and x over sorted y."""
    return max(_area(curve[:, 0], curve[:, 1]), _area(curve[:, 1], curve[:, 0]))


def prd_curve(p, q, angles: int = PRD_ANGLES):
    """-> (precision, recall) [angles] of Sajjadi et al.: lam_i = tan(theta_i), theta = linspace(1e-10, pi / 2 - 1e-10, angles),
    precision_i = sum_k min(lam_i p_k, q_k), recall_i = precision_i / lam_i.  p is the baseline's histogram, q the evaluation set's."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    lam = np.tan(np.linspace(1e-10, math.pi / 2 - 1e-10, angles))
    precision = np.minimum(lam[:, None] * p[None, :], q[None, :]).sum(1)
    return precision, precision / lam


def f_beta_max(precision, recall, beta: float) -> float:
    """max over the curve of F_beta = (1 + beta^2) p r / (beta^2 p + r + 1e-10)"""
    b2 = beta * beta
    return float(np.max((1 + b2) * precision * recall / (b2 * precision + recall + 1e-10)))


def histogram_metrics(p_counts, q_counts, scale: float = 5.0, points: int = 25) -> dict:
    """Everything after the histograms, from the two cell counts (baseline, evaluation): float64 numpy on K numbers -> dict of
    ``mauve``, ``divergence_curve``, ``prd_precision``, ``prd_recall``, ``f_beta`` (beta = 8), ``f_beta_inv`` (beta = 1/8), ``p_hist``
    and ``q_hist`` (the cell frequencies)."""
    p_counts, q_counts = np.asarray(p_counts, dtype=np.float64), np.asarray(q_counts, dtype=np.float64)
    if p_counts.shape != q_counts.shape or p_counts.ndim != 1 or p_counts.sum() <= 0 or q_counts.sum() <= 0:
        raise ValueError("MAUVE: the two histograms must be 1-D, of one length and not empty")
    p, q = p_counts / p_counts.sum(), q_counts / q_counts.sum()
    curve = divergence_curve(p, q, scale, points)
    precision, recall = prd_curve(p, q)
    return {"mauve": mauve_area(curve), "divergence_curve": curve, "prd_precision": precision, "prd_recall": recall,
            "f_beta": f_beta_max(precision, recall, PRD_BETA), "f_beta_inv": f_beta_max(precision, recall, 1.0 / PRD_BETA),
            "p_hist": p, "q_hist": q}


def calc_mauve(x, y, clusters: Optional[int] = None, iterations: int = 100, redo: int = 5, seed: int = 0, scale: float = 5.0,
               points: int = 25, device: int = 0) -> dict:
    """MAUVE and the PRD curve of y against the baseline x: the pooled rows [x; y] are quantised by ``calc_kmeans`` (``clusters`` None:
    ``default_clusters(n, m)``), P and Q are the cell frequencies of the baseline and the evaluation rows.  numpy arrays or torch
    tensors of float16 / bfloat16 / float32; mixed dtypes go to float32.  -> dict of ``histogram_metrics`` plus ``clusters``,
    ``inertia``, ``iterations``, ``converged``, ``empty_clusters``, ``restart``, ``labels_x`` [n], ``labels_y`` [m], ``n`` and ``m``."""
    clusters, iterations, redo, seed, scale, points = check_params(clusters, iterations, redo, seed, scale, points)
    (n, m), d = _check_sets([x, y])
    if clusters is None:
        clusters = default_clusters(n, m)
    if clusters > n + m:
        raise ValueError(f"MAUVE: clusters = {clusters} needs at least {clusters} pooled rows, got {n + m}")
    from .sliced import _one_dtype
    x, y = _one_dtype(x, y)
    km = calc_kmeans([x, y], clusters, iterations=iterations, redo=redo, seed=seed, device=device)
    labels_x, labels_y = km["labels"][:n], km["labels"][n:]
    out = histogram_metrics(np.bincount(labels_x, minlength=clusters), np.bincount(labels_y, minlength=clusters), scale, points)
    out.update(clusters=clusters, inertia=km["inertia"], iterations=km["iterations"], converged=km["converged"],
               empty_clusters=km["empty_clusters"], restart=km["restart"], labels_x=labels_x, labels_y=labels_y, n=n, m=m)
    return out


def check_csv(target: PathLike, header: str = CSV_HEADER) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not ``header``."""
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline()
        if first.rstrip("\r\n") != header.rstrip("\n"):
            raise ValueError(f"{target} has the header {first.strip()!r}; a row of MAUVE goes under {header.strip()!r}: write it to "
                             f"another file")


def append_csv(target: PathLike, row: str) -> None:
    """Append ``row`` (no line end) to the CSV ``target`` under CSV_HEADER (written when the file is new); a file with another header is
    refused, untouched."""
    check_csv(target)
    target = Path(target)
    target.parent.mkdir(parents=True, exist_ok=True)
    if not target.is_file():
        target.write_text(CSV_HEADER)
    with open(target, "a") as fh:
        fh.write(row + "\n")


def csv_row(model: str, baseline, eval_dir, res: dict, redo: int, seed: int, scale: float, max_rows=None) -> str:
    """One CSV row (no line end) of a calc_mauve result under CSV_HEADER."""
    return (f"{model},{baseline},{eval_dir},{res['n']},{res['m']},{res['mauve']!r},{res['f_beta']!r},{res['f_beta_inv']!r},"
            f"{res['clusters']},{res['inertia']!r},{res['iterations']},{res['converged']},{res['empty_clusters']},{redo},{seed},"
            f"{scale!r},{'' if max_rows is None else max_rows}")


def write_cells_csv(target: PathLike, res: dict) -> int:
    """One row per cell of a calc_mauve result under CELLS_CSV_HEADER: the cell, its baseline and evaluation rows, p, q and
    log_ratio = ln(q / p) (-inf for a cell the evaluation set misses, inf for one the baseline misses, nan for an empty cell), sorted
    by log_ratio ascending -- the cells the evaluation set misses first, those with the most baseline rows leading; empty cells last.
    A file with another header is refused, untouched; one with this header is replaced.  -> the rows written."""
    check_csv(target, CELLS_CSV_HEADER)
    k = int(res["clusters"])
    nx, ny = np.bincount(res["labels_x"], minlength=k), np.bincount(res["labels_y"], minlength=k)
    p, q = res["p_hist"], res["q_hist"]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.log(q / p)
    key = np.where(np.isnan(ratio), np.inf, ratio)
    order = sorted(range(k), key=lambda c: (0 if nx[c] + ny[c] else 1, key[c], -int(nx[c]), c))
    target = Path(target)
    target.parent.mkdir(parents=True, exist_ok=True)
    target.write_text(CELLS_CSV_HEADER + "".join(f"{c},{int(nx[c])},{int(ny[c])},{float(p[c])!r},{float(q[c])!r},{float(ratio[c])!r}\n"
                                                 for c in order))
    return k


class Mauve:
    """MAUVE and the PRD curve between two directories of audio, over the embedding caches FrechetAudioDistance writes and reads."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0, clusters: Optional[int] = None,
                 iterations: int = 100, redo: int = 5, seed: int = 0, scale: float = 5.0, max_rows: Optional[int] = None):
        self.clusters, self.iterations, self.redo, self.seed, self.scale, _ = check_params(clusters, iterations, redo, seed, scale)
        if max_rows is not None and (not _is_int(max_rows) or max_rows < 1):
            raise ValueError(f"MAUVE: max_rows must be an integer >= 1, got {max_rows!r}")
        self.max_rows = max_rows
        from .kad import KernelAudioDistance
        self.ml = ml
        self.device_index = device
        self.kad = KernelAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def score(self, baseline: PathLike, eval_dir: PathLike) -> dict:
        """calc_mauve of the rows of ``eval_dir`` against the rows of ``baseline``, each set thinned to ``max_rows`` rows."""
        from .sinkhorn import subsample_rows
        x = subsample_rows(self.kad.load_rows(baseline), self.max_rows, self.seed)
        y = subsample_rows(self.kad.load_rows(eval_dir), self.max_rows, self.seed)
        if x.dtype != y.dtype or x.dtype == np.float64:          # float64 caches and mixed dtypes go to float32
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_mauve(x, y, clusters=self.clusters, iterations=self.iterations, redo=self.redo, seed=self.seed, scale=self.scale,
                          device=self.device_index)


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.mauve", description="MAUVE and the PRD curve between the embedding rows of a baseline "
                       "and an evaluation directory of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the result to this CSV")
    p.add_argument("--clusters", type=int, default=None, help="cells K (default: a tenth of the smaller set, at least 2)")
    p.add_argument("--iterations", type=int, default=100, help="k-means iterations at most (default 100)")
    p.add_argument("--redo", type=int, default=5, help="k-means restarts; the smallest inertia wins (default 5)")
    p.add_argument("--seed", type=int, default=0, help="seed of the restarts' inits and of --max-rows (default 0)")
    p.add_argument("--scale", type=float, default=5.0, help="MAUVE's scaling constant (default 5)")
    p.add_argument("--max-rows", type=int, default=None, help="take this many rows of a set that has more")
    p.add_argument("--cells", type=str, default=None, help="write one row per cell to this CSV, the cells the eval set misses first")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    try:
        check_params(a.clusters, a.iterations, a.redo, a.seed, a.scale)
        if a.max_rows is not None and a.max_rows < 1:
            raise ValueError(f"--max-rows must be >= 1, got {a.max_rows}")
        if a.csv:                                                       # before any work: a CSV with another header is refused
            check_csv(a.csv)
        if a.cells:
            check_csv(a.cells, CELLS_CSV_HEADER)
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    mv = Mauve(model, audio_load_worker=a.workers, load_model=False, clusters=a.clusters, iterations=a.iterations, redo=a.redo,
               seed=a.seed, scale=a.scale, max_rows=a.max_rows)
    res = mv.score(a.baseline, a.eval)
    log.info(f"MAUVE {model.name} of {a.eval} against {a.baseline}: {res['mauve']} (F_8 {res['f_beta']}, F_1/8 {res['f_beta_inv']}; "
             f"{res['clusters']} cells, {res['empty_clusters']} empty, k-means {res['iterations']} iterations, "
             f"{'converged' if res['converged'] else 'not converged'})")
    print(f"{res['mauve']!r}")
    if a.csv:
        append_csv(a.csv, csv_row(model.name, a.baseline, a.eval, res, a.redo, a.seed, a.scale, a.max_rows))
        log.info(f"MAUVE appended to {a.csv}")
    if a.cells:
        write_cells_csv(a.cells, res)
        log.info(f"Cells saved to {a.cells}")


if __name__ == "__main__":
    main()
