"""The Sinkhorn divergence between two sets of embedding rows: the transport distance between the two EMPIRICAL sets, where FAD is the
2-Wasserstein distance between two Gaussians fitted to them (Genevay et al. 2018; Feydy et al. 2019).  With the cost |a - b|^2 / 2 and
the regularisation epsilon = blur^2,

    S = OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2  >= 0,   0 only for equal sets,
    S -> W_2^2 / 2 as blur -> 0,   S -> |mean x - mean y|^2 / 2 as blur -> infinity,

so ``w2_estimate`` = sqrt(2 S) reads on FAD's scale.  The dual potentials say row by row, and so song by song, where S comes from:
S = mean(pot_x) + mean(pot_y).  Everything runs in one fused GPU call (``fad_sinkhorn``, include/fad_hip.h): a fixed
number of Sinkhorn iterations, each half-step one pass of KAD's matrix-core main loop, no n x m matrix ever stored.

    python -m fadtk_amd.sinkhorn <model> <baseline_dir> <eval_dir> [csv] [--blur B | --blur-factor F] [--iterations L] [--indiv]
                                 [--max-rows N --seed S] [-w N]

The default blur is 0.25 x the median pairwise distance of the baseline (the distance KAD's default bandwidth uses).  ``--max-rows N``
takes N rows of each set that has more (``subsample_rows``).  The CSV gets one row per call under CSV_HEADER; with ``--indiv`` it is a
per-file CSV under INDIV_CSV_HEADER instead (every row of every file kept; ``--max-rows`` then thins the baseline only).  Embeddings are
cached as ``python -m fadtk_amd.kad`` caches them.  ``marginal_error`` says how far the fixed number of iterations is from
convergence; above MARGINAL_WARN a warning is logged.
"""
from __future__ import annotations

import logging
import math
from argparse import ArgumentParser
from pathlib import Path
from typing import Optional, Union

import numpy as np

from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,n,m,divergence,w2_estimate,blur,epsilon,iterations,marginal_error,max_rows,seed\n"
INDIV_CSV_HEADER = "file,rows,mean_potential,share\n"
DEFAULT_BLUR_FACTOR = 0.25
MAX_ITERATIONS = 100000
MARGINAL_WARN = 1e-3


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def _check(x, y):
    """the shapes, or a ValueError -- before any file is read or the native library is loaded -> (n, m)"""
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"Sinkhorn divergence needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"Sinkhorn divergence: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[1] < 1 or sx[1] > 2048:
        raise ValueError(f"Sinkhorn divergence: D = {sx[1]} is outside 1 .. 2048")
    if sx[0] < 1 or sy[0] < 1:
        raise ValueError(f"Sinkhorn divergence needs at least 1 row per set, got {sx[0]} and {sy[0]}")
    return int(sx[0]), int(sy[0])


def check_params(blur=None, blur_factor=DEFAULT_BLUR_FACTOR, iterations=100):
    """-> (blur or None, blur_factor, iterations), or a ValueError: ``blur`` and a ``blur_factor`` of one's own together, a value that is
    not finite and > 0, iterations outside 1 .. 100000."""
    if blur is not None and blur_factor != DEFAULT_BLUR_FACTOR:
        raise ValueError("Sinkhorn divergence: give blur or blur_factor, not both")
    for name, v in (("blur", blur), ("blur_factor", blur_factor)):
        if v is not None and not (float(v) > 0 and math.isfinite(float(v))):
            raise ValueError(f"Sinkhorn divergence: {name} must be finite and > 0, got {v}")
    if blur is None and blur_factor is None:
        raise ValueError("Sinkhorn divergence: blur_factor must be finite and > 0, got None")
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"Sinkhorn divergence: iterations must be an integer in 1 .. {MAX_ITERATIONS}, got {iterations!r}")
    return (None if blur is None else float(blur)), float(blur_factor), int(iterations)


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


def subsample_rows(rows, max_rows: Optional[int], seed: int = 0):
    """``rows`` itself when it has at most ``max_rows`` rows (or ``max_rows`` is None), else the rows
    ``sorted(numpy.random.default_rng(seed).choice(len(rows), max_rows, replace=False))`` -- a generator of its own per set, so a seed
    pins the rows of a set whatever the other set is."""
    if max_rows is None or len(rows) <= max_rows:
        return rows
    if int(max_rows) != max_rows or max_rows < 1:
        raise ValueError(f"Sinkhorn divergence: max_rows must be an integer >= 1, got {max_rows}")
    return rows[np.sort(np.random.default_rng(seed).choice(len(rows), int(max_rows), replace=False))]


def calc_sinkhorn_divergence(x, y, blur: Optional[float] = None, blur_factor: float = DEFAULT_BLUR_FACTOR, iterations: int = 100,
                             potentials: bool = False, device: int = 0) -> dict:
    """The debiased Sinkhorn divergence of y against the baseline x (``fad_sinkhorn``) with the cost |a - b|^2 / 2 and epsilon = blur^2;
    ``blur=None``: blur_factor x the median pairwise distance of x (needs 2 rows of x).  ``iterations`` is fixed: no early stop.  numpy
    arrays or torch CUDA tensors of float16 / bfloat16 / float32; mixed dtypes go to float32.  -> dict: ``divergence``, ``ot_xy``,
    ``ot_xx``, ``ot_yy``, ``blur`` (= sqrt(epsilon)), ``epsilon``, ``marginal_error`` (the largest of the three problems' L1 errors of
    the row marginal), ``iterations``, ``n``, ``m``, ``w2_estimate`` (= sqrt(2 max(divergence, 0))) and, with ``potentials``, the
    float64 arrays ``pot_x`` [n], ``pot_y`` [m] (divergence = mean(pot_x) + mean(pot_y)), ``f`` [n] and ``g`` [m]."""
    n, m = _check(x, y)
    blur, blur_factor, iterations = check_params(blur, blur_factor, iterations)
    if blur is None and n < 2:
        raise ValueError("Sinkhorn divergence: the default blur comes from the median pairwise distance of x, which needs 2 rows; pass blur")
    from . import hip
    x, y = _one_dtype(x, y)
    if blur is not None:
        epsilon = blur * blur
    elif blur_factor == DEFAULT_BLUR_FACTOR:
        epsilon = None                                     # the library's own default: no second pass over x for the median
    else:
        median = hip.kad_median_distance(x, device=device)
        if not median > 0:
            raise ValueError("Sinkhorn divergence: the median pairwise distance of x is 0 -- are all its rows identical?  Pass blur")
        epsilon = (blur_factor * median) ** 2
    res = hip.sinkhorn(x, y, epsilon=epsilon, iterations=iterations, device=device, potentials=potentials)
    out = {"divergence": res["divergence"], "ot_xy": res["ot_xy"], "ot_xx": res["ot_xx"], "ot_yy": res["ot_yy"],
           "blur": math.sqrt(res["epsilon"]), "epsilon": res["epsilon"],
           "marginal_error": max(res["marginal_error"], res["marginal_error_xx"], res["marginal_error_yy"]),
           "iterations": res["iterations"], "n": res["n"], "m": res["m"], "w2_estimate": math.sqrt(2.0 * max(res["divergence"], 0.0))}
    if potentials:
        out.update(pot_x=res["pot_x"], pot_y=res["pot_y"], f=res["f"], g=res["g"])
    return out


def warn_if_not_converged(res: dict) -> bool:
    """Log a warning when ``marginal_error`` of a calc_sinkhorn_divergence result is above MARGINAL_WARN -> whether it did."""
    if res["marginal_error"] > MARGINAL_WARN:
        log.warning(f"Sinkhorn divergence: after {res['iterations']} iterations the row marginals are still off by "
                    f"{res['marginal_error']:.3g} (L1); the value is not converged -- use more iterations (--iterations) or a larger "
                    f"blur (--blur / --blur-factor; this run used blur {res['blur']:.6g})")
        return True
    return False


def _check_header(target: PathLike, header: str) -> None:
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline()
        if first.rstrip("\r\n") != header.rstrip("\n"):
            raise ValueError(f"{target} has the header {first.strip()!r}; a row of the Sinkhorn divergence goes under "
                             f"{header.strip()!r}: write it to another file")


def check_csv(target: PathLike, indiv: bool = False) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not CSV_HEADER (INDIV_CSV_HEADER with ``indiv``)."""
    _check_header(target, INDIV_CSV_HEADER if indiv else CSV_HEADER)


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


def csv_row(model: str, baseline, eval_dir, res: dict, max_rows=None, seed=None) -> str:
    """One CSV row (no line end) of a calc_sinkhorn_divergence result under CSV_HEADER."""
    return (f"{model},{baseline},{eval_dir},{res['n']},{res['m']},{res['divergence']!r},{res['w2_estimate']!r},{res['blur']!r},"
            f"{res['epsilon']!r},{res['iterations']},{res['marginal_error']!r},{'' if max_rows is None else max_rows},"
            f"{'' if max_rows is None or seed is None else seed}")


class SinkhornDivergence:
    """The Sinkhorn divergence between two directories of audio, over the embedding caches FrechetAudioDistance writes and reads."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0, blur: Optional[float] = None,
                 blur_factor: float = DEFAULT_BLUR_FACTOR, iterations: int = 100, max_rows: Optional[int] = None, seed: int = 0):
        self.blur, self.blur_factor, self.iterations = check_params(blur, blur_factor, iterations)
        if max_rows is not None and (int(max_rows) != max_rows or max_rows < 1):
            raise ValueError(f"Sinkhorn divergence: max_rows must be an integer >= 1, got {max_rows}")
        from .kad import KernelAudioDistance
        self.ml = ml
        self.device_index = device
        self.max_rows, self.seed = max_rows, seed
        self.kad = KernelAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def _calc(self, x, y, potentials: bool = False) -> dict:
        if x.dtype != y.dtype or x.dtype == np.float64:          # float64 caches and mixed dtypes go to float32
            x, y = x.astype(np.float32), y.astype(np.float32)
        res = calc_sinkhorn_divergence(x, y, blur=self.blur, blur_factor=self.blur_factor, iterations=self.iterations,
                                       potentials=potentials, device=self.device_index)
        warn_if_not_converged(res)
        return res

    def score(self, baseline: PathLike, eval_dir: PathLike) -> dict:
        """calc_sinkhorn_divergence of ``eval_dir`` against ``baseline``, each set thinned to ``max_rows`` rows (subsample_rows)."""
        x = subsample_rows(self.kad.load_rows(baseline), self.max_rows, self.seed)
        y = subsample_rows(self.kad.load_rows(eval_dir), self.max_rows, self.seed)
        return self._calc(x, y)

    def score_individual(self, baseline: PathLike, eval_dir: PathLike, csv_name: Union[Path, str]) -> Path:
        """What every file of ``eval_dir`` adds to the divergence, from ONE call over all their rows: a CSV under INDIV_CSV_HEADER with,
        per file, its row count, the mean of pot_y over its rows, and its share  rows x mean / m  of the divergence (the shares sum to
        mean(pot_y), the evaluation side's part of S), sorted by share, largest first.  Files whose embedding is missing, unreadable,
        empty or of another D are logged and dropped; ``max_rows`` thins the baseline only.  A ``str`` name goes under
        data/sinkhorn-individual/<model>/; an existing CSV is left as it is (one with another header is a ValueError)."""
        csv = Path(csv_name)
        if isinstance(csv_name, str):
            csv = Path("data") / "sinkhorn-individual" / self.ml.name / csv_name
        check_csv(csv, indiv=True)
        if csv.exists():
            log.info(f"CSV file {csv} already exists, exiting...")
            return csv
        x = subsample_rows(self.kad.load_rows(baseline), self.max_rows, self.seed)
        keep = []
        for f in sorted(Path(eval_dir).glob("*.*")):
            try:
                e = np.asarray(self.kad.fad.read_embedding_file(f))
            except Exception as err:      # noqa: BLE001
                log.error(f"Sinkhorn divergence: the embedding of {f} could not be read using model {self.ml.name}: {err}")
                continue
            if e.ndim != 2 or e.shape[1] != x.shape[1] or e.shape[0] < 1:
                log.error(f"Embedding of {f} has shape {e.shape}; expected [>= 1, {x.shape[1]}]")
                continue
            keep.append((f, e))
        if not keep:
            raise ValueError(f"Sinkhorn divergence: no usable embedding file in {eval_dir}")
        dtype = np.result_type(*(e.dtype for _, e in keep))
        y = np.concatenate([e.astype(dtype, copy=False) for _, e in keep])
        res = self._calc(x, y, potentials=True)
        lines, at = [], 0
        for f, e in keep:
            mean = float(np.mean(res["pot_y"][at:at + len(e)]))
            lines.append((str(f).replace(",", "_"), len(e), mean, len(e) * mean / len(y)))
            at += len(e)
        lines.sort(key=lambda r: -r[3])
        csv.parent.mkdir(parents=True, exist_ok=True)
        csv.write_text(INDIV_CSV_HEADER + "".join(f"{f},{r},{mean!r},{share!r}\n" for f, r, mean, share in lines))
        return csv


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.sinkhorn", description="Sinkhorn divergence (debiased entropic optimal transport, cost "
                       "|a - b|^2 / 2) between the embedding rows of a baseline and an evaluation directory of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the result to this CSV (--indiv: write the per-file CSV here)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--blur", type=float, default=None, help="blur = sqrt(epsilon), in the units of the embedding distances")
    g.add_argument("--blur-factor", type=float, default=None, help="blur as a factor of the baseline's median pairwise distance "
                   f"(default {DEFAULT_BLUR_FACTOR})")
    p.add_argument("--iterations", type=int, default=100, help="Sinkhorn iterations, fixed (default 100)")
    p.add_argument("--indiv", action="store_true", help="per-file shares of the divergence into the CSV")
    p.add_argument("--max-rows", type=int, default=None, help="take this many rows of a set that has more")
    p.add_argument("--seed", type=int, default=0, help="seed of --max-rows (default 0)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    try:
        check_params(a.blur, DEFAULT_BLUR_FACTOR if a.blur_factor is None else a.blur_factor, a.iterations)
        if a.max_rows is not None and a.max_rows < 1:
            raise ValueError(f"--max-rows must be >= 1, got {a.max_rows}")
        if a.indiv and not a.csv:
            raise ValueError("--indiv needs the csv argument")
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]
    if a.csv:
        check_csv(a.csv, indiv=a.indiv)                   # before any work: a CSV with another header is refused

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    sd = SinkhornDivergence(model, audio_load_worker=a.workers, load_model=False, blur=a.blur,
                            blur_factor=DEFAULT_BLUR_FACTOR if a.blur_factor is None else a.blur_factor, iterations=a.iterations,
                            max_rows=a.max_rows, seed=a.seed)
    if a.indiv:
        out = sd.score_individual(a.baseline, a.eval, Path(a.csv))
        log.info(f"Per-file shares of the Sinkhorn divergence {model.name} of {a.eval} against {a.baseline} written to {out}")
        return
    res = sd.score(a.baseline, a.eval)
    log.info(f"The Sinkhorn divergence {model.name} between {a.baseline} and {a.eval} is: {res['divergence']} (blur {res['blur']}, "
             f"W2 estimate {res['w2_estimate']}, marginal error {res['marginal_error']:.3g} after {res['iterations']} iterations)")
    print(f"{res['divergence']!r}")
    if a.csv:
        append_csv(a.csv, csv_row(model.name, a.baseline, a.eval, res, a.max_rows, a.seed))
        log.info(f"Sinkhorn divergence appended to {a.csv}")


if __name__ == "__main__":
    main()
