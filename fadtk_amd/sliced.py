"""The sliced 2-Wasserstein distance between two sets of embedding rows (Rabin et al. 2011; Bonneel et al. 2015): both sets are projected
on L random directions, in one dimension optimal transport is sorting, so W_2^2 per direction is a match of the two step quantile
functions, and the L values are averaged.  A transport distance between the two EMPIRICAL sets, as the Sinkhorn divergence is, but with
no blur, no iterations and no convergence question, on all rows, in O((n + m) log) per direction; its Monte-Carlo error over the
directions has an honest estimate (``std_error``).  Everything runs in one GPU call (``fad_sliced_wasserstein``, include/fad_hip.h;
DESIGN.md 4.17): projections on the matrix cores, a segmented radix sort, the match in float64.

    python -m fadtk_amd.sliced <model> <baseline_dir> <eval_dir> [csv] [--projections 512] [--seed 0] [-w N]

The directions are ``sliced_directions(D, projections, seed)``: standard normal, NOT normalised (the library divides each direction's
value by its squared length).  ``fad_scale`` = D x ``sw2_squared`` reads beside FAD's mean term: a pure translation delta gives
E W_l = |delta|^2 / D.  The CSV gets one row per call under CSV_HEADER.  Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.
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


def check_csv(target: PathLike) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not CSV_HEADER."""
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline()
        if first.rstrip("\r\n") != CSV_HEADER.rstrip("\n"):
            raise ValueError(f"{target} has the header {first.strip()!r}; a row of the sliced Wasserstein distance goes under "
                             f"{CSV_HEADER.strip()!r}: write it to another file")


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


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.sliced", description="Sliced 2-Wasserstein distance between the embedding rows of a "
                       "baseline and an evaluation directory of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the result to this CSV")
    p.add_argument("--projections", type=int, default=512, help="random directions (default 512)")
    p.add_argument("--seed", type=int, default=0, help="seed of the directions (default 0)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    try:
        check_params(a.projections, a.seed)
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]
    if a.csv:
        check_csv(a.csv)                                  # before any work: a CSV with another header is refused

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    sw = SlicedWasserstein(model, audio_load_worker=a.workers, load_model=False, projections=a.projections, seed=a.seed)
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
