"""The kernel distance with the polynomial kernel -- "KID" / "KD", the number audio evaluation suites print next to FAD (Binkowski et
al. 2018, Demystifying MMD GANs): the unbiased MMD^2 with k(a, b) = (gamma a.b + coef0)^degree, degree 3, gamma = 1 / D, coef0 = 1,
averaged over many random subsets (usually 100 subsets of 1000 rows) and reported as mean +- std.

Every subset runs in one fused GPU call (``fad_kid_subsets``, include/fad_hip.h): the rows of each subset are gathered
into images of their own and all (x-x, y-y, x-y) blocks go through KAD's matrix-core main loop, no s x s matrix ever stored.  Per
subset  MMD^2 = Sxx / (s (s - 1)) + Syy / (s (s - 1)) - 2 Sxy / s^2  with Sxx, Syy over i != j and Sxy over all s^2 pairs.

    python -m fadtk_amd.kid <model> <baseline_dir> <eval_dir> [csv] [--subsets 100] [--subset-size 1000] [--seed 0]
                            [--degree 3] [--gamma G] [--coef0 1] [--full] [-w N]

``--full`` takes all rows of both sets once instead of subsets (``fad_kid``).  Embeddings are cached as ``python -m fadtk_amd.kad``
caches them.  The CSV gets one row per call under the header
model,baseline,eval,n,m,kid_mean,kid_std,subsets,subset_size,degree,gamma,coef0,seed  (--full: kid_std 0, subsets 0, subset_size 0,
seed empty).
"""
from __future__ import annotations

import logging
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,n,m,kid_mean,kid_std,subsets,subset_size,degree,gamma,coef0,seed\n"


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def _check(x, y):
    """the shapes, or a ValueError -- before any file is read or the native library is loaded -> (n, m)"""
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"kernel distance needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"kernel distance: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"kernel distance needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    return int(sx[0]), int(sy[0])


def _check_subsets(subsets, subset_size, n, m):
    """-> (subsets, subset_size) as ints, or a ValueError: no silent clamp of a subset larger than the smaller set"""
    if int(subsets) != subsets or int(subsets) < 1:
        raise ValueError(f"kernel distance takes at least 1 subset, got {subsets}")
    if int(subset_size) != subset_size or int(subset_size) < 2:
        raise ValueError(f"kernel distance: a subset needs at least 2 rows, got {subset_size}")
    if subset_size > min(n, m):
        raise ValueError(f"kernel distance: subset_size {subset_size} is larger than the smaller set ({min(n, m)} rows); pass a smaller "
                         f"subset_size (or use calc_kernel_distance_full)")
    return int(subsets), int(subset_size)


def subset_indices(n: int, m: int, subsets: int = 100, subset_size: int = 1000, seed: int = 0):
    """The default subsets -> (index_x, index_y), int32 [subsets, subset_size] each.  One ``numpy.random.default_rng(seed)``; for
    q = 0 .. subsets - 1 it draws ``choice(n, subset_size, replace=False)`` and then ``choice(m, subset_size, replace=False)``.  That
    order is part of the interface: a seed pins the result."""
    subsets, subset_size = _check_subsets(subsets, subset_size, n, m)
    rng = np.random.default_rng(seed)
    ix = np.empty((subsets, subset_size), dtype=np.int32)
    iy = np.empty((subsets, subset_size), dtype=np.int32)
    for q in range(subsets):
        ix[q] = rng.choice(n, subset_size, replace=False)
        iy[q] = rng.choice(m, subset_size, replace=False)
    return ix, iy


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


def calc_kernel_distance(x, y, subsets: int = 100, subset_size: int = 1000, degree: int = 3, gamma=None, coef0: float = 1.0,
                         seed: int = 0, indices=None, return_indices: bool = False, device: int = 0) -> dict:
    """The kernel distance of y against the baseline x by the KID protocol (``fad_kid_subsets``): the unbiased polynomial-kernel MMD^2 of
    ``subsets`` random subsets of ``subset_size`` rows of each set.  The subsets come from ``subset_indices(n, m, subsets, subset_size,
    seed)`` unless ``indices=(index_x, index_y)`` gives them (integer [S, s] each; ``subsets``, ``subset_size`` and ``seed`` are then
    not used).  numpy arrays or torch CUDA tensors of float16 / bfloat16 / float32; mixed dtypes go to float32.  ``gamma=None``: 1 / D.
    A ``subset_size`` larger than the smaller set is a ValueError.  -> dict: ``kid_mean``, ``kid_std`` (population, over the subsets),
    ``values`` [S] (float64), ``subsets``, ``subset_size``, ``gamma`` and ``coef0`` (the float32 values used), ``degree`` and, with
    ``return_indices``, ``indices``."""
    from .hip import kid_params
    n, m = _check(x, y)
    degree, g, c = kid_params(degree, gamma, coef0)
    if indices is None:
        ix, iy = subset_indices(n, m, subsets, subset_size, seed)
    else:
        ix, iy = indices
        if len(_shape_of(ix)) != 2 or _shape_of(ix) != _shape_of(iy):
            raise ValueError(f"kernel distance: indices must be two integer [S, s] arrays of one shape, got {_shape_of(ix)} and {_shape_of(iy)}")
        _check_subsets(_shape_of(ix)[0], _shape_of(ix)[1], n, m)
    from . import hip
    x, y = _one_dtype(x, y)
    res = hip.kid_subsets(x, y, ix, iy, degree=degree, gamma=gamma, coef0=coef0, device=device)
    d = _shape_of(x)[1]
    out = {"kid_mean": res["mean"], "kid_std": res["std"], "values": res["mmd2"], "subsets": res["subsets"],
           "subset_size": res["subset_size"], "gamma": float(np.float32(g if g > 0 else 1.0 / d)), "coef0": float(np.float32(c)),
           "degree": degree}
    if return_indices:
        out["indices"] = (ix, iy)
    return out


def calc_kernel_distance_full(x, y, degree: int = 3, gamma=None, coef0: float = 1.0, device: int = 0) -> dict:
    """The unbiased polynomial-kernel MMD^2 over ALL rows of x and y, once (``fad_kid``) -> dict: ``kid`` (= ``mmd2``), ``kxx_mean``,
    ``kyy_mean``, ``kxy_mean``, ``gamma`` and ``coef0`` (the float32 values used), ``degree``, ``n``, ``m``."""
    from .hip import kid_params
    _check(x, y)
    kid_params(degree, gamma, coef0)
    from . import hip
    x, y = _one_dtype(x, y)
    out = hip.kid(x, y, degree=degree, gamma=gamma, coef0=coef0, device=device)
    out["kid"] = out["mmd2"]
    return out


def check_csv(target: PathLike) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not CSV_HEADER: these rows go under their own header."""
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline()
        if first.rstrip("\r\n") != CSV_HEADER.rstrip("\n"):
            raise ValueError(f"{target} has the header {first.strip()!r}; a row of the kernel distance goes under "
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


def csv_row(model: str, baseline, eval_dir, n: int, m: int, res: dict, seed) -> str:
    """One CSV row (no line end) of a calc_kernel_distance or calc_kernel_distance_full result under CSV_HEADER."""
    if "kid_mean" in res:
        return (f"{model},{baseline},{eval_dir},{n},{m},{res['kid_mean']!r},{res['kid_std']!r},{res['subsets']},{res['subset_size']},"
                f"{res['degree']},{res['gamma']!r},{res['coef0']!r},{seed}")
    return f"{model},{baseline},{eval_dir},{n},{m},{res['kid']!r},0.0,0,0,{res['degree']},{res['gamma']!r},{res['coef0']!r},"


class KernelDistance:
    """The polynomial-kernel distance between two directories of audio, over the embedding caches FrechetAudioDistance writes and reads."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0):
        from .kad import KernelAudioDistance
        self.ml = ml
        self.device_index = device
        self.kad = KernelAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def _rows(self, baseline: PathLike, eval_dir: PathLike):
        x = self.kad.load_rows(baseline)
        y = self.kad.load_rows(eval_dir)
        if x.dtype != y.dtype or x.dtype == np.float64:          # float64 caches and mixed dtypes go to float32
            x, y = x.astype(np.float32), y.astype(np.float32)
        return x, y

    def score(self, baseline: PathLike, eval_dir: PathLike, subsets: int = 100, subset_size: int = 1000, degree: int = 3, gamma=None,
              coef0: float = 1.0, seed: int = 0) -> dict:
        """calc_kernel_distance of ``eval_dir`` against ``baseline``, plus ``n`` and ``m``."""
        x, y = self._rows(baseline, eval_dir)
        out = calc_kernel_distance(x, y, subsets=subsets, subset_size=subset_size, degree=degree, gamma=gamma, coef0=coef0, seed=seed,
                                   device=self.device_index)
        out.update(n=len(x), m=len(y))
        return out

    def score_full(self, baseline: PathLike, eval_dir: PathLike, degree: int = 3, gamma=None, coef0: float = 1.0) -> dict:
        """calc_kernel_distance_full of ``eval_dir`` against ``baseline``."""
        x, y = self._rows(baseline, eval_dir)
        return calc_kernel_distance_full(x, y, degree=degree, gamma=gamma, coef0=coef0, device=self.device_index)


def main(argv=None):
    from .cli import _registry, _setup_logging
    from .hip import kid_params
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.kid", description="Kernel distance with the polynomial kernel (KID protocol) between a "
                       "baseline and an evaluation directory of audio, on one GPU: mean and std of the unbiased MMD^2 over random subsets")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the result to this CSV")
    p.add_argument("--subsets", type=int, default=100, help="number of random subsets (default 100)")
    p.add_argument("--subset-size", type=int, default=1000, help="rows of each set per subset (default 1000)")
    p.add_argument("--seed", type=int, default=0, help="seed of the subsets (default 0)")
    p.add_argument("--degree", type=int, default=3, help="degree of the kernel, 1 .. 4 (default 3)")
    p.add_argument("--gamma", type=float, default=None, help="gamma of the kernel (default 1 / D)")
    p.add_argument("--coef0", type=float, default=1.0, help="coef0 of the kernel (default 1)")
    p.add_argument("--full", action="store_true", help="all rows of both sets once instead of subsets")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    try:
        kid_params(a.degree, a.gamma, a.coef0)
        if not a.full:
            _check_subsets(a.subsets, a.subset_size, a.subset_size, a.subset_size)
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]
    if a.csv:
        check_csv(a.csv)                                  # before any work: a CSV with another header is refused

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    kd = KernelDistance(model, audio_load_worker=a.workers, load_model=False)
    if a.full:
        res = kd.score_full(a.baseline, a.eval, degree=a.degree, gamma=a.gamma, coef0=a.coef0)
        log.info(f"The kernel distance {model.name} between {a.baseline} and {a.eval} over all rows is: {res['kid']}")
        print(f"{res['kid']!r}")
    else:
        res = kd.score(a.baseline, a.eval, subsets=a.subsets, subset_size=a.subset_size, degree=a.degree, gamma=a.gamma, coef0=a.coef0,
                       seed=a.seed)
        log.info(f"The kernel distance {model.name} between {a.baseline} and {a.eval} is: {res['kid_mean']} +- {res['kid_std']} "
                 f"({res['subsets']} subsets of {res['subset_size']} rows)")
        print(f"{res['kid_mean']!r} {res['kid_std']!r}")
    if a.csv:
        append_csv(a.csv, csv_row(model.name, a.baseline, a.eval, res["n"], res["m"], res, a.seed))
        log.info(f"Kernel distance appended to {a.csv}")


if __name__ == "__main__":
    main()
