"""Precision, recall, density and coverage: k-nearest-neighbour manifold metrics between two sets of embedding rows.

An addition beyond fadtk (Kynkaanniemi et al. 2019, "Improved Precision and Recall Metric for Assessing Generative Models"; Naeem et
al. 2020, "Reliable Fidelity and Diversity Metrics for Generative Models"), computed by the same library on the same embedding caches
as KAD.  x is the baseline ("real") set, y the evaluation ("fake") set, r_X(i) the distance from x_i to its k-th nearest OTHER row of
x (r_Y(j) likewise within y):

    precision = share of y_j inside some ball B(x_i, r_X(i))         (fidelity)
    recall    = share of x_i inside some ball B(y_j, r_Y(j))         (diversity)
    density   = mean over y_j of #{i : y_j in B(x_i, r_X(i))} / k
    coverage  = share of x_i whose ball B(x_i, r_X(i)) holds some y_j

All comparisons are strict, on squared float32 distances (``fad_prdc``, include/fad_hip.h).  The n x m distance matrix is never
stored: two radius passes and one cross pass on the matrix cores.

    python -m fadtk_amd.prdc <model> <baseline_dir> <eval_dir> [csv] [-k K] [-w N]
"""
from __future__ import annotations

import logging
import time
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

from .kad import KernelAudioDistance
from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,k,precision,recall,density,coverage,time\n"
METRICS = ("precision", "recall", "density", "coverage")


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def calc_precision_recall_density_coverage(x, y, k: int = 5, device: int = 0, details: bool = False) -> dict:
    """Precision, recall, density and coverage of the rows of y against the baseline rows x with k neighbours, on the GPU
    (``fad_prdc``) -> dict of the four values.  numpy arrays or torch CUDA tensors of float16 / bfloat16 / float32.
    ``details=True`` adds per-row arrays: ``radius_x`` [n] and ``radius_y`` [m] (the k-NN distances, float64 square roots of the
    float32 squared radii the comparisons used), ``balls_y`` [m] (baseline balls holding y_j) and ``recalled_x`` / ``covered_x`` [n]
    (bool)."""
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"PRDC needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"PRDC: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if not 1 <= int(k) <= 16:
        raise ValueError(f"PRDC: k must be in 1 .. 16, got {k}")
    if sx[0] <= k or sy[0] <= k:
        raise ValueError(f"PRDC with k = {k} needs more than {k} rows per set, got {sx[0]} and {sy[0]}")
    from . import hip
    res = hip.prdc(x, y, k=k, device=device, details=details)
    out = {key: float(res[key]) for key in METRICS}
    if details:
        out.update(radius_x=np.sqrt(res["radius2_x"].astype(np.float64)), radius_y=np.sqrt(res["radius2_y"].astype(np.float64)),
                   balls_y=res["balls_y"], recalled_x=(res["flags_x"] & 1).astype(bool), covered_x=(res["flags_x"] & 2).astype(bool))
    return out


class PrecisionRecall:
    """Precision, recall, density and coverage between two directories of audio, over the embedding caches FrechetAudioDistance
    writes and reads (the rows KernelAudioDistance.load_rows loads: a statistics ``.npz`` is refused)."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0):
        self.ml = ml
        self.device_index = device
        self.kad = KernelAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def load_rows(self, path: PathLike) -> np.ndarray:
        return self.kad.load_rows(path)

    def score(self, baseline: PathLike, eval: PathLike, k: int = 5, details: bool = False) -> dict:
        x = self.load_rows(baseline)
        y = self.load_rows(eval)
        if x.dtype == np.float64:             # embedding caches are float32 / float16; a float64 cache is narrowed explicitly
            x = x.astype(np.float32)
        if y.dtype == np.float64:
            y = y.astype(np.float32)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_precision_recall_density_coverage(x, y, k=k, device=self.device_index, details=details)


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.prdc", description="k-NN precision, recall, density and coverage between two "
                       "directories of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline (real) dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the result to this CSV")
    p.add_argument("-k", type=int, default=5, help="nearest neighbours per radius, 1 .. 16 (default 5)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    model = models[a.model]

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    res = PrecisionRecall(model, audio_load_worker=a.workers, load_model=False).score(a.baseline, a.eval, k=a.k)
    if a.csv:
        target = Path(a.csv)
        target.parent.mkdir(parents=True, exist_ok=True)
        if not target.is_file():
            target.write_text(CSV_HEADER)
        with open(target, "a") as fh:
            fh.write(f"{model.name},{a.baseline},{a.eval},{a.k},{','.join(repr(res[m]) for m in METRICS)},{time.time()}\n")
        log.info(f"PRDC appended to {a.csv}")
    log.info(f"PRDC {model.name} (k = {a.k}) between {a.baseline} and {a.eval}: "
             + ", ".join(f"{m} {res[m]}" for m in METRICS))
    for m in METRICS:
        print(f"{m} {res[m]!r}")


if __name__ == "__main__":
    main()
