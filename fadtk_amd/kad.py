"""Kernel Audio Distance (KAD): the unbiased Gaussian-kernel MMD^2 between two sets of embedding rows.

An addition beyond fadtk's FAD (Chung et al. 2025, "KAD: No More FAD! An Effective and Efficient Evaluation Metric for Audio
Generation"), computed by the same library on the same embedding caches:

    k(a, b) = exp(-|a - b|^2 / (2 sigma^2))
    MMD^2   = mean_{i != j} k(x_i, x_j) + mean_{i != j} k(y_i, y_j) - 2 mean_{i, j} k(x_i, y_j)

x is the baseline, y the evaluation set: all frames of all cached ``.npy`` files of a directory, concatenated (the rows FAD feeds
to ``calc_embd_statistics``).  sigma defaults to the median pairwise distance within the baseline
(``np.median(scipy.spatial.distance.pdist(x))``).  The score is reported as ``scale * MMD^2`` (scale 1 by default) and may be
negative: the estimator is unbiased.

    python -m fadtk_amd.kad <model> <baseline_dir> <eval_dir> [csv] [--bandwidth S] [--scale F] [-w N]
"""
from __future__ import annotations

import logging
import time
from argparse import ArgumentParser
from pathlib import Path
from typing import Optional

import numpy as np

from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,kad,bandwidth,scale,time\n"


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def calc_kernel_audio_distance(x, y, bandwidth: Optional[float] = None, scale: float = 1.0, device: int = 0, details: bool = False):
    """scale * MMD^2 between the rows of x (baseline) and y, on the GPU (``fad_kad``).  numpy arrays or torch CUDA tensors of
    float16 / bfloat16 / float32.  ``details=True`` returns (value, dict of the fad_kad_result fields)."""
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"KAD needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"KAD: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"KAD needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    from . import hip
    res = hip.kad(x, y, bandwidth=bandwidth, device=device)
    value = float(scale) * res["mmd2"]
    return (value, res) if details else value


class KernelAudioDistance:
    """KAD between two directories of audio, over the embedding caches FrechetAudioDistance writes and reads."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0):
        from .fad import FrechetAudioDistance
        self.ml = ml
        self.device_index = device
        self.fad = FrechetAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def load_rows(self, path: PathLike) -> np.ndarray:
        p = Path(path)
        bundled = Path(__file__).parent / "stats" / (str(path).lower() + ".npz")
        if p.is_file() or (not p.exists() and bundled.exists()):
            raise ValueError(f"KAD needs the embedding rows of a dataset directory; {path} is a statistics file (mu, cov only)")
        if not p.is_dir():
            raise ValueError(f"KAD: {path} is not a directory")
        return self.fad.load_embeddings(p)

    def score(self, baseline: PathLike, eval: PathLike, bandwidth: Optional[float] = None, scale: float = 1.0, details: bool = False):
        x = self.load_rows(baseline)
        y = self.load_rows(eval)
        if x.dtype == np.float64:             # embedding caches are float32 / float16; a float64 cache is narrowed explicitly
            x = x.astype(np.float32)
        if y.dtype == np.float64:
            y = y.astype(np.float32)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_kernel_audio_distance(x, y, bandwidth=bandwidth, scale=scale, device=self.device_index, details=details)


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.kad", description="Kernel Audio Distance (unbiased Gaussian-kernel MMD^2) "
                       "between two directories of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the result to this CSV")
    p.add_argument("--bandwidth", type=float, default=None, help="kernel sigma (default: median pairwise distance of the baseline)")
    p.add_argument("--scale", type=float, default=1.0, help="factor applied to the reported MMD^2 (default 1)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    model = models[a.model]

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    kad = KernelAudioDistance(model, audio_load_worker=a.workers, load_model=False)
    value, res = kad.score(a.baseline, a.eval, bandwidth=a.bandwidth, scale=a.scale, details=True)
    if a.csv:
        target = Path(a.csv)
        target.parent.mkdir(parents=True, exist_ok=True)
        if not target.is_file():
            target.write_text(CSV_HEADER)
        with open(target, "a") as fh:
            fh.write(f"{model.name},{a.baseline},{a.eval},{value!r},{res['bandwidth']!r},{a.scale!r},{time.time()}\n")
        log.info(f"KAD score appended to {a.csv}")
    log.info(f"The KAD {model.name} score between {a.baseline} and {a.eval} is: {value} (bandwidth {res['bandwidth']})")
    print(value)


if __name__ == "__main__":
    main()
