"""Is an evaluation directory distinguishable from the baseline at all -- with no bandwidth to choose?  The leave-one-out
k-nearest-neighbour two-sample test (Schilling 1986, Henze 1988; the classifier two-sample test of Lopez-Paz & Oquab 2017 with a k-NN
classifier; the sample-based metric Xu et al. 2018 found most informative for generative models).

The baseline's and the evaluation set's embedding rows are pooled, and every row is classified by the majority label of its k nearest
OTHER pooled rows (k odd).  The accuracy is near 0.5 when the sets are indistinguishable, above 0.5 when they differ, and well below
0.5 when evaluation rows sit on top of baseline rows.  Its two halves diagnose the failure: an evaluation-row accuracy near 1 with a
low baseline-row accuracy is mode collapse; both low is memorisation.  The neighbour graph does not depend on the labels, so one fused
GPU pass finds it (``fad_nn_test``, include/fad_hip.h) and all P random relabellings are then classified by one bit-parallel kernel:
p_value = (1 + #{null >= observed}) / (P + 1) on the integer counts of correct rows (upper tail: distinguishable), p_value_low the
same with <= (lower tail: memorised).  Both are exact under exchangeability.

    python -m fadtk_amd.nn_test <model> <baseline_dir> <eval_dir> <csv> [-k 1] [-p 1000] [--seed 0] [-w N]

Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.  The CSV gets one row per call under the header
model,baseline,eval,k,n,m,accuracy,accuracy_baseline,accuracy_eval,p_value,p_value_low,permutations,seed.
"""
from __future__ import annotations

import logging
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,k,n,m,accuracy,accuracy_baseline,accuracy_eval,p_value,p_value_low,permutations,seed\n"


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def _check(x, y, k) -> int:
    """the shapes and k, or a ValueError -- before any file is read or the native library is loaded -> k"""
    from .hip import nn_test_k
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"nearest-neighbour test needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"nearest-neighbour test: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"nearest-neighbour test needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    return nn_test_k(k, sx[0] + sy[0])


def _check_permutations(permutations) -> int:
    from .hip import KAD_MAX_PERMUTATIONS
    if not 1 <= int(permutations) <= KAD_MAX_PERMUTATIONS:
        raise ValueError(f"nearest-neighbour test takes 1 .. {KAD_MAX_PERMUTATIONS} permutations, got {permutations}")
    return int(permutations)


def check_csv(target: PathLike) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not CSV_HEADER: these rows go under their own header."""
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline()
        if first.rstrip("\r\n") != CSV_HEADER.rstrip("\n"):
            raise ValueError(f"{target} has the header {first.strip()!r}; a row of the nearest-neighbour test goes under "
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


def calc_nearest_neighbour_test(x, y, k: int = 1, permutations: int = 1000, seed: int = 0, labels=None, return_labels: bool = False,
                                return_graph: bool = False, device: int = 0) -> dict:
    """Is y distinguishable from the baseline x at all?  The leave-one-out k-NN two-sample test on the pooled rows (``fad_nn_test``):
    every pooled row is classified by the majority label of its k nearest other pooled rows (k odd, 1 .. 15), and the count of correct
    rows is compared with its counts under ``permutations`` random relabellings that hold the sizes at n and m.  Labellings come from
    ``kad.random_labellings`` (a seeded generator on the device) unless ``labels`` gives them (bool / uint8 [P, N] or packed words
    [P, ceil(N / 32)]).  numpy arrays or torch CUDA tensors of float16 / bfloat16 / float32; mixed dtypes go to float32.  -> dict:
    ``accuracy``, ``accuracy_baseline`` (of the rows of x), ``accuracy_eval`` (of the rows of y), ``p_value`` (upper tail:
    distinguishable), ``p_value_low`` (lower tail: memorised), ``null`` [P] (float64 accuracies of the random labellings),
    ``null_correct_baseline`` and ``null_correct_eval`` [P] (int64), ``n``, ``m``, ``k``, ``permutations``, ``seed`` (None when labels
    are given) and, with ``return_labels``, ``labels`` (packed words); with ``return_graph``, ``index`` [N, k] (int32, pooled row
    numbering: y_j is row n + j) and ``dist2`` [N, k] (float32), numpy arrays in ascending (d^2, index)."""
    k = _check(x, y, k)
    sx, sy = _shape_of(x), _shape_of(y)
    from . import hip
    if labels is None:
        permutations = _check_permutations(permutations)
        from .kad import random_labellings
        labels = random_labellings(sx[0], sy[0], permutations, seed=seed, device=device)
    else:
        seed = None
    if hip.K._is_torch(x) and hip.K._is_torch(y):
        if x.dtype != y.dtype:                     # one dtype, as calc_kernel_audio_distance_permutation_test casts mixed sets
            x, y = x.float(), y.float()
    elif not hip.K._is_torch(x) and not hip.K._is_torch(y):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
    res = hip.nn_test(x, y, labels, k=k, device=device, return_graph=return_graph)
    n, m = int(res["n"]), int(res["m"])
    out = {"accuracy": res["accuracy"], "accuracy_baseline": res["accuracy_x"], "accuracy_eval": res["accuracy_y"],
           "p_value": res["p_value"], "p_value_low": res["p_value_low"],
           "null": (res["null_correct_x"] + res["null_correct_y"]).astype(np.float64) / float(n + m),
           "null_correct_baseline": res["null_correct_x"], "null_correct_eval": res["null_correct_y"], "n": n, "m": m, "k": int(res["k"]),
           "permutations": int(len(res["null_correct_x"])), "seed": seed}
    if return_labels:
        out["labels"] = labels
    if return_graph:
        for key in ("index", "dist2"):
            out[key] = res[key].cpu().numpy() if hip.K._is_torch(res[key]) else res[key]
    return out


class NearestNeighbourTest:
    """The leave-one-out k-NN two-sample test between two directories of audio, over the embedding caches FrechetAudioDistance writes
    and reads."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0):
        from .kad import KernelAudioDistance
        self.ml = ml
        self.device_index = device
        self.kad = KernelAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def test(self, baseline: PathLike, eval_dir: PathLike, k: int = 1, permutations: int = 1000, seed: int = 0) -> dict:
        """calc_nearest_neighbour_test of ``eval_dir`` against ``baseline``, the rows loaded as KernelAudioDistance.load_rows loads
        them; float64 caches and mixed dtypes go to float32."""
        from .hip import nn_test_k
        nn_test_k(k)
        _check_permutations(permutations)
        x = self.kad.load_rows(baseline)
        y = self.kad.load_rows(eval_dir)
        if x.dtype != y.dtype or x.dtype == np.float64:
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_nearest_neighbour_test(x, y, k=k, permutations=permutations, seed=seed, device=self.device_index)


def main(argv=None):
    from .cli import _registry, _setup_logging
    from .hip import KAD_MAX_PERMUTATIONS, nn_test_k
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.nn_test", description="Leave-one-out k-nearest-neighbour two-sample test between a "
                       "baseline and an evaluation directory of audio, on one GPU: accuracy near 0.5 is indistinguishable, above it "
                       "distinguishable, well below it memorised")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, help="append the result to this CSV")
    p.add_argument("-k", type=int, default=1, help="neighbours per row: odd, 1 .. 15 (default 1)")
    p.add_argument("-p", "--permutations", type=int, default=1000, help=f"random labellings (1 .. {KAD_MAX_PERMUTATIONS}, default 1000)")
    p.add_argument("--seed", type=int, default=0, help="seed of the labellings (default 0)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    try:
        nn_test_k(a.k)
        _check_permutations(a.permutations)
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]
    check_csv(a.csv)                                      # before any work: a CSV with another header is refused

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    nn = NearestNeighbourTest(model, audio_load_worker=a.workers, load_model=False)
    res = nn.test(a.baseline, a.eval, k=a.k, permutations=a.permutations, seed=a.seed)
    append_csv(a.csv, f"{model.name},{a.baseline},{a.eval},{res['k']},{res['n']},{res['m']},{res['accuracy']!r},"
                      f"{res['accuracy_baseline']!r},{res['accuracy_eval']!r},{res['p_value']!r},{res['p_value_low']!r},"
                      f"{res['permutations']},{a.seed}")
    log.info(f"Nearest-neighbour test appended to {a.csv}")
    log.info(f"The {res['k']}-NN accuracy {model.name} between {a.baseline} and {a.eval} is: {res['accuracy']} (baseline rows "
             f"{res['accuracy_baseline']}, eval rows {res['accuracy_eval']}; p = {res['p_value']:.4g}, lower tail {res['p_value_low']:.4g} "
             f"over {res['permutations']} permutations)")
    print(f"{res['accuracy']!r} {res['p_value']!r} {res['p_value_low']!r}")


if __name__ == "__main__":
    main()
