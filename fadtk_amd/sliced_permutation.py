"""Is an evaluation directory distinguishable from the baseline at all?  The two-sample permutation test of the sliced 2-Wasserstein
distance: no bandwidth to choose, no O(N^2) pair pass.

The baseline's and the evaluation set's embedding rows are pooled, projected on the random directions and sorted once per direction;
the pooled rows are relabelled at random P times with the sizes held, every labelling splits the sorted projections into its two sorted
groups, and the sliced distance is recomputed for all of them in one GPU call (``fad_sliced_permutation_test``).
p = (1 + #{null >= observed}) / (P + 1), for the mean over the directions (``p_value``) and for the largest slice (``p_value_max``).

    python -m fadtk_amd.sliced_permutation <model> <baseline_dir> <eval_dir> [csv] [-p 1000] [--projections 512] [--seed 0] [-w N]

Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.  The CSV gets one row per call under CSV_HEADER.
"""
from __future__ import annotations

import logging
from argparse import ArgumentParser
from pathlib import Path

from .sliced import MAX_PERMUTATIONS, SlicedWasserstein, check_params, check_permutations
from .sliced import check_csv as _check_csv
from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,n,m,sw2_squared,sliced_w2,std_error,max_sliced,p_value,p_value_max,permutations,projections,seed\n"


def check_csv(target: PathLike) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not CSV_HEADER."""
    _check_csv(target, CSV_HEADER)


def csv_row(model: str, baseline, eval_dir, res: dict) -> str:
    """One CSV row (no line end) of a calc_sliced_wasserstein_permutation_test result under CSV_HEADER."""
    return (f"{model},{baseline},{eval_dir},{res['n']},{res['m']},{res['sw2_squared']!r},{res['sliced_w2']!r},{res['std_error']!r},"
            f"{res['max_sliced']!r},{res['p_value']!r},{res['p_value_max']!r},{res['permutations']},{res['projections']},"
            f"{'' if res['seed'] is None else res['seed']}")


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


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.sliced_permutation", description="Two-sample permutation test of the sliced "
                       "2-Wasserstein distance between a baseline and an evaluation directory of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", default=None, help="append the result to this CSV")
    p.add_argument("-p", "--permutations", type=int, default=1000, help=f"random labellings (1 .. {MAX_PERMUTATIONS}, default 1000)")
    p.add_argument("--projections", type=int, default=512, help="random directions (default 512)")
    p.add_argument("--seed", type=int, default=0, help="seed of the directions and of the labellings (default 0)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    try:
        check_params(a.projections, a.seed)
        check_permutations(a.permutations)
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]
    if a.csv:                                              # before any work: a CSV with another header is refused
        check_csv(a.csv)

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    sw = SlicedWasserstein(model, audio_load_worker=a.workers, load_model=False, projections=a.projections, seed=a.seed)
    res = sw.score_permutation_test(a.baseline, a.eval, permutations=a.permutations)
    if a.csv:
        append_csv(a.csv, csv_row(model.name, a.baseline, a.eval, res))
        log.info(f"Sliced Wasserstein permutation test appended to {a.csv}")
    log.info(f"The sliced Wasserstein distance {model.name} between {a.baseline} and {a.eval} is: SW2^2 = {res['sw2_squared']} "
             f"(p = {res['p_value']:.4g}, by the largest slice p = {res['p_value_max']:.4g}, over {res['permutations']} permutations "
             f"and {res['projections']} directions)")
    print(f"{res['sw2_squared']!r} {res['p_value']!r} {res['p_value_max']!r}")


if __name__ == "__main__":
    main()
