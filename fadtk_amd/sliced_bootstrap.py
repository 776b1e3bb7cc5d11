"""How certain is the sliced 2-Wasserstein distance of an evaluation directory, and is directory A really closer to the baseline than
directory B?  The bootstrap of the sliced distance, with FILES as the resampling units by default: the frames of one song are not
independent, so resampling rows understates the spread.

The baseline's and every evaluation set's embedding rows are projected on the random directions and sorted once per direction; every
resample of a set is the set with a count per row, so its sorted projections are the sorted array with every key repeated by its
row's count, and the distance is recomputed for all resamples in one GPU call per evaluation set (``fad_sliced_bootstrap``, DESIGN.md
4.21).  Every evaluation set meets the same resamples of the baseline, so the differences between sets are paired.

    python -m fadtk_amd.sliced_bootstrap <model> <baseline_dir> <evalA> [<evalB> ...] [--csv F] [-b 1000] [--confidence 0.95] [--rows]
                                         [--projections 512] [--seed 0] [-w N]

Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.  The CSV gets, under CSV_HEADER, one row per evaluation set (``kind`` =
SET_KIND: the distance, the replicates' mean and spread, ``bias``, the percentile interval ``ci_lo`` .. ``ci_hi`` and the basic one) and
one per pair of sets (``kind`` = PAIR_KIND, ``eval`` against ``other``: ``sw2_squared`` holds the observed difference, ``ci_lo`` ..
``ci_hi`` its percentile interval, ``prob_closer`` the share of replicates in which ``eval`` is closer to the baseline than ``other``).
The plug-in distance is biased upward (see ``calc_sliced_wasserstein_bootstrap``): read ``ci_basic``, or the pair rows, in which the
bias largely cancels.
"""
from __future__ import annotations

import logging
from argparse import ArgumentParser
from pathlib import Path

from .sliced import MAX_REPLICATES, SlicedWasserstein, check_bootstrap, check_params
from .sliced import check_csv as _check_csv
from .utils import PathLike

log = logging.getLogger("fadtk_amd")
CSV_HEADER = ("kind,model,baseline,eval,other,unit,n,m,sw2_squared,std_error,boot_mean,boot_std,bias,ci_lo,ci_hi,ci_basic_lo,ci_basic_hi,"
              "prob_closer,replicates,confidence,projections,seed\n")
SET_KIND = "set"
PAIR_KIND = "pair"


def check_csv(target: PathLike) -> None:
    """Refuse (ValueError) an existing CSV whose first line is not CSV_HEADER."""
    _check_csv(target, CSV_HEADER)


def _tail(res: dict) -> str:
    return f"{res['replicates']},{res['confidence']!r},{res['projections']},{'' if res['seed'] is None else res['seed']}"


def set_csv_row(model: str, baseline, eval_dir, res: dict) -> str:
    """One CSV row (no line end) of a calc_sliced_wasserstein_bootstrap result under CSV_HEADER."""
    return (f"{SET_KIND},{model},{baseline},{eval_dir},,{res['unit']},{res['n']},{res['m']},{res['sw2_squared']!r},{res['std_error']!r},"
            f"{res['boot_mean']!r},{res['boot_std']!r},{res['bias']!r},{res['ci_percentile'][0]!r},{res['ci_percentile'][1]!r},"
            f"{res['ci_basic'][0]!r},{res['ci_basic'][1]!r},,{_tail(res)}")


def pair_csv_row(model: str, baseline, eval_dir, other_dir, res_i: dict, res_j: dict, pair: dict) -> str:
    """One CSV row (no line end) of one pair of a calc_sliced_wasserstein_bootstrap_compare result under CSV_HEADER: ``res_i`` and
    ``res_j`` the two sets' dicts, ``pair`` their entry of ``pairs``."""
    return (f"{PAIR_KIND},{model},{baseline},{eval_dir},{other_dir},{res_i['unit']},{res_i['n']},,{pair['diff_observed']!r},,,,,"
            f"{pair['ci_diff'][0]!r},{pair['ci_diff'][1]!r},,,{pair['prob_closer']!r},{_tail(res_i)}")


def csv_rows(model: str, baseline, eval_dirs, res: dict) -> list:
    """-> the rows of a compare result: one per evaluation set, then one per pair (i < j)."""
    rows = [set_csv_row(model, baseline, e, r) for e, r in zip(eval_dirs, res["sets"])]
    rows += [pair_csv_row(model, baseline, eval_dirs[i], eval_dirs[j], res["sets"][i], res["sets"][j], p) for (i, j), p in res["pairs"].items()]
    return rows


def append_csv(target: PathLike, rows) -> None:
    """Append ``rows`` (no line ends) to the CSV ``target`` under CSV_HEADER (written when the file is new); a file with another header
    is refused, untouched."""
    check_csv(target)
    target = Path(target)
    target.parent.mkdir(parents=True, exist_ok=True)
    if not target.is_file():
        target.write_text(CSV_HEADER)
    with open(target, "a") as fh:
        fh.write("".join(r + "\n" for r in rows))


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.sliced_bootstrap", description="Bootstrap intervals of the sliced 2-Wasserstein distance "
                       "between a baseline and one or more evaluation directories of audio, and of the differences between them, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, nargs="+", help="directories to evaluate")
    p.add_argument("--csv", type=str, default=None, help="append the rows to this CSV")
    p.add_argument("-b", "--replicates", type=int, default=1000, help=f"bootstrap replicates (1 .. {MAX_REPLICATES}, default 1000)")
    p.add_argument("--confidence", type=float, default=0.95, help="level of the intervals (default 0.95)")
    p.add_argument("--rows", action="store_true", help="resample rows, not files")
    p.add_argument("--projections", type=int, default=512, help="random directions (default 512)")
    p.add_argument("--seed", type=int, default=0, help="seed of the directions and of the resamples (default 0)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    try:
        check_params(a.projections, a.seed)
        check_bootstrap(a.replicates, a.confidence)
    except ValueError as e:
        p.error(str(e))
    model = models[a.model]
    if a.csv:                                              # before any work: a CSV with another header is refused
        check_csv(a.csv)

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, *a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    sw = SlicedWasserstein(model, audio_load_worker=a.workers, load_model=False, projections=a.projections, seed=a.seed)
    res = sw.score_bootstrap(a.baseline, a.eval, replicates=a.replicates, confidence=a.confidence, rows=a.rows)
    if a.csv:
        append_csv(a.csv, csv_rows(model.name, a.baseline, a.eval, res))
        log.info(f"Sliced Wasserstein bootstrap appended to {a.csv}")
    for e, r in zip(a.eval, res["sets"]):
        log.info(f"The sliced Wasserstein distance {model.name} between {a.baseline} and {e} is: SW2^2 = {r['sw2_squared']} "
                 f"({100 * r['confidence']:g} % basic interval {r['ci_basic'][0]:.6g} .. {r['ci_basic'][1]:.6g}, percentile "
                 f"{r['ci_percentile'][0]:.6g} .. {r['ci_percentile'][1]:.6g}, bias {r['bias']:.3g}, over {r['replicates']} resamples of "
                 f"{r['unit']}s and {r['projections']} directions)")
        print(f"{r['sw2_squared']!r} {r['ci_basic'][0]!r} {r['ci_basic'][1]!r}")
    for (i, j), pr in res["pairs"].items():
        log.info(f"{a.eval[i]} against {a.eval[j]}: difference {pr['diff_observed']:.6g} (interval {pr['ci_diff'][0]:.6g} .. "
                 f"{pr['ci_diff'][1]:.6g}); {a.eval[i]} is the closer one in {100 * pr['prob_closer']:.1f} % of the resamples")


if __name__ == "__main__":
    main()
