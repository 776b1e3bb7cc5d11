"""Is an evaluation directory distinguishable from the baseline at all?  The two-sample permutation test of the Kernel Audio Distance.

The baseline's and the evaluation set's embedding rows are pooled and relabelled at random P times with the sizes held; MMD^2 is
recomputed for every labelling in one fused GPU pass (``fad_kad_permutation_test``), and p = (1 + #{null >= observed}) / (P + 1).
sigma defaults to the median pairwise distance of the pooled rows, which keeps the test exact.

    python -m fadtk_amd.kad_permutation <model> <baseline_dir> <eval_dir> [csv] [-p 1000] [--seed 0] [--bandwidth S] [--kernel K] [--scale F] [-w N]
                                        [--bandwidth-factors F1,F2,... | --bandwidths S1,S2,...]

Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.  A CSV gets one row per call
(model, baseline, eval, kad, p_value, permutations, seed, bandwidth, scale, time; with ``--kernel iq`` or ``imq`` one more column,
kernel).

A test at one sigma is blind to differences that live at another scale.  ``--bandwidth-factors`` (multiples of the pooled median) or
``--bandwidths`` (sigma values) run the test at 1 .. 16 bandwidths on the same labellings in one fused pass
(``fad_kad_permutation_sweep``) and add the min-p aggregate over them, one p-value that does not depend on having picked the right
sigma.  The CSV then gets one row per bandwidth under a header with one more column, p_aggregated (before kernel), and
the printed line is p_aggregated followed by the per-bandwidth p-values.
"""
from __future__ import annotations

import logging
import time
from argparse import ArgumentParser
from pathlib import Path

from .kad import KAD_KERNELS, KernelAudioDistance, _aggregate_request, _float_list, append_csv, check_csv

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,kad,p_value,permutations,seed,bandwidth,scale,time\n"
AGG_CSV_HEADER = CSV_HEADER.rstrip("\n") + ",p_aggregated\n"      # the aggregated form: one row per bandwidth


def check_csv_form(target, header: str, kernel: str) -> None:
    """check_csv for ``header``, and a refusal (ValueError) of a CSV that begins with the other of CSV_HEADER and AGG_CSV_HEADER, in
    either kernel form: no CSV mixes rows of the single and of the aggregated test."""
    check_csv(target, header, kernel)
    other = CSV_HEADER if header == AGG_CSV_HEADER else AGG_CSV_HEADER
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline().rstrip("\r\n")
        if first in (other.rstrip("\n"), other.rstrip("\n") + ",kernel"):
            raise ValueError(f"{target} has the header {first!r}; these rows go under {header.strip()!r}: write them to another file")


def main(argv=None):
    from .cli import _registry, _setup_logging
    from .hip import KAD_MAX_PERMUTATIONS
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.kad_permutation", description="Two-sample permutation test of the Kernel Audio "
                       "Distance between a baseline and an evaluation directory of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", default=None, help="append the result to this CSV")
    p.add_argument("-p", "--permutations", type=int, default=1000, help=f"random labellings (1 .. {KAD_MAX_PERMUTATIONS}, default 1000)")
    p.add_argument("--seed", type=int, default=0, help="seed of the labellings (default 0)")
    bw = p.add_mutually_exclusive_group()
    bw.add_argument("--bandwidth", type=float, default=None, help="kernel sigma (default: median pairwise distance of the pooled rows)")
    bw.add_argument("--bandwidth-factors", type=_float_list, default=None, metavar="F1,F2,...",
                    help="the test at several bandwidths in one fused pass, each a multiple of the median pairwise distance of the pooled "
                         "rows, and the min-p aggregate over them: one CSV row per bandwidth with one more column, p_aggregated (1 .. 16 "
                         "values > 0)")
    bw.add_argument("--bandwidths", type=_float_list, default=None, metavar="S1,S2,...",
                    help="as --bandwidth-factors, the sigma values themselves")
    p.add_argument("--kernel", type=str, choices=list(KAD_KERNELS), default="gaussian",
                   help="gaussian exp(-t), iq 1 / (1 + t) or imq 1 / sqrt(1 + t), t = d^2 / (2 sigma^2) (default gaussian); a CSV written "
                        "for iq or imq has one more column, kernel")
    p.add_argument("--scale", type=float, default=1.0, help="factor applied to the reported MMD^2 (default 1)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    if not 1 <= a.permutations <= KAD_MAX_PERMUTATIONS:
        p.error(f"--permutations must lie in 1 .. {KAD_MAX_PERMUTATIONS}, got {a.permutations}")
    sweep = a.bandwidths is not None or a.bandwidth_factors is not None
    if sweep:
        try:
            _aggregate_request(a.bandwidths, a.bandwidth_factors)
        except ValueError as e:
            p.error(str(e))
    model = models[a.model]
    if a.csv:                                              # before any work: a CSV of another form is refused
        check_csv_form(a.csv, AGG_CSV_HEADER if sweep else CSV_HEADER, a.kernel)

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    kad = KernelAudioDistance(model, audio_load_worker=a.workers, load_model=False)
    t0 = time.time()
    if sweep:
        res = kad.aggregated_test(a.baseline, a.eval, permutations=a.permutations, seed=a.seed, factors=a.bandwidth_factors,
                                  bandwidths=a.bandwidths, scale=a.scale, kernel=a.kernel)
        elapsed = time.time() - t0
        rows = [f"{model.name},{a.baseline},{a.eval},{float(v)!r},{float(pv)!r},{res['permutations']},{a.seed},{float(s)!r},{a.scale!r},"
                f"{elapsed!r},{res['p_aggregated']!r}" for v, pv, s in zip(res["kad"], res["p_values"], res["bandwidths"])]
        if a.csv:
            append_csv(a.csv, AGG_CSV_HEADER, rows, a.kernel)
            log.info(f"{len(rows)} rows of the aggregated KAD permutation test appended to {a.csv}")
        for v, pv, s in zip(res["kad"], res["p_values"], res["bandwidths"]):
            log.info(f"The KAD {model.name} score between {a.baseline} and {a.eval} is: {float(v)} (p = {float(pv):.4g}, bandwidth {float(s)})")
        log.info(f"Aggregated over these {len(rows)} bandwidths: p = {res['p_aggregated']:.4g} over {res['permutations']} permutations")
        print(" ".join([repr(res["p_aggregated"]), *(repr(float(pv)) for pv in res["p_values"])]))
        return
    res = kad.permutation_test(a.baseline, a.eval, permutations=a.permutations, seed=a.seed, bandwidth=a.bandwidth, scale=a.scale,
                               kernel=a.kernel)
    elapsed = time.time() - t0
    if a.csv:
        append_csv(a.csv, CSV_HEADER, [f"{model.name},{a.baseline},{a.eval},{res['kad']!r},{res['p_value']!r},{res['permutations']},{a.seed},"
                                       f"{res['bandwidth']!r},{a.scale!r},{elapsed!r}"], a.kernel)
        log.info(f"KAD permutation test appended to {a.csv}")
    log.info(f"The KAD {model.name} score between {a.baseline} and {a.eval} is: {res['kad']} (p = {res['p_value']:.4g} over "
             f"{res['permutations']} permutations, bandwidth {res['bandwidth']})")
    print(f"{res['kad']!r} {res['p_value']!r}")


if __name__ == "__main__":
    main()
