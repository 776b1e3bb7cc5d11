"""Is an evaluation directory distinguishable from the baseline at all?  The two-sample permutation test of the Kernel Audio Distance.

The baseline's and the evaluation set's embedding rows are pooled and relabelled at random P times with the sizes held; MMD^2 is
recomputed for every labelling in one fused GPU pass (``fad_kad_permutation_test``), and p = (1 + #{null >= observed}) / (P + 1).
sigma defaults to the median pairwise distance of the pooled rows, which keeps the test exact.

    python -m fadtk_amd.kad_permutation <model> <baseline_dir> <eval_dir> [csv] [-p 1000] [--seed 0] [--bandwidth S] [--kernel K] [--scale F] [-w N]

Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.  A CSV gets one row per call
(model, baseline, eval, kad, p_value, permutations, seed, bandwidth, scale, time; with ``--kernel iq`` or ``imq`` one more column,
kernel).
"""
from __future__ import annotations

import logging
import time
from argparse import ArgumentParser
from pathlib import Path

from .kad import KAD_KERNELS, KernelAudioDistance, append_csv, check_csv

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,kad,p_value,permutations,seed,bandwidth,scale,time\n"


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
    p.add_argument("--bandwidth", type=float, default=None, help="kernel sigma (default: median pairwise distance of the pooled rows)")
    p.add_argument("--kernel", type=str, choices=list(KAD_KERNELS), default="gaussian",
                   help="gaussian exp(-t), iq 1 / (1 + t) or imq 1 / sqrt(1 + t), t = d^2 / (2 sigma^2) (default gaussian); a CSV written "
                        "for iq or imq has one more column, kernel")
    p.add_argument("--scale", type=float, default=1.0, help="factor applied to the reported MMD^2 (default 1)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    if not 1 <= a.permutations <= KAD_MAX_PERMUTATIONS:
        p.error(f"--permutations must lie in 1 .. {KAD_MAX_PERMUTATIONS}, got {a.permutations}")
    model = models[a.model]
    if a.csv:
        check_csv(a.csv, CSV_HEADER, a.kernel)             # before any work: a CSV of the other form is refused

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    kad = KernelAudioDistance(model, audio_load_worker=a.workers, load_model=False)
    t0 = time.time()
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
