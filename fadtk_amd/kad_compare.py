"""Kernel Audio Distance of several evaluation directories against one baseline, with standard errors and paired comparisons.

One GPU call (``fad_kad_uncertainty``) gives every set's KAD with one sigma, the first-order covariance of the estimates, and from it
the paired z / p of every two sets: "model A scores 0.0121 and model B 0.0134 against the same baseline -- is that a difference?".
The estimate is first-order (meaningful for sets that differ from the baseline).

    python -m fadtk_amd.kad_compare <model> <baseline_dir> <eval_dir> [<eval_dir> ...] [--csv F] [--bandwidth S] [--kernel K] [--scale F] [-w N]

Embeddings are cached as ``python -m fadtk_amd.kad`` caches them.  ``--csv`` appends one row per evaluation set
(model, baseline, eval, kad, stderr, bandwidth, scale; with ``--kernel iq`` or ``imq`` one more column, kernel); the pairwise z / p
table is logged.
"""
from __future__ import annotations

import logging
from argparse import ArgumentParser
from pathlib import Path

from .kad import KAD_KERNELS, KernelAudioDistance, append_csv, check_csv

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,kad,stderr,bandwidth,scale\n"


def main(argv=None):
    from .cli import _registry, _setup_logging
    from .hip import KAD_MAX_SETS
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.kad_compare", description="Kernel Audio Distance of several directories of audio "
                       "against one baseline, with standard errors and paired z / p, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, nargs="+", help=f"directories to evaluate (1 .. {KAD_MAX_SETS})")
    p.add_argument("--csv", type=str, default=None, help="append one row per evaluation directory to this CSV")
    p.add_argument("--bandwidth", type=float, default=None, help="kernel sigma (default: median pairwise distance of the baseline)")
    p.add_argument("--kernel", type=str, choices=list(KAD_KERNELS), default="gaussian",
                   help="gaussian exp(-t), iq 1 / (1 + t) or imq 1 / sqrt(1 + t), t = d^2 / (2 sigma^2) (default gaussian); a CSV written "
                        "for iq or imq has one more column, kernel")
    p.add_argument("--scale", type=float, default=1.0, help="factor applied to the reported MMD^2 and its standard error (default 1)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    a = p.parse_args(argv)
    if len(a.eval) > KAD_MAX_SETS:
        p.error(f"at most {KAD_MAX_SETS} evaluation directories, got {len(a.eval)}")
    model = models[a.model]
    if a.csv:
        check_csv(a.csv, CSV_HEADER, a.kernel)             # before any work: a CSV of the other form is refused

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, *a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    kad = KernelAudioDistance(model, audio_load_worker=a.workers, load_model=False)
    res = kad.score_many(a.baseline, a.eval, bandwidth=a.bandwidth, scale=a.scale, kernel=a.kernel)
    if a.csv:
        append_csv(a.csv, CSV_HEADER, [f"{model.name},{a.baseline},{e},{float(v)!r},{float(se)!r},{res.bandwidth!r},{a.scale!r}"
                                       for e, v, se in zip(a.eval, res.values, res.stderr)], a.kernel)
        log.info(f"KAD scores appended to {a.csv}")
    for e, v, se in zip(a.eval, res.values, res.stderr):
        log.info(f"The KAD {model.name} score between {a.baseline} and {e} is: {v} +- {se} (bandwidth {res.bandwidth})")
        print(f"{e} {float(v)!r} {float(se)!r}")
    z, pv = res.compare()
    for s in range(len(a.eval)):
        for t in range(s + 1, len(a.eval)):
            log.info(f"{a.eval[s]} vs {a.eval[t]}: difference {res.values[s] - res.values[t]:.6g}, z = {z[s, t]:.3f}, p = {pv[s, t]:.3g}")


if __name__ == "__main__":
    main()
