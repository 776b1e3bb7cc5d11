"""KAD permutation sweep timing: one fad_kad_permutation_sweep of B bandwidths against B calls of fad_kad_permutation_test_k with the
same bandwidths and labellings (device events around whole library calls).

    python scripts/probe_kad_permutation_sweep.py [--n 100000] [--dims 128,512] [--perms 199,999] [--B 4] [--runs 3] [--only-sweep]

Per D: n = m fp16 rows on the device, the pooled median found once outside the timing, explicit sigma_b = median x {0.25, 0.5, 1, 2}
(B = 4; a geometric ladder over [0.25, 2] otherwise), the labellings drawn once on the device.  Per P the two routes alternate in one
process, --runs times each after one untimed call of each (code object, workspaces); one JSON line with both lists of times (ms), their
ranges, the ratio of the medians, the spread of the single calls and the two requirements of DESIGN.md 4.13: at P <= 255 the sweep
faster than its single calls by more than their spread, at any P not slower than them by more than that spread.  `max_dev_in_sd` is
the largest difference between a sweep entry and its single call, in null standard deviations (0 where the cuts agree).  --only-sweep
times the sweep alone: for a run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402
from fadtk_amd.kad import random_labellings  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="128,512")
    ap.add_argument("--perms", default="199,999")
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only-sweep", action="store_true")
    a = ap.parse_args()
    B = a.B
    gen = torch.Generator(device="cuda").manual_seed(1)
    for d in map(int, a.dims.split(",")):
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        y = (torch.randn((a.n, d), generator=gen, device="cuda") + 0.05).half()
        median = hip.kad_median_distance(torch.cat([x, y]))
        sigmas = [median * 0.25 * 8.0 ** (b / (B - 1)) for b in range(B)] if B > 1 else [median]
        for P in map(int, a.perms.split(",")):
            labels = random_labellings(a.n, a.n, P, seed=P)

            def sweep():
                return hip.kad_permutation_sweep(x, y, labels, bandwidths=sigmas)

            def singles():
                return [hip.kad_permutation_test(x, y, labels, bandwidth=s) for s in sigmas]
            got = sweep()
            r = {"d": d, "n": a.n, "P": P, "B": B, "sigma_median": median, "p_aggregated": got["p_aggregated"],
                 "p_values": got["p_values"].tolist()}
            if not a.only_sweep:
                ref = singles()
                r["max_dev_in_sd"] = max(float(max(abs(got["mmd2"][b] - ref[b]["mmd2"]), np.max(np.abs(got["null"][b] - ref[b]["null"])))
                                               / np.std(ref[b]["null"])) for b in range(B))
            ts, tb = [], []
            for _ in range(a.runs):                           # alternating: drift of the clocks falls on both routes alike
                ts.append(timed(sweep))
                if not a.only_sweep:
                    tb.append(timed(singles))
            r.update(ms_sweep=ts, ms_sweep_range=[min(ts), max(ts)])
            if tb:
                spread = max(tb) - min(tb)
                r.update(ms_singles=tb, ms_singles_range=[min(tb), max(tb)], ms_singles_spread=spread,
                         ratio_of_medians=statistics.median(ts) / statistics.median(tb),
                         faster_by_more_than_spread=statistics.median(tb) - statistics.median(ts) > spread,
                         not_slower_by_more_than_spread=statistics.median(ts) - statistics.median(tb) <= spread)
            print(json.dumps(r), flush=True)
            del labels
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
