"""KAD bandwidth sweep timing: one fad_kad_sweep of B bandwidths against B calls of fad_kad_k with the same bandwidths (device events
around whole library calls).

    python scripts/probe_kad_sweep.py [--n 100000] [--dims 128,512] [--sweep 1,4,8] [--kernel gaussian,iq] [--runs 3] [--only-sweep]

Per D: n = m fp16 rows on the device, the baseline's median found once outside the timing, sigma_b = median x a geometric ladder over
[0.25, 4] (B = 1: the median itself).  Per kernel and B the two routes alternate in one process, --runs times each after one untimed
call of each (code object, workspaces); one JSON line with both lists of times (ms), their ranges, the ratio of the medians, and whether
the slowest sweep beat the fastest of the B single calls.  The first line also carries `s_first_call`, the wall time of the process's
first KAD call, which loads KAD's code object.  --only-sweep times the sweep alone: for a run under `rocprofv3 --kernel-trace --stats`,
where the longest single launch of each kernel is the `max_us` column of scripts/rocpd_summary.py."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402


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
    ap.add_argument("--sweep", default="1,4,8", help="comma-separated numbers of bandwidths B")
    ap.add_argument("--kernel", default="gaussian,iq")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only-sweep", action="store_true")
    a = ap.parse_args()
    kernels = a.kernel.split(",")
    for k in kernels:
        hip.kad_kernel_code(k)
    gen = torch.Generator(device="cuda").manual_seed(1)
    first_call = None
    for d in map(int, a.dims.split(",")):
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        y = (torch.randn((a.n, d), generator=gen, device="cuda") + 0.05).half()
        t0 = time.perf_counter()
        median = hip.kad_median_distance(x)
        if first_call is None:
            first_call = time.perf_counter() - t0
        for kernel in kernels:
            for B in map(int, a.sweep.split(",")):
                sigmas = [median * 0.25 * 16.0 ** (b / (B - 1)) for b in range(B)] if B > 1 else [median]

                def sweep():
                    return hip.kad_sweep(x, y, bandwidths=sigmas, kernel=kernel)

                def singles():
                    return [hip.kad(x, y, bandwidth=s, kernel=kernel) for s in sigmas]
                got = sweep()
                r = {"d": d, "n": a.n, "kernel": kernel, "B": B, "sigma_median": median}
                if not a.only_sweep:
                    ref = singles()
                    r["max_rel_diff_mmd2"] = max(abs(got["mmd2"][b] - ref[b]["mmd2"]) / abs(ref[b]["mmd2"]) for b in range(B))
                ts, tb = [], []
                for _ in range(a.runs):                       # alternating: drift of the clocks falls on both routes alike
                    ts.append(timed(sweep))
                    if not a.only_sweep:
                        tb.append(timed(singles))
                r.update(ms_sweep=ts, ms_sweep_range=[min(ts), max(ts)])
                if tb:
                    r.update(ms_singles=tb, ms_singles_range=[min(tb), max(tb)], ratio_of_medians=statistics.median(ts) / statistics.median(tb),
                             sweep_in_single_calls=statistics.median(ts) / (statistics.median(tb) / B), slowest_sweep_beats_fastest_singles=max(ts) < min(tb))
                if first_call is not None:
                    r["s_first_call"], first_call = first_call, None
                print(json.dumps(r), flush=True)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
