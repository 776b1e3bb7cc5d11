"""KAD standard-error timing (device events around single library calls): fad_kad_uncertainty against fad_kad on the same rows, the
bandwidth given to both.

    python scripts/probe_kad_uncertainty.py [--n 100000] [--m 100000] [--d 128,512,1024] [--sets 1,4] [--reps 3]
    python scripts/probe_kad_uncertainty.py --n 1000000 --m 1000000 --d 128 --sets 1 --reps 1 --no-kad    (under rocprofv3)

Per (D, S), float16 rows: ms_unc (pack, the one Z x Z pass, the row / set / covariance reductions), ms_kad (one fad_kad(x, y_0)),
their ratio, and the ratio of pairs each call walks: 2 (n^2 / 2 + m^2 / 2 + n m) for S = 1, and each further set adds m^2 + 2 n m.
The longest single launch comes from `rocprofv3 --kernel-trace --stats` on the second form (scripts/rocpd_summary.py)."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402


def timed(fn, reps):
    fn()                                                  # code object, workspaces
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--d", default="128,512,1024")
    ap.add_argument("--sets", default="1,4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kad", action="store_true", help="time fad_kad_uncertainty only")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    for d in map(int, a.d.split(",")):
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        sigma = float(d) ** 0.5 * 1.4                     # about the median distance of these rows; given to both calls
        for S in map(int, a.sets.split(",")):
            ys = [(torch.randn((a.m, d), generator=gen, device="cuda") * (1.0 + 0.02 * s) + 0.02 * s).half() for s in range(S)]
            n, m = a.n, a.m
            r = {"d": d, "n": n, "m": m, "sets": S, "sigma": sigma}
            r["ms_unc"] = timed(lambda: hip.kad_uncertainty(x, ys, bandwidth=sigma), a.reps)
            kad_pairs = n * n / 2 + m * m / 2 + n * m
            r["pairs_ratio"] = (2 * kad_pairs + (S - 1) * (m * m + 2 * n * m)) / kad_pairs
            if not a.no_kad:
                r["ms_kad"] = timed(lambda: hip.kad(x, ys[0], bandwidth=sigma), a.reps)
                r["ratio_vs_kad"] = r["ms_unc"] / r["ms_kad"]
                r["pair_rate_vs_kad"] = r["pairs_ratio"] / r["ratio_vs_kad"]
            print(json.dumps(r), flush=True)
            del ys
            torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
