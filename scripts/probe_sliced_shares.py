"""Sliced Wasserstein per-row shares timing (device events around whole library calls), several runs each, alternating in one process
with the plain call on the same inputs.

    python scripts/probe_sliced_shares.py [--sizes 10000,100000] [--dims 128,512] [--projections 512] [--reps 3] [--once N,D]

Per (n = m, D), fp16 rows on the device, L = `projections` standard normal directions, one JSON line:
  shares_ms      fad_sliced_shares: the plain call's work with the key-index sort, the two cost kernels, the per-row sums and the
                 read-back of n + m float64 sums;
  plain_ms       fad_sliced_wasserstein on the same inputs;
  same_result    the result fields of the two calls have the same bits;
  sum_x, sum_y   the sums of the shares beside sw2_squared;
  plan           fad_sliced_last_plan of the shares call: chunks, directions per chunk, sort passes, workgroups per segment.
Every run's time is listed, so the spread between runs shows next to the ratio.  ``--once N,D`` makes one warmed call and one timed
call of the shares entry alone at that shape and prints nothing else: the command a kernel trace is taken of
(rocprofv3 --kernel-trace --stats -- python scripts/probe_sliced_shares.py --once 100000,128)."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402
from fadtk_amd.sliced import sliced_directions  # noqa: E402
from probe_sliced import alternating, once, rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--dims", default="128,512")
    ap.add_argument("--projections", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    L = a.projections
    gen = torch.Generator(device="cuda").manual_seed(1)
    if a.once:
        n, d = map(int, a.once.split(","))
        x, y = rows(n, d, gen)
        theta = sliced_directions(d, L, 0)
        hip.sliced_shares(x, y, theta)
        print(json.dumps({"n": n, "D": d, "L": L, "shares_ms": round(once(lambda: hip.sliced_shares(x, y, theta)), 3)}), flush=True)
        return
    for n in map(int, a.sizes.split(",")):
        for d in map(int, a.dims.split(",")):
            x, y = rows(n, d, gen)
            theta = sliced_directions(d, L, 0)
            fns = {"shares_ms": lambda: hip.sliced_shares(x, y, theta), "plain_ms": lambda: hip.sliced_wasserstein(x, y, theta)}
            t = alternating(fns, a.reps)
            plain = hip.sliced_wasserstein(x, y, theta)
            res = hip.sliced_shares(x, y, theta)
            same = all(res[k] == plain[k] for k in ("sw2_squared", "std_error", "max_sliced", "max_index"))
            r = {"n": n, "m": n, "D": d, "dtype": "fp16", "projections": L, **t, "sw2_squared": res["sw2_squared"], "same_result": same,
                 "sum_x": float(res["share_x"].sum()), "sum_y": float(res["share_y"].sum()), "plan": hip.sliced_last_plan(),
                 "shares_over_plain_min": round(min(t["shares_ms"]) / min(t["plain_ms"]), 2)}
            print(json.dumps(r), flush=True)
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
