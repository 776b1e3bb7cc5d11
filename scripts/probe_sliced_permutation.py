"""Sliced Wasserstein permutation test timing (device events around whole library calls), several runs each, alternating in one process
with the loop a user had to write before: P + 1 plain calls on rows gathered by the same labellings.

    python scripts/probe_sliced_permutation.py [--sizes 10000,100000] [--dims 128,512] [--projections 512] [--perms 200,1000]
                                               [--loop-at 200] [--reps 3] [--once N,D,P]

Per (n = m, D, P), fp16 rows on the device, L = `projections` standard normal directions, P labellings from kad.random_labellings on the
device, one JSON line:
  perm_ms        fad_sliced_permutation_test: the pooled pack, the labellings' words, projections and the key-index sort of the pooled
                 rows, every round's split, match and finish, the read-back of L (P + 1) sums, the statistics on the host;
  loop_ms        hip.sliced_wasserstein(Z[u], Z[~u]) for the observed and the P labellings, the gathers included -- run in full where
                 P <= `loop-at`; above it `loop_ms_extrapolated` = (P + 1) x the measured plain call, marked as what it is;
  plain_ms       one fad_sliced_wasserstein(x, y) call;
  same_observed  the new call's observed fields have the plain call's bits;
  plan           fad_sliced_permutation_last_plan.
Every run's time is listed.  ``--once N,D,P`` makes one warmed call and one timed call of the new entry alone and prints nothing else:
the command a kernel trace is taken of (rocprofv3 --kernel-trace --stats -- python scripts/probe_sliced_permutation.py --once
100000,128,200)."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402
from fadtk_amd.kad import random_labellings  # noqa: E402
from fadtk_amd.sliced import sliced_directions  # noqa: E402
from probe_sliced import alternating, once, rows  # noqa: E402


def unpack(labels, N):
    """packed int32 words [P, W] on the device -> bool [P, N]"""
    shifts = torch.arange(32, device=labels.device, dtype=torch.int32)
    return ((labels.unsqueeze(2) >> shifts) & 1).bool().reshape(labels.shape[0], -1)[:, :N]


def loop(z, n, masks, theta):
    """the yardstick: the observed labelling and every mask, one plain call each on gathered rows"""
    out = [hip.sliced_wasserstein(z[:n], z[n:], theta)["sw2_squared"]]
    for u in masks:
        out.append(hip.sliced_wasserstein(z[u], z[~u], theta)["sw2_squared"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--dims", default="128,512")
    ap.add_argument("--projections", type=int, default=512)
    ap.add_argument("--perms", default="200,1000")
    ap.add_argument("--loop-at", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    L = a.projections
    gen = torch.Generator(device="cuda").manual_seed(1)
    if a.once:
        n, d, P = map(int, a.once.split(","))
        x, y = rows(n, d, gen)
        theta = sliced_directions(d, L, 0)
        labels = random_labellings(n, n, P, seed=0)
        hip.sliced_permutation_test(x, y, labels, theta)
        ms = once(lambda: hip.sliced_permutation_test(x, y, labels, theta))
        print(json.dumps({"n": n, "D": d, "L": L, "P": P, "perm_ms": round(ms, 3), "plan": hip.sliced_permutation_last_plan()}), flush=True)
        return
    for n in map(int, a.sizes.split(",")):
        for d in map(int, a.dims.split(",")):
            x, y = rows(n, d, gen)
            z = torch.cat([x, y])
            theta = sliced_directions(d, L, 0)
            for P in map(int, a.perms.split(",")):
                labels = random_labellings(n, n, P, seed=0)
                fns = {"perm_ms": lambda: hip.sliced_permutation_test(x, y, labels, theta), "plain_ms": lambda: hip.sliced_wasserstein(x, y, theta)}
                full = P <= a.loop_at
                if full:
                    masks = unpack(labels, 2 * n)
                    fns["loop_ms"] = lambda: loop(z, n, masks, theta)
                t = alternating(fns, a.reps)
                res = hip.sliced_permutation_test(x, y, labels, theta)
                plan = hip.sliced_permutation_last_plan()
                plain = hip.sliced_wasserstein(x, y, theta)
                same = all(res[k] == plain[k] for k in ("sw2_squared", "std_error", "max_sliced", "max_index"))
                r = {"n": n, "m": n, "D": d, "dtype": "fp16", "projections": L, "P": P, **t, "sw2_squared": res["sw2_squared"],
                     "p_value": res["p_value"], "p_value_max": res["p_value_max"], "same_observed": same, "plan": plan}
                if full:
                    want = loop(z, n, masks, theta)
                    r["same_null_as_loop"] = bool(want[0] == res["sw2_squared"] and list(res["null"]) == want[1:])
                    r["loop_over_perm_min"] = round(min(t["loop_ms"]) / min(t["perm_ms"]), 2)
                else:
                    r["loop_ms_extrapolated"] = round((P + 1) * min(t["plain_ms"]), 1)
                    r["extrapolated_loop_over_perm_min"] = round(r["loop_ms_extrapolated"] / min(t["perm_ms"]), 2)
                print(json.dumps(r), flush=True)
                del labels
            del x, y, z
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
