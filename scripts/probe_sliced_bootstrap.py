"""Sliced Wasserstein bootstrap timing (device events around whole library calls), several runs each, alternating in one process with the
loop a user had to write before: B + 1 plain calls on rows gathered by the same counts (np.repeat on the device).

    python scripts/probe_sliced_bootstrap.py [--sizes 100000] [--dims 128,512] [--projections 512] [--replicates 200] [--files 2000]
                                             [--reps 3] [--once N,D,B[,F]]

Per (n = m, D, B), fp16 rows on the device, L = `projections` standard normal directions, counts from sliced.bootstrap_counts, one JSON
line with unit "row" and, at the first D, one with unit "file" (`files` files of n / files rows on both sides):
  boot_ms        fad_sliced_bootstrap: the two packs, the count words and their upload, projections and the key-index sorts of both
                 sets, every round's two expansions, match and finish, the read-back of L (B + 1) sums, the statistics on the host;
  loop_ms        hip.sliced_wasserstein on (x, y) and on torch.repeat_interleave of both sets by every replicate's counts, the gathers
                 included;
  plain_ms       one fad_sliced_wasserstein(x, y) call;
  same_observed  the new call's observed fields have the plain call's bits;  same_boot_as_loop  boot has the loop's bits;
  plan           fad_sliced_bootstrap_last_plan.
Every run's time is listed.  ``--once N,D,B[,F]`` makes one warmed call and one timed call of the new entry alone and prints nothing
else: the command a kernel trace is taken of (rocprofv3 --kernel-trace --stats -- python scripts/probe_sliced_bootstrap.py --once
100000,128,200)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402
from fadtk_amd.sliced import bootstrap_counts, sliced_directions  # noqa: E402
from probe_sliced import alternating, once, rows  # noqa: E402


def counts(n, B, files):
    """(counts_x, counts_y) uint8 [B x n]: rows as units, or `files` files of n / files rows"""
    sizes = np.ones(n, dtype=np.int64) if not files else np.full(files, n // files, dtype=np.int64)
    return bootstrap_counts(sizes, B, 0, 0), bootstrap_counts(sizes, B, 0, 1)


def loop(x, y, cx_dev, cy_dev, theta):
    """the yardstick: the sets as given and every replicate, one plain call each on gathered rows"""
    out = [hip.sliced_wasserstein(x, y, theta)["sw2_squared"]]
    for a, b in zip(cx_dev, cy_dev):
        out.append(hip.sliced_wasserstein(torch.repeat_interleave(x, a, dim=0), torch.repeat_interleave(y, b, dim=0), theta)["sw2_squared"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000")
    ap.add_argument("--dims", default="128,512")
    ap.add_argument("--projections", type=int, default=512)
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--files", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    L, B = a.projections, a.replicates
    gen = torch.Generator(device="cuda").manual_seed(1)
    if a.once:
        n, d, B, *files = map(int, a.once.split(","))
        x, y = rows(n, d, gen)
        theta = sliced_directions(d, L, 0)
        cx, cy = counts(n, B, files[0] if files else 0)
        hip.sliced_bootstrap(x, y, cx, cy, theta)
        ms = once(lambda: hip.sliced_bootstrap(x, y, cx, cy, theta))
        print(json.dumps({"n": n, "D": d, "L": L, "B": B, "files": files[0] if files else 0, "boot_ms": round(ms, 3),
                          "plan": hip.sliced_bootstrap_last_plan()}), flush=True)
        return
    for n in map(int, a.sizes.split(",")):
        for di, d in enumerate(map(int, a.dims.split(","))):
            x, y = rows(n, d, gen)
            theta = sliced_directions(d, L, 0)
            for files in ((0, a.files) if di == 0 and a.files else (0,)):
                cx, cy = counts(n, B, files)
                cx_dev, cy_dev = torch.from_numpy(cx.astype(np.int64)).cuda(), torch.from_numpy(cy.astype(np.int64)).cuda()
                fns = {"boot_ms": lambda: hip.sliced_bootstrap(x, y, cx, cy, theta), "plain_ms": lambda: hip.sliced_wasserstein(x, y, theta),
                       "loop_ms": lambda: loop(x, y, cx_dev, cy_dev, theta)}
                t = alternating(fns, a.reps)
                res = hip.sliced_bootstrap(x, y, cx, cy, theta, per_replicate=True)
                plan = hip.sliced_bootstrap_last_plan()
                plain = hip.sliced_wasserstein(x, y, theta)
                want = loop(x, y, cx_dev, cy_dev, theta)
                tot = res["totals"]
                r = {"n": n, "m": n, "D": d, "dtype": "fp16", "projections": L, "B": B, "unit": "file" if files else "row", "files": files, **t,
                     "sw2_squared": res["sw2_squared"], "boot_mean": float(res["boot"].mean()), "boot_std": float(res["boot"].std(ddof=1)),
                     "totals_min_max": [int(tot.min()), int(tot.max())],
                     "same_observed": all(res[k] == plain[k] for k in ("sw2_squared", "std_error", "max_sliced", "max_index")),
                     "same_boot_as_loop": bool(want[0] == res["sw2_squared"] and list(res["boot"]) == want[1:]), "plan": plan,
                     "loop_over_boot_min": round(min(t["loop_ms"]) / min(t["boot_ms"]), 2)}
                print(json.dumps(r), flush=True)
                del cx_dev, cy_dev
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
