"""Leave-one-out k-NN two-sample test timing (device events around whole library calls) against fad_nearest on the same sets.

    python scripts/probe_nn_test.py [--n 100000] [--dims 512] [--ks 1,5] [--perms 1000] [--reps 3]

Per D, fp16, n = m, and k: fad_nn_test with P labellings (rows and labellings on the device), the same call with 31 labellings (one
labelling word: the self pass with next to no votes, so the difference is the vote kernel's and the label preparation's share), and
fad_nearest (k as given, authenticity off) on the same x and y.  The self pass walks (n + m)^2 pairs against fad_nearest's n m, so at
n = m the expectation is 4 such calls; `ratio` is nn_test_ms / nearest_ms."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402
from fadtk_amd.kad import random_labellings  # noqa: E402


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
    ap.add_argument("--dims", default="512")
    ap.add_argument("--ks", default="1,5")
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    n = a.n
    labels = random_labellings(n, n, a.perms, seed=0)
    few = labels[:31].contiguous()
    for d in map(int, a.dims.split(",")):
        x = torch.randn((n, d), generator=gen, device="cuda").half()
        y = (torch.randn((n, d), generator=gen, device="cuda") * 1.05 + 0.03).half()
        for k in map(int, a.ks.split(",")):
            t_near = timed(lambda: hip.nearest(x, y, k=k, authenticity=False), a.reps)
            t_all = timed(lambda: hip.nn_test(x, y, labels, k=k), a.reps)
            t_few = timed(lambda: hip.nn_test(x, y, few, k=k), a.reps)
            res = hip.nn_test(x, y, labels, k=k)
            row = {"D": d, "n": n, "m": n, "k": k, "permutations": a.perms, "nn_test_ms": round(t_all, 2), "nn_test_31_labellings_ms": round(t_few, 2),
                   "nearest_ms": round(t_near, 2), "ratio": round(t_all / t_near, 3), "ratio_31_labellings": round(t_few / t_near, 3),
                   "accuracy": res["accuracy"], "accuracy_x": res["accuracy_x"], "accuracy_y": res["accuracy_y"], "p_value": res["p_value"]}
            print(json.dumps(row), flush=True)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
