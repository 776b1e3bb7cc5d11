"""Sinkhorn divergence timing (device events around whole library calls), several runs each, alternating in one process.

    python scripts/probe_sinkhorn.py [--sizes 10000,100000] [--dims 128,512] [--iterations 100] [--reps 3] [--torch-max 10000]

Per (n = m, D), fp16 rows on the device, one JSON line:
  sinkhorn_ms      fad_sinkhorn at `iterations` iterations and a fixed epsilon (0.25 x the median distance of 5000 rows, squared);
  sinkhorn_1_ms    the same call at 1 iteration: the packs, the diagnostic step and 2 of the half-steps per problem;
  per_iteration_ms (min sinkhorn_ms - min sinkhorn_1_ms) / (iterations - 1): 6 half-steps, 2 per problem;
  kad_ms           fad_kad on the same rows at a fixed bandwidth: XX and YY over their triangles and XY over the rectangle, 2 rectangles
                   of tiles in all;
  kad_individual_ms  fad_kad_individual with the evaluation rows as songs of 2 rows (the band pass is then the diagonal tiles only): XX's
                   triangle and the per-column cross pass over the rectangle;
  cross_pass_ms    min kad_individual_ms - min kad_ms / 4: the cross pass alone, the pass a half-step is built on;
  half_step_over_cross_pass   per_iteration_ms / 6 / cross_pass_ms;
  torch_ms         (n <= --torch-max) the same iteration in torch on the same GPU: C = cdist^2 / 2 in float32, stored once per
                   problem, torch.logsumexp per half-step;  torch_divergence next to divergence.
Every run's time is listed, so the spread between runs shows next to the differences."""
import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternating(fns, reps):
    """{name: [ms per run]}: a warm-up call of each (code object, workspaces), then reps rounds of one run each, in turn"""
    for fn in fns.values():
        fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(round(once(fn), 3))
    return out


def torch_ot(a, b, eps, iterations):
    C = 0.5 * torch.cdist(a, b) ** 2
    n, m = C.shape
    f, g = torch.zeros(n, device=C.device), torch.zeros(m, device=C.device)
    for _ in range(iterations):
        f = -eps * (torch.logsumexp((g[None, :] - C) / eps, dim=1) - math.log(m))
        g = -eps * (torch.logsumexp((f[:, None] - C) / eps, dim=0) - math.log(n))
    return f.double().mean().item() + g.double().mean().item()


def torch_sinkhorn(x, y, eps, iterations):
    x, y = x.float(), y.float()
    return torch_ot(x, y, eps, iterations) - 0.5 * torch_ot(x, x, eps, iterations) - 0.5 * torch_ot(y, y, eps, iterations)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--dims", default="128,512")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-max", type=int, default=10000)
    a = ap.parse_args()
    L = a.iterations
    gen = torch.Generator(device="cuda").manual_seed(1)
    for n in map(int, a.sizes.split(",")):
        for d in map(int, a.dims.split(",")):
            x = torch.randn((n, d), generator=gen, device="cuda").half()
            y = (torch.randn((n, d), generator=gen, device="cuda") + 0.05).half()
            sigma = hip.kad_median_distance(x[:5000].contiguous())
            eps = (0.25 * sigma) ** 2
            offsets = np.arange(0, n + 1, 2, dtype=np.int64)
            offsets[-1] = n
            fns = {"sinkhorn_ms": lambda: hip.sinkhorn(x, y, epsilon=eps, iterations=L),
                   "sinkhorn_1_ms": lambda: hip.sinkhorn(x, y, epsilon=eps, iterations=1),
                   "kad_ms": lambda: hip.kad(x, y, bandwidth=sigma),
                   "kad_individual_ms": lambda: hip.kad_individual(x, y, offsets, bandwidth=sigma)}
            if n <= a.torch_max:
                fns["torch_ms"] = lambda: torch_sinkhorn(x, y, eps, L)
            t = alternating(fns, a.reps)
            res = hip.sinkhorn(x, y, epsilon=eps, iterations=L)
            per_it = (min(t["sinkhorn_ms"]) - min(t["sinkhorn_1_ms"])) / max(L - 1, 1)
            cross = min(t["kad_individual_ms"]) - min(t["kad_ms"]) / 4
            r = {"n": n, "m": n, "D": d, "dtype": "fp16", "iterations": L, "epsilon": eps, **t, "per_iteration_ms": round(per_it, 4),
                 "cross_pass_ms": round(cross, 4), "half_step_over_cross_pass": round(per_it / 6 / cross, 3),
                 "divergence": res["divergence"], "marginal_error": res["marginal_error"], "plan": hip.kad_last_plan()}
            if n <= a.torch_max:
                r["torch_divergence"] = torch_sinkhorn(x, y, eps, L)
                r["torch_over_sinkhorn_min"] = round(min(t["torch_ms"]) / min(t["sinkhorn_ms"]), 2)
            print(json.dumps(r), flush=True)
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
