"""Polynomial-kernel distance timing (device events around whole library calls), three runs each, alternating in one process.

    python scripts/probe_kid.py [--n 100000] [--dims 128,512] [--reps 3] [--subsets 100,1000] [--subset-size 1000] [--no-torch] [--no-full]

Per D, one JSON line each:
  (a) fad_kid_subsets at `subsets` x `subset_size` (device rows, device indices) against the torch formulation on the same GPU:
      index_select, batched fp16 matmul widened to float32, pow, masked sums per subset (25 subsets a batch: 250 MB of pair matrices);
  (b) fad_kid over all rows against fad_kad_k (Gaussian, fixed bandwidth) on the same rows: the same main loop and walk, epilogues of
      the same length.
Every run's time is listed, so the spread between runs shows next to the difference between the two.  Under
`rocprofv3 --kernel-trace --stats` (a run of its own) scripts/rocpd_summary.py gives the share of gather-pack, pass and reduce and the
longest single launch (`max_us`)."""
import argparse
import json
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


def torch_subsets(x, y, ix, iy, gamma, batch=25):
    s = ix.shape[1]
    vals = []
    for q0 in range(0, ix.shape[0], batch):
        xs = x.index_select(0, ix[q0:q0 + batch].reshape(-1).long()).view(-1, s, x.shape[1])
        ys = y.index_select(0, iy[q0:q0 + batch].reshape(-1).long()).view(-1, s, y.shape[1])
        def k(a, b):
            return (torch.bmm(a, b.transpose(1, 2)).float() * gamma + 1.0).pow(3)
        kxx, kyy, kxy = k(xs, xs), k(ys, ys), k(xs, ys)
        sxx = kxx.sum((1, 2), dtype=torch.float64) - kxx.diagonal(dim1=1, dim2=2).sum(1, dtype=torch.float64)
        syy = kyy.sum((1, 2), dtype=torch.float64) - kyy.diagonal(dim1=1, dim2=2).sum(1, dtype=torch.float64)
        vals.append((sxx + syy) / (s * (s - 1)) - 2 * kxy.sum((1, 2), dtype=torch.float64) / (s * s))
    v = torch.cat(vals)
    return v.mean().item(), v.std(unbiased=False).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="128,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--subsets", default="100,1000")
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-full", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    rng = np.random.default_rng(0)
    s = a.subset_size
    for d in map(int, a.dims.split(",")):
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        y = (torch.randn((a.n, d), generator=gen, device="cuda") + 0.05).half()
        for S in map(int, a.subsets.split(",")):
            ix = torch.from_numpy(np.stack([rng.choice(a.n, s, replace=False) for _ in range(S)]).astype(np.int32)).cuda()
            iy = torch.from_numpy(np.stack([rng.choice(a.n, s, replace=False) for _ in range(S)]).astype(np.int32)).cuda()
            fns = {"kid_subsets_ms": lambda: hip.kid_subsets(x, y, ix, iy)}
            if not a.no_torch:
                fns["torch_ms"] = lambda: torch_subsets(x, y, ix, iy, 1.0 / d)
            t = alternating(fns, a.reps)
            got = hip.kid_subsets(x, y, ix, iy)
            r = {"probe": "a", "D": d, "n": a.n, "subsets": S, "subset_size": s, **t, "kid_mean": got["mean"], "kid_std": got["std"]}
            if not a.no_torch:
                r["torch_mean"], r["torch_std"] = torch_subsets(x, y, ix, iy, 1.0 / d)
                r["speedup_min_over_min"] = round(min(t["torch_ms"]) / min(t["kid_subsets_ms"]), 2)
            print(json.dumps(r), flush=True)
            del ix, iy
        if not a.no_full:
            sigma = hip.kad_median_distance(x[:5000].contiguous())
            t = alternating({"kid_full_ms": lambda: hip.kid(x, y), "kad_gaussian_ms": lambda: hip.kad(x, y, bandwidth=sigma)}, a.reps)
            r = {"probe": "b", "D": d, "n": a.n, "m": a.n, **t, "kid": hip.kid(x, y)["mmd2"], "kad": hip.kad(x, y, bandwidth=sigma)["mmd2"],
                 "kid_over_kad_min": round(min(t["kid_full_ms"]) / min(t["kad_gaussian_ms"]), 3),
                 "kad_spread": round(max(t["kad_gaussian_ms"]) - min(t["kad_gaussian_ms"]), 3)}
            print(json.dumps(r), flush=True)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
