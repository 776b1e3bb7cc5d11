"""Sliced Wasserstein timing (device events around whole library calls), several runs each, alternating in one process with a torch
formulation on the same GPU.

    python scripts/probe_sliced.py [--sizes 10000,100000] [--dims 128,512] [--projections 512] [--reps 3] [--once N,D]

Per (n = m, D), fp16 rows on the device, L = `projections` standard normal directions, one JSON line:
  sliced_ms      fad_sliced_wasserstein: the two packs, the directions' image from the host, projections, both sorts, the match, the
                 read-back of L sums;
  torch_ms       the same distance in torch: x.float() @ theta.T, torch.sort along the rows, the mean squared difference per direction
                 over the squared length of the direction (theta rounded to fp16 first, as the library rounds it); it holds both
                 L x n float32 matrices twice over (values and sort output);
  sw2_squared and torch_sw2_squared must agree (float32 projections either way, the float32 sum of squares on torch's side);
  plan           fad_sliced_last_plan: chunks, directions per chunk, sort passes, workgroups per segment.
Every run's time is listed, so the spread between runs shows next to the differences.  ``--once N,D`` makes one warmed call and one
timed call of the library alone at that shape and prints nothing else: the command a kernel trace is taken of
(rocprofv3 --kernel-trace --stats -- python scripts/probe_sliced.py --once 100000,128), for the split projection / sort / match."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402
from fadtk_amd.sliced import sliced_directions  # noqa: E402


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


def torch_sliced(x, y, theta_dev, q_dev):
    a = torch.sort(x.float() @ theta_dev.T, dim=0).values
    b = torch.sort(y.float() @ theta_dev.T, dim=0).values
    w = ((a - b) ** 2).mean(dim=0).double() / q_dev
    return w.mean().item()


def rows(n, d, gen):
    x = torch.randn((n, d), generator=gen, device="cuda").half()
    y = (1.1 * torch.randn((n, d), generator=gen, device="cuda") + 0.05).half()
    return x, y


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
        hip.sliced_wasserstein(x, y, theta)
        print(json.dumps({"n": n, "D": d, "L": L, "sliced_ms": round(once(lambda: hip.sliced_wasserstein(x, y, theta)), 3)}), flush=True)
        return
    for n in map(int, a.sizes.split(",")):
        for d in map(int, a.dims.split(",")):
            x, y = rows(n, d, gen)
            theta = sliced_directions(d, L, 0)
            theta_dev = torch.from_numpy(theta).cuda().half().float()
            q_dev = (theta_dev.double() ** 2).sum(dim=1)
            fns = {"sliced_ms": lambda: hip.sliced_wasserstein(x, y, theta), "torch_ms": lambda: torch_sliced(x, y, theta_dev, q_dev)}
            t = alternating(fns, a.reps)
            res = hip.sliced_wasserstein(x, y, theta)
            r = {"n": n, "m": n, "D": d, "dtype": "fp16", "projections": L, **t, "sw2_squared": res["sw2_squared"],
                 "std_error": res["std_error"], "torch_sw2_squared": torch_sliced(x, y, theta_dev, q_dev), "plan": hip.sliced_last_plan(),
                 "torch_over_sliced_min": round(min(t["torch_ms"]) / min(t["sliced_ms"]), 2)}
            print(json.dumps(r), flush=True)
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
