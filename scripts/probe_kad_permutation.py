"""KAD permutation-test timing (device events around single calls): fad_kad_permutation_test against fad_kad on the same rows, the
bandwidth given to both, and a torch formulation of the same statistics.

    python scripts/probe_kad_permutation.py [--n 100000] [--m 100000] [--d 128,512,1024] [--perms 100,1000] [--reps 3]
    python scripts/probe_kad_permutation.py --d 512 --perms 1000 --reps 1 --no-torch          (under rocprofv3)

Per (D, P), float16 rows: ms_call (the whole call: pack, labels and their layouts, the r pass, the permutation pass, the statistics),
ms_labels (P seeded labellings generated and packed on the device), ms_kad (one fad_kad(x, y)) and their ratio; with torch, ms_torch:
K in chunks of 8192 rows (f16 GEMM for the distances, f16 or f32 exponentials) times the 0/1 labelling matrix U [N x (P + 1)] on
rocBLAS, the full square.  The r pass, the permutation pass and the longest launch come from `rocprofv3 --kernel-trace --stats`."""
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


def torch_form(x, y, U, sigma, kdtype, chunk=8192):
    """t for every column of U from K' (chunked, full square) times U on rocBLAS"""
    z = torch.cat([x, y])
    N, n, m = z.shape[0], x.shape[0], y.shape[0]
    nz = (z.float() * z.float()).sum(1)
    g = 1.0 / (2.0 * sigma * sigma)
    KU = torch.empty((N, U.shape[1]), dtype=torch.float32, device=z.device)
    r = torch.empty(N, dtype=torch.float32, device=z.device)
    Uk = U.to(kdtype)
    for i0 in range(0, N, chunk):
        zc = z[i0:i0 + chunk]
        d2 = (nz[i0:i0 + chunk, None] + nz[None, :] - 2.0 * (zc @ z.T).float()).clamp_min_(0)
        k = torch.exp(-g * d2)
        idx = torch.arange(zc.shape[0], device=z.device)
        k[idx, idx + i0] = 0.0
        r[i0:i0 + chunk] = k.sum(1)
        KU[i0:i0 + chunk] = (k.to(kdtype) @ Uk).float()
    q = (U * KU).sum(0).double()
    R = (U.T @ r).double()
    T = r.double().sum()
    return q / (n * (n - 1.0)) + (T - 2 * R + q) / (m * (m - 1.0)) - 2 * (R - q) / (n * m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--d", default="128,512,1024")
    ap.add_argument("--perms", default="100,1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(5)
    out = []
    for d in [int(v) for v in a.d.split(",")]:
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        y = (torch.randn((a.m, d), generator=gen, device="cuda") * 1.05 + 0.02).half()
        sigma = hip.kad_median_distance(torch.cat([x, y]))
        ms_kad = timed(lambda: hip.kad(x, y, bandwidth=sigma), a.reps)
        for P in [int(v) for v in a.perms.split(",")]:
            lab = random_labellings(a.n, a.m, P, seed=1)
            ms_lab = timed(lambda: random_labellings(a.n, a.m, P, seed=1), a.reps)
            res = {}

            def call():
                res.update(hip.kad_permutation_test(x, y, lab, bandwidth=sigma))
            ms_call = timed(call, a.reps)
            row = {"n": a.n, "m": a.m, "d": d, "P": P, "ms_call": round(ms_call, 2), "ms_labels": round(ms_lab, 2),
                   "ms_kad": round(ms_kad, 2), "call_over_kad": round(ms_call / ms_kad, 2), "p_value": res["p_value"],
                   "mmd2": res["mmd2"]}
            out.append(row)
            print(json.dumps(row), flush=True)
    if not a.no_torch:
        d, P = 512, 1000
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        y = (torch.randn((a.m, d), generator=gen, device="cuda") * 1.05 + 0.02).half()
        sigma = hip.kad_median_distance(torch.cat([x, y]))
        lab = random_labellings(a.n, a.m, P, seed=1)
        N = a.n + a.m
        shifts = torch.arange(32, device="cuda", dtype=torch.int64)
        bits = ((lab.to(torch.int64) & 0xffffffff)[:, :, None] >> shifts) & 1
        U = torch.cat([torch.cat([torch.ones(a.n), torch.zeros(a.m)]).cuda()[None], bits.reshape(P, -1)[:, :N].float()]).T.contiguous()
        mine = hip.kad_permutation_test(x, y, lab, bandwidth=sigma)
        for kdt in (torch.float16, torch.float32):
            tt = {}
            ms = timed(lambda: tt.update(t=torch_form(x, y, U, sigma, kdt)), 1)
            t = tt["t"].cpu().numpy()
            sd = float(t[1:].std())
            row = {"torch": str(kdt), "d": d, "P": P, "ms_torch": round(ms, 1), "max_dt_over_sd_vs_library":
                   float(max(abs(t[0] - mine["mmd2"]), abs(t[1:] - mine["null"]).max()) / sd)}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
