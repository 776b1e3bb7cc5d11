"""Nearest-neighbour timing (device events around whole library calls) against a chunked torch formulation (cdist + topk).

    python scripts/probe_nearest.py [--n 100000] [--dims 512,128,1024] [--ks 1,5] [--reps 3] [--no-torch]

Per D, fp16, n = m, and k: the nearest pass alone (fad_nearest without authenticity) and the whole call with authenticity (plus the
radius pass of X with k = 1); fad_prdc's radius pass of X alone (fad_prdc of X against k + 1 rows, as scripts/probe_prdc.py times it)
and fad_kad at a fixed bandwidth over the same sets (XX + YY triangles and XY) for their pair rates; each pass's pair rate against
them.  The torch formulation: torch.cdist in float32 on chunks of evaluation rows, topk over the baseline; its indices are compared
with the library's (rows whose k-lists differ, and whether each differing row is a near tie)."""
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


def torch_nearest(x, y, k, chunk=4096):
    xf, yf = x.float(), y.float()
    idx = torch.empty((y.shape[0], k), dtype=torch.int64, device=x.device)
    dist = torch.empty((y.shape[0], k), device=x.device)
    for i in range(0, y.shape[0], chunk):
        t = torch.topk(torch.cdist(yf[i:i + chunk], xf), k, dim=1, largest=False)
        dist[i:i + chunk], idx[i:i + chunk] = t.values, t.indices
    return dist, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="512,128,1024")
    ap.add_argument("--ks", default="1,5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    n = a.n
    out = []
    for d in map(int, a.dims.split(",")):
        x = torch.randn((n, d), generator=gen, device="cuda").half()
        y = (torch.randn((n, d), generator=gen, device="cuda") * 1.05 + 0.03).half()
        t_kad = timed(lambda: hip.kad(x, y, bandwidth=float(d) ** 0.5), a.reps)
        kad_rate = (n * n / 2 + n * n / 2 + n * n) / (t_kad * 1e-3)
        for k in map(int, a.ks.split(",")):
            ys = y[:k + 1].contiguous()
            t_near = timed(lambda: hip.nearest(x, y, k=k, authenticity=False), a.reps)
            t_all = timed(lambda: hip.nearest(x, y, k=k, authenticity=True), a.reps)
            t_prdc_rx = timed(lambda: hip.prdc(x, ys, k=k), a.reps)
            res = hip.nearest(x, y, k=k, authenticity=True)
            row = {"D": d, "n": n, "k": k, "nearest_ms": round(t_near, 2), "nearest_auth_ms": round(t_all, 2),
                   "prdc_radius_ms": round(t_prdc_rx, 2), "kad_ms": round(t_kad, 2), "kad_pairs_per_s": kad_rate,
                   "nearest_vs_prdc_radius": round(t_near / t_prdc_rx, 3),
                   "nearest_rate_vs_kad": round(n * n / (t_near * 1e-3) / kad_rate, 3),
                   "auth_call_rate_vs_kad": round(2 * n * n / (t_all * 1e-3) / kad_rate, 3),
                   "authenticity": res["authenticity"], "copied": res["copied"]}
            if not a.no_torch:
                torch.cuda.synchronize()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                dist, idx = torch_nearest(x, y, k)
                ev[1].record()
                torch.cuda.synchronize()
                row["torch_ms"] = round(ev[0].elapsed_time(ev[1]), 1)
                row["speedup"] = round(row["torch_ms"] / t_near, 1)
                mine = torch.from_numpy(res["index"].astype("int64")).cuda()
                diff = (mine != idx).any(1)
                row["rows_differing_from_torch"] = int(diff.sum().item())
                if row["rows_differing_from_torch"]:             # a differing row whose k-th distances agree to 1e-3 is a near tie
                    mine_d = torch.from_numpy(res["dist2"]).cuda().sqrt()
                    row["differing_rows_not_near_ties"] = int(((mine_d - dist).abs().max(1).values > 1e-3 * dist[:, -1])[diff].sum().item())
            print(json.dumps(row), flush=True)
            out.append(row)
        del x, y
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
