"""PRDC timing (device events around whole library calls) against a chunked torch formulation (cdist + topk, then threshold counts).

    python scripts/probe_prdc.py [--n 100000] [--dims 512,128,1024] [--k 5] [--reps 3] [--no-torch] [--big]

Per D, fp16, n = m: the whole fad_prdc call; the radius pass of X alone (fad_prdc of X against k + 1 rows) and of Y alone (k + 1 rows
against Y), the cross pass as the difference; fad_kad at a fixed bandwidth over the same sets (XX + YY triangles and XY, n^2 / 2 +
m^2 / 2 + n m pairs) for its pair rate; each pass's pair rate against it.  The torch formulation: torch.cdist in float32 on chunks of
rows, topk for the radii, then the two threshold tests in chunks; its results are compared with the library's.  --big adds one call at
n = m = 10^6, D = 128 (per-launch times: run under `rocprofv3 --kernel-trace --stats`, the `max_us` column of scripts/rocpd_summary.py)."""
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


def torch_prdc(x, y, k, chunk=4096):
    xf, yf = x.float(), y.float()

    def radii(a):
        r = torch.empty(a.shape[0], device=a.device)
        for i in range(0, a.shape[0], chunk):
            r[i:i + chunk] = torch.topk(torch.cdist(a[i:i + chunk], a), k + 1, dim=1, largest=False).values[:, k]
        return r
    rx, ry = radii(xf), radii(yf)
    balls = torch.zeros(y.shape[0], dtype=torch.int64, device=x.device)
    rec = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    cov = torch.zeros_like(rec)
    for i in range(0, x.shape[0], chunk):
        dd = torch.cdist(xf[i:i + chunk], yf)
        p1 = dd < rx[i:i + chunk, None]
        balls += p1.sum(0)
        cov[i:i + chunk] = p1.any(1)
        rec[i:i + chunk] = (dd < ry[None, :]).any(1)
    n, m = x.shape[0], y.shape[0]
    return {"precision": (balls > 0).sum().item() / m, "recall": rec.sum().item() / n, "density": balls.sum().item() / (k * m),
            "coverage": cov.sum().item() / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="512,128,1024")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--big", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    n, k = a.n, a.k
    out = []
    for d in map(int, a.dims.split(",")):
        x = torch.randn((n, d), generator=gen, device="cuda").half()
        y = (torch.randn((n, d), generator=gen, device="cuda") * 1.05 + 0.03).half()
        xs, ys = x[:k + 1].contiguous(), y[:k + 1].contiguous()
        t_all = timed(lambda: hip.prdc(x, y, k=k), a.reps)
        t_rx = timed(lambda: hip.prdc(x, ys, k=k), a.reps)
        t_ry = timed(lambda: hip.prdc(xs, y, k=k), a.reps)
        t_kad = timed(lambda: hip.kad(x, y, bandwidth=float(d) ** 0.5), a.reps)
        kad_rate = (n * n / 2 + n * n / 2 + n * n) / (t_kad * 1e-3)
        t_cross = t_all - t_rx - t_ry
        res = hip.prdc(x, y, k=k)
        row = {"D": d, "n": n, "k": k, "prdc_ms": round(t_all, 2), "radius_x_ms": round(t_rx, 2), "radius_y_ms": round(t_ry, 2),
               "cross_ms_est": round(t_cross, 2), "kad_ms": round(t_kad, 2), "kad_pairs_per_s": kad_rate,
               "radius_rate_vs_kad": round(n * n / (t_rx * 1e-3) / kad_rate, 3),
               "cross_rate_vs_kad": round(n * n / (t_cross * 1e-3) / kad_rate, 3) if t_cross > 0 else None,
               **{key: res[key] for key in ("precision", "recall", "density", "coverage")}}
        if not a.no_torch:
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            ref = torch_prdc(x, y, k)
            ev[1].record()
            torch.cuda.synchronize()
            row["torch_ms"] = round(ev[0].elapsed_time(ev[1]), 1)
            row["speedup"] = round(row["torch_ms"] / t_all, 1)
            row["torch_values"] = ref
        print(json.dumps(row), flush=True)
        out.append(row)
        del x, y
        torch.cuda.empty_cache()
    if a.big:
        nb = 1_000_000
        x = torch.randn((nb, 128), generator=gen, device="cuda").half()
        y = (torch.randn((nb, 128), generator=gen, device="cuda") * 1.05 + 0.03).half()
        t = timed(lambda: hip.prdc(x, y, k=k), 1)
        row = {"D": 128, "n": nb, "k": k, "prdc_ms": round(t, 1)}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


if __name__ == "__main__":
    main()
