"""k-means timing (device events around whole library calls) against fad_nearest on the same shape and against a torch formulation.

    python scripts/probe_kmeans.py [--n 100000] [--dims 128,512] [--ks 20,1000,10000] [--iters 5] [--reps 3] [--no-torch] [--one D,K]

Per D and K, fp16, two sets of n rows pooled (N = 2 n), init = K pooled rows (fadtk_amd.mauve.seed_rows):
  - fad_kmeans with max_iter = iters and with max_iter = 0 (a pure assignment); the time per iteration is their difference over iters
    (pack, planes of the init and the closing assignment are in both);
  - fad_nearest with k = 1 on the same centroid / row shape (the centroids rounded to fp16 as the baseline, the pooled rows as the
    evaluation set): one assignment's main loop at ONE plane -- expect the pure assignment at roughly `planes` times that;
  - a torch formulation of one iteration (float32 matmul + argmin in chunks, index_add_ + division), alternated with the library in one
    process, three runs each after a warm-up.
The assign / sort / update split comes from a kernel trace of `--one D,K` (one shape, no torch), a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/probe_kmeans.py --one 512,10000
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fadtk_amd import hip  # noqa: E402
from fadtk_amd.mauve import seed_rows  # noqa: E402


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


def torch_iteration(z, c, chunk=8192):
    """one Lloyd iteration in float32: labels by matmul + argmin, means by index_add_ (empty clusters keep their centroid)"""
    c2 = (c * c).sum(1)
    labels = torch.empty(z.shape[0], dtype=torch.int64, device=z.device)
    for i in range(0, z.shape[0], chunk):
        labels[i:i + chunk] = (c2[None, :] - 2.0 * (z[i:i + chunk] @ c.T)).argmin(1)
    sums = torch.zeros_like(c).index_add_(0, labels, z)
    counts = torch.bincount(labels, minlength=c.shape[0]).to(c.dtype)
    return torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], c), labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="128,512")
    ap.add_argument("--ks", default="20,1000,10000")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--one", default=None, help="D,K: one shape, library only (for a kernel trace)")
    a = ap.parse_args()
    shapes = [(d, k) for d in map(int, a.dims.split(",")) for k in map(int, a.ks.split(","))]
    if a.one:
        shapes, a.no_torch = [tuple(map(int, a.one.split(",")))], True
    gen = torch.Generator(device="cuda").manual_seed(1)
    n = a.n
    rows = {}
    for d, k in shapes:
        if d not in rows:
            rows.clear()
            torch.cuda.empty_cache()
            centres = torch.randn((64, d), generator=gen, device="cuda") * 2.0
            pick = torch.randint(0, 64, (2 * n,), generator=gen, device="cuda")
            z = (torch.randn((2 * n, d), generator=gen, device="cuda") + centres[pick]).half()
            rows[d] = (z[:n].contiguous(), z[n:].contiguous(), z)
        x, y, z = rows[d]
        init = z[torch.from_numpy(seed_rows(2 * n, k, 0, 0)).cuda()].float().cpu().numpy()
        t_assign = timed(lambda: hip.kmeans([x, y], init, iterations=0, return_dist2=False), a.reps)
        t_loop = timed(lambda: hip.kmeans([x, y], init, iterations=a.iters, return_dist2=False), a.reps)
        res = hip.kmeans([x, y], init, iterations=a.iters, return_dist2=False)
        plan = hip.kmeans_last_plan()
        per_iter = (t_loop - t_assign) / max(res["iterations"], 1)
        row = {"D": d, "N": 2 * n, "K": k, "planes": plan["planes"], "iterations": res["iterations"], "assign_call_ms": round(t_assign, 2),
               "loop_call_ms": round(t_loop, 2), "ms_per_iteration": round(per_iter, 2), "assign_launches": plan["assign_launches"],
               "max_chunks": plan["max_chunks"], "inertia": res["inertia"]}
        if k >= 2:                                             # fad_nearest refuses a baseline of one row only with authenticity
            base = torch.from_numpy(init).cuda().half()
            t_near = timed(lambda: hip.nearest(base, z, k=1, authenticity=False), a.reps)
            row["nearest_k1_ms"] = round(t_near, 2)
            row["assign_vs_nearest"] = round(t_assign / t_near, 2)
            row["iteration_vs_nearest"] = round(per_iter / t_near, 2)
        if not a.no_torch:
            zf, c0 = z.float(), torch.from_numpy(init).cuda()
            torch_iteration(zf, c0)                            # warm-up
            ts, tl = [], []
            for _ in range(a.reps):                            # alternated with the library in one process
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                c = c0
                for _ in range(a.iters):
                    c, labels = torch_iteration(zf, c)
                ev[1].record()
                torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]) / a.iters)
                tl.append(timed(lambda: hip.kmeans([x, y], init, iterations=a.iters, return_dist2=False), 1))
            row["torch_ms_per_iteration"] = round(min(ts), 2)
            row["loop_call_ms_alternated"] = round(min(tl), 2)
            row["speedup_per_iteration"] = round(min(ts) / max(per_iter, 1e-9), 1)
            agree = (labels.cpu().numpy() == hip.kmeans([x, y], c.cpu().numpy(), iterations=0, return_dist2=False)["labels"]).mean()
            row["labels_agreeing_with_torch"] = round(float(agree), 5)
            del zf
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    main()
