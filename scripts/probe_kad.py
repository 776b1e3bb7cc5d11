"""KAD kernel timing (device events around single library calls) against a torch formulation that writes the pair matrix.

    python scripts/probe_kad.py [--n 100000] [--dims 512,128,1024] [--reps 3] [--no-torch] [--dup F] [--kernel gaussian,iq,imq]

Per D: the median pass (fad_kad_median_distance), the three sum passes at a fixed bandwidth (fad_kad), the XX pass alone (fad_kad
against a 2-row set), their issued MFMA TFLOP/s (128 x 128 tiles x padded depth x 2, the masked halves of diagonal tiles included),
the share of the 2.5 PF fp16 spec and of the 1.64 PF measured ceiling, and chunked torch fp16 matmul + exp + sum
(--no-torch leaves it out).  --dup F: the first F of the baseline rows are copies of row 0 (d^2 = 0 for most pairs: every histogram
count lands in one bin, the worst case of the median's LDS atomics).  --kernel: one line per D and kernel, in one process (the median
and the torch formulation are timed with the first kernel only; the torch pass is the Gaussian's); the first line also carries
`s_first_call`, the wall time of the process's first KAD call, which loads KAD's code object.  Under `rocprofv3 --kernel-trace --stats` the longest single
launch of each kernel is the `max_us` column of scripts/rocpd_summary.py."""
import argparse
import json
import sys
import time
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


def torch_pass(x, y, sigma, chunk=8192):
    g = 1.0 / (2 * sigma * sigma)
    nx, ny = (x.float() ** 2).sum(1), (y.float() ** 2).sum(1)
    tot = torch.zeros((), dtype=torch.float64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        s = (x[i:i + chunk] @ y.T).float()
        tot += torch.exp(-g * (nx[i:i + chunk, None] + ny[None, :] - 2 * s).clamp_min_(0)).sum(dtype=torch.float64)
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="512,128,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dup", type=float, default=0.0)
    ap.add_argument("--kernel", default="gaussian", help="comma-separated: gaussian, iq, imq")
    a = ap.parse_args()
    kernels = a.kernel.split(",")
    for k in kernels:
        hip.kad_kernel_code(k)
    first_call = None
    gen = torch.Generator(device="cuda").manual_seed(1)
    out = []
    for d in map(int, a.dims.split(",")):
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        y = (torch.randn((a.n, d), generator=gen, device="cuda") + 0.05).half()
        if a.dup > 0:
            x[: int(a.dup * a.n)] = x[0]
        y2 = y[:2].contiguous()
        t0 = time.perf_counter()
        sigma = hip.kad_median_distance(x)
        if first_call is None:
            first_call = time.perf_counter() - t0
        dp = -(-d // 64) * 64
        T = -(-a.n // 128)
        tile_flop = 128 * 128 * dp * 2
        tri, rect = T * (T + 1) // 2, T * T
        t_med = timed(lambda: hip.kad_median_distance(x), a.reps)
        t_torch = None if a.no_torch else timed(lambda: torch_pass(x, x, sigma) + torch_pass(y, y, sigma) - 2 * torch_pass(x, y, sigma), 1)
        f_sum = (2 * tri + rect) * tile_flop
        for kernel in kernels:
            t_sum = timed(lambda: hip.kad(x, y, bandwidth=sigma, kernel=kernel), a.reps)
            t_xx = timed(lambda: hip.kad(x, y2, bandwidth=sigma, kernel=kernel), a.reps)
            first = kernel == kernels[0]
            r = {"d": d, "n": a.n, "dup": a.dup, "kernel": kernel, "sigma": sigma, "ms_median_3_passes": t_med if first else None,
                 "ms_kad_3_passes": t_sum, "ms_xx_pass": t_xx, "ms_torch_matmul_exp_sum": t_torch if first else None,
                 "tflops_kad": f_sum / t_sum / 1e9, "tflops_xx": tri * tile_flop / t_xx / 1e9}
            r["share_of_2p5_pf"] = r["tflops_kad"] / 2500
            r["share_of_1p64_pf"] = r["tflops_kad"] / 1640
            r["speedup_vs_torch"] = t_torch / t_sum if t_torch and first else None
            if not out:
                r["s_first_call"] = first_call
            print(json.dumps(r), flush=True)
            out.append(r)
        del x, y, y2
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
