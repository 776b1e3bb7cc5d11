"""Per-song KAD timing (device events around single library calls): fad_kad_individual against fad_kad on the same rows and against
the loop of one fad_kad call per song.

    python scripts/probe_kad_individual.py [--n 100000] [--reps 3] [--loop-songs 100] [--shapes 10000x2x768,32x1500x768,2000x2250x128]

Per shape (S songs x m frames x D, float16, a baseline of n rows):
  - ms_indiv_bw: fad_kad_individual with the bandwidth given (pack, XX triangle, cross pass, band pass, per-song reduction);
  - ms_indiv_median: the same without it (adds the three histogram passes of the median);
  - ms_xx: fad_kad(x, 2 rows) -- the baseline's pack and XX triangle, the part fad_kad_individual does once;
  - ms_fad_kad_cat: fad_kad(x, Y) over the concatenated song rows (XX + YY + XY; left out when YY would exceed --max-yy-tiles) and
    ms_yy: fad_kad(2 rows, Y) (YY + a 2-row XY), so that ms_fad_kad_cat - ms_xx - ms_yy estimates fad_kad's XY pass;
  - ms_loop_per_song: one fad_kad(x, song) per song over --loop-songs songs (median bandwidth, as a caller without one would run it),
    and the loop's time extrapolated to all S songs.
Cross pass pairs/s against fad_kad's XY pass: the cross and band kernels' times come from `rocprofv3 --kernel-trace --stats` on this
script (kad_cols_kernel<*, false> / <*, true>; scripts/rocpd_summary.py), the XY estimate from the events above."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-songs", type=int, default=100)
    ap.add_argument("--shapes", default="10000x2x768,32x1500x768,2000x2250x128")
    ap.add_argument("--max-yy-tiles", type=int, default=20_000_000)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    for shape in a.shapes.split(","):
        S, m, d = map(int, shape.split("x"))
        x = torch.randn((a.n, d), generator=gen, device="cuda").half()
        y = (torch.randn((S * m, d), generator=gen, device="cuda") + 0.05).half()
        off = np.arange(S + 1, dtype=np.int64) * m
        sigma = hip.kad_median_distance(x)
        x2 = x[:2].contiguous()
        y2 = y[:2].contiguous()
        M, TI, TJ = S * m, -(-a.n // 128), -(-(S * m) // 128)
        r = {"songs": S, "frames": m, "d": d, "n": a.n, "sigma": sigma}
        r["ms_indiv_bw"] = timed(lambda: hip.kad_individual(x, y, off, bandwidth=sigma), a.reps)
        r["ms_indiv_median"] = timed(lambda: hip.kad_individual(x, y, off), a.reps)
        r["ms_xx"] = timed(lambda: hip.kad(x, y2, bandwidth=sigma), a.reps)
        if TJ * (TJ + 1) // 2 <= a.max_yy_tiles:
            r["ms_fad_kad_cat"] = timed(lambda: hip.kad(x, y, bandwidth=sigma), a.reps)
            r["ms_yy"] = timed(lambda: hip.kad(x2, y, bandwidth=sigma), a.reps)
            r["ms_xy_estimate"] = r["ms_fad_kad_cat"] - r["ms_xx"] - r["ms_yy"]
            r["xy_pairs_per_s_fad_kad"] = a.n * M / (r["ms_xy_estimate"] * 1e-3)
        k = min(a.loop_songs, S)

        def loop():
            for s in range(k):
                hip.kad(x, y[off[s]:off[s + 1]])
        r["ms_loop_per_song"] = timed(loop, 1) / k
        r["s_loop_all_songs_extrapolated"] = r["ms_loop_per_song"] * S / 1e3
        r["speedup_vs_loop_median"] = r["ms_loop_per_song"] * S / r["ms_indiv_median"]
        r["cross_tiles"], r["cross_pairs"] = TI * TJ, a.n * M
        print(json.dumps(r), flush=True)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
