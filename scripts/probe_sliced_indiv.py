"""Per-song sliced Wasserstein timing (device events around whole calls): fad_sliced_individual on all songs in one call against the
only route there was before it, a loop of calc_sliced_wasserstein(x, song) over the same songs, in one process.

    python scripts/probe_sliced_indiv.py [--shapes 2000x2250x128,32x1500x768,10000x2x768] [--baseline 100000] [--projections 512]
                                         [--reps 3] [--loop-reps 1] [--once SxMxD]

Per shape S x M x D (S songs of M frames, fp16 rows on the device, a baseline of `baseline` rows, L = `projections` standard normal
directions), one JSON line:
  indiv_ms       hip.sliced_individual: both packs, the directions' image from the host, per chunk the baseline's projections and
                 global sort, the songs' projections, the resident song sort, the per-song match, the read-back of L x S sums; `reps`
                 runs after a warm-up, every run listed;
  loop_ms        the loop of hip.sliced_wasserstein(x, song_s) over the S songs, `loop-reps` runs after a warm-up of 3 calls (every call
                 of the loop re-packs the baseline, re-projects it and re-sorts it);
  equal_bits     every song's sw2_squared, std_error, max_sliced and max_index of the one call equal the loop's, bit for bit;
  plan           fad_sliced_individual_last_plan.
``--once SxMxD`` makes one warmed call and one timed call of the per-song entry alone at that shape: the command a kernel trace is taken of
(rocprofv3 --kernel-trace --stats -- python scripts/probe_sliced_indiv.py --once 2000x2250x128) for the split baseline sort /
projections / resident sort / match.  No counters run in it."""
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


def make(shape, baseline, gen):
    S, M, d = map(int, shape.split("x"))
    x = torch.randn((baseline, d), generator=gen, device="cuda").half()
    rows = (1.1 * torch.randn((S * M, d), generator=gen, device="cuda") + 0.05).half()
    shift = 0.02 * torch.arange(S, device="cuda").repeat_interleave(M).remainder(17).half()
    rows = rows + shift[:, None]                           # the songs differ from one another
    return S, M, d, x, rows, np.arange(S + 1, dtype=np.int64) * M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x2250x128,32x1500x768,10000x2x768")
    ap.add_argument("--baseline", type=int, default=100000)
    ap.add_argument("--projections", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    L = a.projections
    gen = torch.Generator(device="cuda").manual_seed(1)
    if a.once:
        S, M, d, x, rows, off = make(a.once, a.baseline, gen)
        theta = sliced_directions(d, L, 0)
        hip.sliced_individual(x, rows, off, theta)
        ms = once(lambda: hip.sliced_individual(x, rows, off, theta))
        print(json.dumps({"songs": S, "frames": M, "D": d, "n": a.baseline, "L": L, "indiv_ms": round(ms, 3),
                          "plan": hip.sliced_individual_last_plan()}), flush=True)
        return
    for shape in a.shapes.split(","):
        S, M, d, x, rows, off = make(shape, a.baseline, gen)
        theta = sliced_directions(d, L, 0)
        res = hip.sliced_individual(x, rows, off, theta)   # the warm-up
        indiv = [round(once(lambda: hip.sliced_individual(x, rows, off, theta)), 3) for _ in range(a.reps)]
        plan = hip.sliced_individual_last_plan()
        for s in range(3):
            hip.sliced_wasserstein(x, rows[off[s]:off[s + 1]], theta)
        singles = []

        def loop():
            singles.clear()
            for s in range(S):
                singles.append(hip.sliced_wasserstein(x, rows[off[s]:off[s + 1]], theta))
        loops = [round(once(loop), 3) for _ in range(a.loop_reps)]
        equal = all(np.float64(res[k][s]).tobytes() == np.float64(singles[s][k]).tobytes() for s in range(S)
                    for k in ("sw2_squared", "std_error", "max_sliced")) and all(res["max_index"][s] == singles[s]["max_index"] for s in range(S))
        print(json.dumps({"songs": S, "frames": M, "D": d, "n": a.baseline, "dtype": "fp16", "projections": L, "indiv_ms": indiv,
                          "loop_ms": loops, "loop_over_indiv_min": round(min(loops) / min(indiv), 2), "equal_bits": bool(equal),
                          "all_ok": bool(np.all(res["status"] == 0)), "plan": plan}), flush=True)
        del x, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
