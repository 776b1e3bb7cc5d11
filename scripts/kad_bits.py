#!/usr/bin/env python
"""The bits of every KAD-family entry on seeded inputs, for comparing two builds of the library byte for byte.

    python scripts/kad_bits.py > bits.txt

No arguments, one process, a few seconds on the GPU.  Every call writes a "## case" line, one line per output value -- float.hex() of
a float, the integer itself; an array of more than 16 values as its shape and the SHA-256 of its bytes -- and hip.kad_last_plan() on
one line, so two builds agree only if they give the same values AND cut their passes into the same launches.  What is printed is one
line per (family of inputs, entry): the number of its calls and the SHA-256 of all their lines, which keeps the two committed outputs
small; `--values` prints the lines themselves, to find the call and the value at which two builds part.  The list runs twice: with
FAD_KAD_LAUNCH_BUDGET unset, then at 1 (the floor of 64 tiles per launch, the small budget of tests/test_gpu_kad_launch_cut.py).  At
n = 300 and m = 200 that floor still holds every pass in one launch, so the last family (11 and 12 row blocks) is there for the budget
to cut into several launches.

profiles/kad_host_bits_parent.txt and profiles/kad_host_bits.txt are this script's output before and after the host side of kad.hip
was put on shared plumbing; they are identical.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fadtk_amd import hip  # noqa: E402

ENV = "FAD_KAD_LAUNCH_BUDGET"
DEV = torch.device("cuda", 0)
TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}
VALUES = "--values" in sys.argv[1:]
LINES = []                                     # the lines of the entry being run


def emit(tag, value):
    if isinstance(value, dict):
        for k in sorted(value):
            emit(f"{tag}.{k}" if tag else k, value[k])
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            emit(f"{tag}[{i}]", v)
    elif value is None:
        LINES.append(f"{tag} None")
    elif isinstance(value, torch.Tensor):
        emit(tag, value.cpu().numpy())
    elif isinstance(value, np.ndarray):
        a = np.ascontiguousarray(value)
        if a.size > 16:
            LINES.append(f"{tag} {a.dtype}{list(a.shape)} sha256 {hashlib.sha256(a.tobytes()).hexdigest()}")
        else:
            for i, v in enumerate(a.reshape(-1)):
                emit(f"{tag}[{i}]", v.item())
    elif isinstance(value, float):
        LINES.append(f"{tag} {value.hex()}")
    else:
        LINES.append(f"{tag} {int(value)}")


def call(tag, f):
    LINES.append(f"## {tag}")
    emit("", f())
    plan = hip.kad_last_plan()
    LINES.append("plan " + " ".join(f"{k}={plan[k]}" for k in sorted(plan)))


def entry_done(family_tag, entry):
    """print the entry's calls: their lines, or their count and the digest of the lines"""
    if VALUES:
        print(f"# {family_tag}")
        print("\n".join(LINES))
    else:
        calls = sum(line.startswith("## ") for line in LINES)
        print(f"{family_tag} | {entry} | calls={calls} sha256={hashlib.sha256(chr(10).join(LINES).encode()).hexdigest()}")
    LINES.clear()


def rows(a, dt, layout):
    """float32 numpy rows -> the rows as the case passes them: contiguous device rows, device rows at a pitch of D + 3, or host rows"""
    if layout == "host":
        return a.astype(np.float16) if dt == "float16" else a.astype(np.float32)
    t = torch.from_numpy(a).to(DEV).to(TORCH_DT[dt])
    if layout == "pitch":
        buf = torch.zeros((t.shape[0], t.shape[1] + 3), dtype=t.dtype, device=DEV)
        buf[:, :t.shape[1]] = t
        return buf[:, :t.shape[1]]
    return t


def labellings(n, m, P, rng):
    u = np.zeros((P, n + m), dtype=bool)
    for p in range(P):
        u[p, rng.permutation(n + m)[:n]] = True
    return hip.pack_labels(u)


def family(tag, n, m, d, dt, layout, many_labellings):
    rng = np.random.default_rng(1000 * d + n)
    x32 = rng.standard_normal((n, d)).astype(np.float32)
    y32 = (1.1 * rng.standard_normal((m, d)) + 0.2).astype(np.float32)
    y2_32 = (0.9 * rng.standard_normal((3 * m // 4, d)) - 0.1).astype(np.float32)
    x, y, y2 = rows(x32, dt, layout), rows(y32, dt, layout), rows(y2_32, dt, layout)
    given = 0.9 * float(np.sqrt(2.0 * d))
    factors = [0.5, 1.0, 2.0, 0.75, 1.5, 3.0, 0.25, 1.25, 4.0]
    labs = {P: labellings(n, m, P, rng) for P in ((40, 1100) if many_labellings else (40,))}

    call("median", lambda: hip.kad_median_distance(x))
    entry_done(tag, "median")
    for kernel in ("gaussian", "iq", "imq"):
        for bw in (None, given):
            call(f"kad {kernel} bw={bw is not None}", lambda: hip.kad(x, y, bandwidth=bw, kernel=kernel))
    entry_done(tag, "kad")
    for B in (1, 3, 5, 9):
        call(f"sweep factors B={B}", lambda: hip.kad_sweep(x, y, factors=factors[:B]))
    call("sweep bandwidths B=3", lambda: hip.kad_sweep(x, y, bandwidths=[given * f for f in factors[:3]]))
    entry_done(tag, "sweep")
    for P, words in labs.items():
        for bw in (None, given):
            call(f"permutation_test P={P} bw={bw is not None}", lambda: hip.kad_permutation_test(x, y, words, bandwidth=bw))
    entry_done(tag, "permutation_test")
    for P, words in labs.items():
        for B in (1, 2, 3, 5):
            call(f"permutation_sweep P={P} factors B={B}", lambda: hip.kad_permutation_sweep(x, y, words, factors=factors[:B]))
        call(f"permutation_sweep P={P} bandwidths B=1", lambda: hip.kad_permutation_sweep(x, y, words, bandwidths=[given]))
    entry_done(tag, "permutation_sweep")
    offsets = [0, m // 4, m // 4, 2 * m // 3, m]                                  # four songs, the second one empty
    for bw in (None, given):
        call(f"individual bw={bw is not None}", lambda: hip.kad_individual(x, y, offsets, bandwidth=bw))
    entry_done(tag, "individual")
    for bw in (None, given):
        call(f"uncertainty bw={bw is not None}", lambda: hip.kad_uncertainty(x, [y, y2], bandwidth=bw, rows=True))
    entry_done(tag, "uncertainty")
    for k in (1, 5):
        call(f"prdc k={k}", lambda: hip.prdc(x, y, k=k, details=True))
    entry_done(tag, "prdc")
    for k in (1, 5):
        call(f"nearest k={k}", lambda: hip.nearest(x, y, k=k, authenticity=True))
    entry_done(tag, "nearest")
    for k in (1, 3):
        call(f"nn_test k={k}", lambda: hip.nn_test(x, y, labs[40], k=k, return_graph=True))
    entry_done(tag, "nn_test")
    call("kid", lambda: hip.kid(x, y))
    entry_done(tag, "kid")
    ix, iy = rng.integers(0, n, (7, 96)), rng.integers(0, m, (7, 96))
    if layout != "host":
        ix, iy = torch.from_numpy(ix).to(DEV), torch.from_numpy(iy).to(DEV)
    call("kid_subsets", lambda: hip.kid_subsets(x, y, ix, iy))
    entry_done(tag, "kid_subsets")


def everything():
    for d in (70, 512):
        for dt in ("float16", "bfloat16", "float32"):
            family(f"n=300 m=200 d={d} {dt}", 300, 200, d, dt, "device", True)
    family("n=300 m=200 d=70 float16 pitch=73", 300, 200, 70, "float16", "pitch", True)
    family("n=300 m=200 d=70 float32 host", 300, 200, 70, "float32", "host", True)
    family("n=300 m=200 d=70 float16 host", 300, 200, 70, "float16", "host", True)
    # 11 and 12 row blocks: at the small budget every pass of these calls takes several launches
    family("n=1290 m=1410 d=70 float16", 1290, 1410, 70, "float16", "device", False)


def main():
    os.environ.pop(ENV, None)
    print("# budget unset")
    everything()
    os.environ[ENV] = "1"
    print("# budget 1")
    everything()
    os.environ.pop(ENV, None)


if __name__ == "__main__":
    main()
