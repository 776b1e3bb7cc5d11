"""np.mean's float32 running column sums written out plainly, rows on which the ORDER of those sums shows, and the case
tables that test_running_sum_host.py (CPU: the rows discriminate) and test_gpu_running_sums.py (GPU: the walks reproduce the sums)
share.  Nothing here touches a GPU.

float16 frames have 11 significant bits: a float32 sum of a few thousand of them at ONE scale is exact and every order gives the same
bits.  `hostile_rows` spreads every column over 25 binades (+-m 2^e, e = -10 .. 14): 36 bits of span against float32's 24, so every add
rounds, and regrouping, merging partial sums or one row too many changes the sum in most columns at any row count from a few dozen."""
import functools

import numpy as np

DTYPES = ("float16", "bfloat16", "float32")


# --------------------------------------------------------------------------------- the reference
def as_f32(x):
    """The stored values as float32 (exact for float16 and bfloat16: the kernels widen the same way)."""
    if type(x).__module__.split(".")[0] == "torch":
        import torch
        return x.to(torch.float32).numpy()
    return np.asarray(x).astype(np.float32)


def running_sum(xf32, start=None):
    """s = s + row in float32, the rows one after the other."""
    xf32 = np.asarray(xf32)
    assert xf32.dtype == np.float32 and xf32.ndim == 2
    s = np.zeros(xf32.shape[1], dtype=np.float32) if start is None else np.array(start, dtype=np.float32)
    with np.errstate(all="ignore"):                     # (Inf - Inf = NaN is part of the contract)
        for row in xf32:
            s = s + row
    assert s.dtype == np.float32
    return s


def mean_of(run, n):
    """What finalize returns for a float32 running sum: float32(float64(run) / n), widened (fad_common.h: numpy_mean_of_f32_sum)."""
    with np.errstate(all="ignore"):
        return np.float64(np.float32(np.float64(run) / n))


# --------------------------------------------------------------------------------- rows
def hostile_rows(rng, n, d, dtype):
    """[n x d] of +-m 2^e, m in [1, 2), e uniform in -10 .. 14, rounded to the storage type: float16 / float32 numpy arrays, bfloat16 a
    torch CPU tensor.  |x| <= 2^15, which float16 holds."""
    x = (1.0 + rng.random((n, d))) * np.exp2(rng.integers(-10, 15, size=(n, d))) * rng.choice((-1.0, 1.0), size=(n, d))
    if dtype == "bfloat16":
        import torch
        return torch.from_numpy(x).to(torch.bfloat16)
    return x.astype(dtype)


@functools.lru_cache(maxsize=None)
def rows_for(dtype, d, n, tag=0):
    """The hostile rows of one case: a function of (dtype, d, n, tag) alone, so that the host test judges the very rows the GPU test feeds.
    Treat the result as read-only."""
    return hostile_rows(np.random.default_rng([DTYPES.index(dtype), d, n, tag]), n, d, dtype)


def gaussian_rows(n, d, offset, dtype):
    """The rows of test_calc_embd_statistics_returns_numpys_own_mean_for_frames_with_an_offset (test_gpu_parity.py), seed and all."""
    rng = np.random.default_rng(n + d)
    return np.maximum(rng.standard_normal((n, d)) * 0.3 + offset, 0).astype(dtype)


# --------------------------------------------------------------------------------- wrong orders (to prove that the rows discriminate)
def grouped(x, g):
    """Groups of g consecutive rows summed from zero, the group sums then added in order (a walk that merges per-group partial sums)."""
    parts = np.stack([running_sum(x[i:i + g]) for i in range(0, x.shape[0], g)])
    return running_sum(parts)


def halves(x):
    """Two halves walked apart and merged."""
    h = x.shape[0] // 2
    with np.errstate(all="ignore"):
        return running_sum(x[:h]) + running_sum(x[h:])


def exact_rounded(x):
    """The exact sum, rounded once (float64 holds it: 36 bits of span + 14 bits of row count)."""
    with np.errstate(all="ignore"):
        return x.astype(np.float64).sum(axis=0).astype(np.float32)


def last_row_twice(x):
    """One row too many."""
    return running_sum(x[-1:], start=running_sum(x))


WRONG_ORDERS = (("grouped 4", lambda x: grouped(x, 4), 0.25), ("grouped 16", lambda x: grouped(x, 16), 0.25), ("halves", halves, 0.25),
                ("exact rounded", exact_rounded, 0.25), ("last row twice", last_row_twice, 0.50))
SHARP_FROM = 33            # row counts below this test row counting and edges, not order: no share is asked of them


def shares(x):
    """-> {wrong order: share of the columns whose float32 MEAN it changes} for float32 rows x."""
    n = x.shape[0]
    want = mean_of(running_sum(x), n)
    return {name: float(np.mean(mean_of(f(x), n) != want)) for name, f, _ in WRONG_ORDERS}


# --------------------------------------------------------------------------------- case tables
# A. one plain update.  (route, dtype, d, n, placement); routes: moments.hip running_sums -- "h16": float16, d % 8 == 0, base and pitch
# 16-byte aligned -> moments_running_colsum_h16 on the side stream; everything else moments_running_colsum<T, WIDE> on the caller's
# stream, WIDE when d % (16 / sizeof T) == 0 and base and pitch are 16-byte aligned.  Host rows are staged to ld = d on an aligned base.
H16_N = (2, 3, 15, 16, 17, 47, 48, 49, 191, 192, 193, 383, 385, 768, 769, 961, 1537, 1729)      # 16-row sets, 192-row tiles, ntiles 1 .. 10
GEN_N = (2, 17, 1023, 1024, 1025, 2048, 2049, 3073)                                              # 1024-row tiles, two LDS buffers


def _plain_cases():
    c = []
    for d in (136, 512):                  # 136: the last workgroup half filled, d % 32 != 0; 512: cdiv(d, 16) % 32 == 0, the XCD remap
        for n in H16_N:
            for pl in ("dev", "pitch8"):
                c.append(("h16", "float16", d, n, pl))
    for d in (16, 24, 1024):
        for n in (193, 961):
            for pl in ("dev", "pitch8"):
                c.append(("h16", "float16", d, n, pl))
    for n in (193, 1025):
        c.append(("h16", "float16", 136, n, "host"))
    generic = (("f16 narrow", "float16", 20, "dev"), ("f16 narrow", "float16", 136, "odd"),
               ("bf16 wide", "bfloat16", 16, "dev"), ("bf16 wide", "bfloat16", 136, "dev"),
               ("bf16 narrow", "bfloat16", 20, "dev"), ("bf16 narrow", "bfloat16", 136, "odd"),
               ("f32 wide", "float32", 12, "dev"), ("f32 wide", "float32", 132, "dev"),
               ("f32 narrow", "float32", 17, "dev"), ("f32 narrow", "float32", 132, "odd"))
    for route, dtype, d, pl in generic:
        for n in GEN_N:
            c.append((route, dtype, d, n, pl))
    c.append(("f32 wide", "float32", 132, 1025, "host"))
    c.append(("f32 wide", "bfloat16", 136, 1025, "host"))      # (a host bfloat16 tensor goes in widened to float32: _capi.rows_view)
    return tuple(c)


PLAIN_CASES = _plain_cases()

# B. carry across updates (float16, d = 136): pieces of one matrix
CARRY_PIECES = (1, 16, 175, 577)                      # cumulative 1, 17, 192, 769
ALTERNATING_PIECES = ((193, "dev"), (383, "odd"), (385, "dev"))      # 961 rows: h16 walk, generic kernel, h16 walk
# ... detached: each walk long enough (9 - 12 cycles a row: 0.3, 0.04 and 0.2 ms) to be still running when the host has enqueued the next
DETACHED_PIECES = ((80000, "dev"), (10001, "odd"), (50000, "dev"))
RESET_FEEDS = (385, 193)

# C. update_multi: 17 handles with rows (fad_moments_update_multi drops the empty one first, then splits what is left into launches of
# 16 + 1) and one without; 3 bfloat16 handles in one launch
MULTI_D = 136
MULTI_N = (193, 2, 3, 15, 16, 17, 0, 47, 48, 49, 191, 192, 383, 385, 768, 769, 961, 1537)
MULTI_BF16_N = (17, 1025, 2049)

# D. update_multi_indexed: the IDX walk (d >= 512 and every list >= 16 d long) and the gather fallback
INDEXED_D, INDEXED_SRC, INDEXED_LENGTHS = 512, 300, (8192, 8257, 8448)
GATHER_D, GATHER_SRC, GATHER_LENGTH = 136, 300, 193


def index_list(length, n_src, tag):
    return np.random.default_rng([length, n_src, tag]).integers(0, n_src, size=length).astype(np.int32)


# E. update_segmented(want_runsums=True).  (route, dtype, d, sizes, placement)
EDGE_SIZES = (0, 1, 3, 4, 5, 31, 32, 33, 36, 67, 300)                 # the 32- / 4- / 1-row and 8- / 1-row loops of segment_running_sums
SEGMENT_CASES = (
    ("job table h16", "float16", 256, (8200, 300, 0, 257, 1, 769), "dev"),
    ("job table h16", "float16", 256, (8200, 300, 0, 257, 1, 769), "host"),
    ("thread per 8 columns", "float16", 136, EDGE_SIZES, "dev"),
    ("thread per 8 columns", "float16", 136, EDGE_SIZES, "host"),
    ("thread per 8 columns", "bfloat16", 136, EDGE_SIZES, "dev"),
    ("thread per column", "float32", 17, EDGE_SIZES, "dev"),
    ("thread per column", "bfloat16", 20, EDGE_SIZES, "dev"),
    ("thread per column", "float16", 136, EDGE_SIZES, "odd"),
    ("tile kernel WALK", "float16", 128, (256, 700, 2250, 257, 8192), "dev"),
    ("tile kernel WALK", "bfloat16", 128, (256, 700, 2250, 257, 8192), "dev"),
)

# F. non-finite entries on the generic routes
NONFINITE_CASES = (("bf16 wide", "bfloat16", 136, 1025, "dev"), ("f32 narrow", "float32", 17, 1025, "dev"), ("f16 narrow", "float16", 136, 1025, "odd"))


def segment_rows(dtype, d, sizes):
    return rows_for(dtype, d, int(sum(sizes)), tag=1)


def order_inputs():
    """Every matrix whose running sum the GPU test holds a walk to, as (label, float32 rows), each once."""
    seen = set()
    for route, dtype, d, n, _ in PLAIN_CASES + NONFINITE_CASES:
        if (dtype, d, n) not in seen:
            seen.add((dtype, d, n))
            yield f"plain {dtype} d={d} n={n}", as_f32(rows_for(dtype, d, n))
    for dtype, ns in (("float16", RESET_FEEDS + tuple(MULTI_N)), ("bfloat16", MULTI_BF16_N)):
        for n in ns:
            if n > 0 and (dtype, MULTI_D, n) not in seen:
                seen.add((dtype, MULTI_D, n))
                yield f"plain {dtype} d={MULTI_D} n={n}", as_f32(rows_for(dtype, MULTI_D, n))
    # the carry cases: the whole matrix and every prefix the GPU test compares
    for pieces in (CARRY_PIECES, tuple(p for p, _ in ALTERNATING_PIECES), (sum(p for p, _ in DETACHED_PIECES),)):
        total = int(sum(pieces))
        x = as_f32(rows_for("float16", MULTI_D, total))
        for at in np.cumsum(pieces):
            yield f"carry float16 d={MULTI_D} total={total} n={at}", x[:at]
    src = as_f32(rows_for("float16", INDEXED_D, INDEXED_SRC))
    for k, length in enumerate(INDEXED_LENGTHS):
        yield f"indexed d={INDEXED_D} length={length}", src[index_list(length, INDEXED_SRC, k)]
    yield f"gathered d={GATHER_D} length={GATHER_LENGTH}", as_f32(rows_for("float16", GATHER_D, GATHER_SRC))[index_list(GATHER_LENGTH, GATHER_SRC, 0)]
    for route, dtype, d, sizes, _ in SEGMENT_CASES:
        if (dtype, d, sizes) in seen:
            continue
        seen.add((dtype, d, sizes))
        x = as_f32(segment_rows(dtype, d, sizes))
        off = np.concatenate([[0], np.cumsum(sizes)])
        for s, n in enumerate(sizes):
            yield f"segment {dtype} d={d} n={n}", x[off[s]:off[s + 1]]
