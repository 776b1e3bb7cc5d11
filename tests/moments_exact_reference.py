"""Integer-valued rows and their exact raw moments: the oracle of tests/test_gpu_moments_exact.py.

For rows whose entries are small integers every quantity the moments kernels form is an integer (or a multiple of one fixed
power of two) that its number format holds exactly: the float16 / bfloat16 products, the float32 MFMA partial sums over one
split of at most 8192 + 64 rows, the float32 column sums of eight rows, the float64 reduce over the splits and the float64
un-shift of the shift guard.  The raw moments a handle exports -- n, sum x, sum x x^T -- then equal the integer result to the last
bit, whatever the order of summation, the split plan, the number of sets in the launch or the kernel variant.

Nothing here needs a GPU.  ``bit_budget`` is the condition that makes the equalities legitimate (tests/test_moments_exact_host.py
keeps it at <= 24 bits for every family the GPU file feeds); ``guard_shifts`` and ``rows_per_split`` mirror what the tile kernels
and ``plan_splits`` (fadtk_amd/csrc/moments.hip) do, so that the budget of a guarded set is taken on the x - c the second pass sums.
"""
import math

import numpy as np

RUN_ROWS = 8192 + 64          # the longest run of rows one workgroup sums in float32 (plan_splits caps a run at 8192; + one stage of slack)


# ------------------------------------------------------------------------------------------ generators
def column_ranges(d, lo, hi):
    """Column j draws from [-a_j, b_j]: a_j walks through 1 .. A with a stride coprime to most A, b_j = a_j - 1, a_j or a_j + 1
    in turn (its own sign pattern: a mean of -1/2, 0 or +1/2 -- far inside mean^2 <= var, so the shift guard stays down).
    A = two thirds of the bound, which leaves room for the neighbour coupling of ``int_rows``."""
    a_max, b_max = (2 * abs(int(lo))) // 3, (2 * int(hi)) // 3
    assert a_max >= 1 and b_max >= 1 and lo < 0 < hi
    j = np.arange(d)
    a = 1 + (7 * j + 3) % a_max
    b = np.clip(a + (j % 3) - 1, 1, b_max)
    return a.astype(np.int64), b.astype(np.int64)


def int_rows(seed, n, d, lo=-31, hi=31):
    """Integer-valued rows [n x d] (float64) inside [lo, hi]: column j uniform on its own range [-a_j, b_j], then
    x_j += u_{j-1} / 2 rounded away from zero -- an asymmetric neighbour coupling in the spirit of ``structured_rows``: every column has its own
    variance, every neighbouring pair its own covariance of the order of n, and a swap of rows between sets, of columns, of
    32-column fragments or of tiles changes the expected integers.  Different seeds give unrelated matrices."""
    rng = np.random.default_rng(seed)
    a, b = column_ranges(d, lo, hi)
    u = rng.integers(0, 1 << 20, size=(n, d), dtype=np.int64) % (a + b + 1) - a
    x = u.copy()
    x[:, 1:] += np.sign(u[:, :-1]) * ((np.abs(u[:, :-1]) + 1) // 2)
    assert n == 0 or (lo <= x.min() and x.max() <= hi)
    return x.astype(np.float64)


def int_rows_torch(seed, n, d, lo=-31, hi=31, device="cpu", dtype=None):
    """The family of ``int_rows`` drawn by torch on ``device`` (a seeded generator of that device; other numbers than numpy's, the
    same ranges, coupling and bounds).  -> tensor [n x d] of ``dtype`` (default float16)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    a, b = column_ranges(d, lo, hi)
    a_t = torch.as_tensor(a, dtype=torch.int32, device=device)
    w_t = torch.as_tensor(a + b + 1, dtype=torch.int32, device=device)
    u = torch.randint(0, 1 << 20, (n, d), generator=g, device=device, dtype=torch.int32) % w_t - a_t
    x = u.clone()
    x[:, 1:] += torch.sign(u[:, :-1]) * torch.div(u[:, :-1].abs() + 1, 2, rounding_mode="floor")
    return x.to(dtype if dtype is not None else torch.float16)


def offset_columns(x, cols, base=48, spread=1, seed=0):
    """A copy of ``x`` whose columns ``cols[:-1]`` are base + integers in [-spread, spread] and whose column ``cols[-1]`` is the
    constant ``base``: |mean| >> std within every split, which raises the shift guard (mean^2 > 64 var: 2304 against 64 x 2/3).
    Works on numpy arrays and torch tensors alike (the offsets are drawn by numpy on the host either way)."""
    cols = list(cols)
    assert len(cols) >= 2
    n = x.shape[0]
    rng = np.random.default_rng(1000003 + seed)
    off = rng.integers(-spread, spread + 1, size=(n, len(cols) - 1)).astype(np.float64) + base
    if isinstance(x, np.ndarray):
        y = x.copy()
        y[:, cols[:-1]] = off
        y[:, cols[-1]] = base
        return y
    import torch
    y = x.clone()
    y[:, cols[:-1]] = torch.as_tensor(off, device=x.device).to(x.dtype)
    y[:, cols[-1]] = base
    return y


# ------------------------------------------------------------------------------------------ reference
def exact_moments(x):
    """-> (n, sum x [d], sum x x^T [d x d]) as float64 holding integers.  A float64 BLAS product of integer values is exact whatever
    its order of summation as long as every sum of absolute products stays below 2^53 (asserted)."""
    x64 = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    assert x64.ndim == 2
    if x64.size:
        assert np.array_equal(x64, np.rint(x64)), "exact_moments wants integer-valued rows"
        assert float(np.abs(x64).max()) ** 2 * max(x64.shape[0], 1) < 2.0 ** 53
    return x64.shape[0], x64.sum(axis=0), x64.T @ x64


def packed(n, s, m):
    """(n, sum x, sum x x^T) in the layout of ``Moments.export()``."""
    return np.concatenate([[float(n)], np.asarray(s, dtype=np.float64).ravel(), np.asarray(m, dtype=np.float64).ravel()])


# ------------------------------------------------------------------------------------------ split plans
def _cdiv(a, b):
    return -(-a // b)


def slab_items(d):
    """Work items per row-split of the 256-column-slab kernel (tile256_roles.h, item_types): P + Q per pair of superblocks, an X
    for every other tile above the diagonal, a Z for the last superblock of an odd count."""
    nsb = _cdiv(d, 256)
    pairs = nsb // 2
    return 2 * pairs + (nsb * (nsb - 1) // 2 - pairs) + (nsb & 1)


def rows_per_split(ns, d, kernel, n_cu=256):
    """``plan_splits`` of fadtk_amd/csrc/moments.hip for one launch over sets of ``ns`` rows: the run of rows every workgroup sums.
    kernel "tile128": 128 x 128 tiles, stages of 32 rows, two workgroups per CU; "slab": stages of 32 rows (64 with a Z item), one
    workgroup per CU.  Both: at least 256 rows, at most 8192."""
    ns = [int(v) for v in ns]
    if kernel == "slab":
        nsb = _cdiv(d, 256)
        items_per_split, kb, wg_per_cu = slab_items(d), (64 if nsb & 1 else 32), 1
    else:
        nt = _cdiv(d, 128)
        items_per_split, kb, wg_per_cu = nt * (nt + 1) // 2, 32, 2
    min_rows, max_rows = 256, 8192
    slots = n_cu * wg_per_cu
    total, longest = sum(ns), max(max(ns), 1)

    def items(r):
        return sum(_cdiv(v, r) for v in ns) * items_per_split

    r_cap = _cdiv(min(max_rows, longest), kb) * kb
    if r_cap > max_rows:
        r_cap = (max_rows // kb) * kb
    r_cap = max(r_cap, kb)
    rounds = _cdiv(items(r_cap), slots)
    r = _cdiv(_cdiv(total * items_per_split, rounds * slots), kb) * kb
    r = max(r, _cdiv(min_rows, kb) * kb)
    while r < r_cap and items(r) > rounds * slots:
        r += kb
    return min(r, r_cap)


# ------------------------------------------------------------------------------------------ shift guard and bit budget
def guard_shifts(x, r):
    """What the first pass of a tile kernel leaves for splits of ``r`` rows (moments_kernels.h, end of tile_h16_tr_body;
    moments_tile256.h likewise): -> (hit [S] bool, c [S x d] float64).  hit: some column of the split has mean^2 > 64 var (the set's
    flag is the OR over its splits); c: float16(mean) where mean^2 > var, 0 elsewhere -- the shifts of the second pass."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    S = max(_cdiv(n, r), 1)
    hit, c = np.zeros(S, dtype=bool), np.zeros((S, d))
    for q in range(S):
        blk = x[q * r:(q + 1) * r]
        nr = float(blk.shape[0])
        if nr == 0:
            continue
        sx, s2 = blk.sum(axis=0), (blk * blk).sum(axis=0)
        mean = sx / nr
        var = s2 / nr - mean * mean
        hit[q] = bool(np.any(~(mean * mean <= 64.0 * var) & ~((sx == 0.0) & (s2 == 0.0))))
        worth = (mean * mean > var) & (np.abs(mean) < 65000.0)
        c[q] = np.where(worth, mean.astype(np.float32).astype(np.float16).astype(np.float64), 0.0)
    return hit, c


def _frac_bits(v):
    """Smallest f with v * 2^f integer for every entry of v (v holds multiples of a power of two; 40 = give up)."""
    for f in range(41):
        s = v * (2.0 ** f)
        if np.array_equal(s, np.rint(s)):
            return f
    return 41


def bit_budget(x, rows_per_run=RUN_ROWS, shifts=None):
    """Significand bits the largest float32 partial sum of products can need.

    The MFMAs add exact products x_i x_j in some order; every intermediate sum is a multiple of the product grid 2^-(f_i + f_j)
    (f_j = fractional bits of column j) and is bounded by sum |x_i x_j| over the run, so it is exact in float32 iff
    log2(sum |x_i x_j|) + f_i + f_j <= 24.  By Cauchy-Schwarz that expression is at most the mean of its two diagonal values
    log2(sum x_i^2) + 2 f_i and log2(sum x_j^2) + 2 f_j, and the diagonal is among the pairs: the maximum over all pairs IS
    max_j [log2(sum x_j^2) + 2 f_j] -- O(n d) instead of O(n d^2).

    shifts = None: the run is ANY window of ``rows_per_run`` consecutive rows (a superset: whole blocks of 32 rows that cover one).
    shifts = (r, c): splits of r rows, evaluated on x - c[split] -- what the second pass of the shift guard sums."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    if n == 0:
        return 0.0
    if shifts is not None:
        r, c = shifts
        y = x.copy()
        for q in range(c.shape[0]):
            y[q * r:(q + 1) * r] -= c[q]
        run2 = np.stack([(y[q * r:(q + 1) * r] ** 2).sum(axis=0) for q in range(c.shape[0])])
    else:
        y = x
        pad = (-n) % 32
        sq = np.concatenate([y * y, np.zeros((pad, d))]).reshape(-1, 32, d).sum(axis=1)
        w = min(_cdiv(rows_per_run, 32) + 1, sq.shape[0])
        cs = np.concatenate([np.zeros((1, d)), np.cumsum(sq, axis=0)])
        run2 = cs[w:] - cs[:-w]
    worst = run2.max(axis=0)
    if np.array_equal(y, np.rint(y)):                 # integers throughout: no fractional bits anywhere
        return math.log2(worst.max()) if worst.max() > 0 else 0.0
    bits = 0.0
    for j in range(d):
        if worst[j] > 0:
            bits = max(bits, math.log2(worst[j]) + 2 * _frac_bits(y[:, j]))
    return bits
