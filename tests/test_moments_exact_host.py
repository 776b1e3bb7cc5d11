"""Host side of the exact moments tests: what makes the equalities of tests/test_gpu_moments_exact.py legitimate.

The GPU file asserts ``np.array_equal`` on raw moments.  That is only fair if every float32 partial sum the tile kernels form is
exact for the rows they are fed: ``bit_budget <= 24`` for every input family of that file, under the split plan of the whole chip
and under that of 8 CUs, with the shift guard's shifts taken as the kernels form them.  This is a condition the families were
chosen to meet, not a measurement of the kernels.  No GPU is needed here.
"""
import math

import numpy as np
import pytest

import moments_exact_reference as X
import test_gpu_moments_exact as G              # the shapes, seeds and generators of the GPU file itself

CUS = (256, 8)                                  # the MI355X's CUs, and FAD_MOMENTS_CUS=8


def _kernel(d, knob="1"):
    return "slab" if (d >= 512 and knob == "1") else "tile128"


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("n,d", [(0, 5), (1, 1), (17, 7), (300, 33), (1029, 64)])
def test_exact_moments_against_int64_einsum(n, d):
    x = X.int_rows(n + d, n, d)
    xi = x.astype(np.int64)
    cnt, s, m = X.exact_moments(x)
    assert cnt == n and s.dtype == np.float64 and m.dtype == np.float64
    assert np.array_equal(s, xi.sum(axis=0))
    assert np.array_equal(m, np.einsum("ki,kj->ij", xi, xi))
    p = X.packed(cnt, s, m)
    assert p.shape == (1 + d + d * d,) and p[0] == n


def test_int_rows_are_structured():
    """Every column its own range, neighbours coupled, other seeds other rows; the torch generator draws the same family."""
    import torch
    x = X.int_rows(3, 100000, 40)
    a, b = X.column_ranges(40, -31, 31)
    assert len({(int(p), int(q)) for p, q in zip(a, b)}) >= 20
    assert x.min() >= -31 and x.max() <= 31 and np.array_equal(x, np.rint(x))
    c = np.cov(x, rowvar=False)
    assert np.all(np.diag(c, 1) > 0.4) and len(set(np.round(np.diag(c, 1)))) >= 10 and np.abs(np.diag(np.corrcoef(x, rowvar=False), 3)).max() < 0.02
    assert not np.array_equal(x, X.int_rows(4, 100000, 40))
    t = X.int_rows_torch(3, 100000, 40).double().numpy()
    assert t.min() >= -31 and t.max() <= 31 and np.array_equal(t, np.rint(t))
    for j in range(40):
        assert t[:, j].min() >= -(a[j] + (a[j - 1] + 1) // 2 if j else a[j]) and t[:, j].max() <= (b[j] + (b[j - 1] + 1) // 2 if j else b[j])
    assert np.all(np.diag(np.cov(t, rowvar=False), 1) > 0.4)


def test_split_plans():
    """``rows_per_split`` is plan_splits: the counts the GPU file's comments quote."""
    assert X.slab_items(512) == 2 and X.slab_items(768) == 5 and X.slab_items(2048) == 32
    assert X.rows_per_split([70001], 8, "tile128", 256) == 256              # 274 splits: the two-level reduce
    assert X.rows_per_split([200003], 128, "tile128", 256) == 416           # 481 splits
    assert X.rows_per_split([70001], 8, "tile128", 8) == 4384               # 16 splits
    assert X.rows_per_split([200003], 128, "tile128", 8) == 6272            # 32 splits
    assert X.rows_per_split([16 * 768 + 33], 768, "slab", 8) == 4160
    for d in (8, 128, 504, 520, 2048):
        for n_cu in CUS:
            for n in (16 * d, 16 * d + 257, 200003):
                for k in ("tile128", "slab") if d >= 512 else ("tile128",):
                    r = X.rows_per_split([n], d, k, n_cu)
                    assert min(256, -(-n // 32) * 32) <= r <= 8192 and r % 32 == 0


# ------------------------------------------------------------------------------------------ bit budgets: plain families
def test_budget_worst_case_of_the_bounds():
    """My own count: entries in [-31, 31] give at most 961 x (8192 + 64 + the 32 rows of slack of the window) < 2^23 per partial sum;
    the guard sets' plain columns in [-8, 8] against a shifted column (|x - c| <= 1.3 on the 2^-5 grid): 8 x 1.3 x 8288 x 2^5 < 2^22."""
    worst = np.full((3 * X.RUN_ROWS, 4), 31.0)
    worst[::2, 1] = -31.0
    b = X.bit_budget(worst)
    assert b == pytest.approx(math.log2(961 * (X.RUN_ROWS + 32)))
    assert b < 23
    assert 8 * 1.3 * (X.RUN_ROWS + 32) * 32 < 2 ** 22


def _assert_plain(x, ns, d, kernel, what):
    """Budget of plain rows under both plans.  The shift guard stays down -- except where the last split is a single row (n = 16 D + 1
    in runs of 256 rows: no variance, the flag goes up and the whole set takes the second pass).  Then every shift must leave
    x - c an error-free float16 difference (the single row: c = x, x - c = 0; every other split: c = 0, mean^2 <= var) -- a
    fractional c would bring TwoSum's e into play, whose e e term the second pass drops -- and the budget is taken on x - c."""
    assert X.bit_budget(x) <= 24, what
    for n_cu in CUS:
        r = X.rows_per_split(ns, d, kernel, n_cu)
        hit, c = X.guard_shifts(x, r)
        if not hit.any():
            continue
        assert x.shape[0] % r == 1 and not hit[:-1].any() and not c[:-1].any(), f"{what}: the guard would fire at {r} rows per split"
        assert np.array_equal(c[-1], x[-1])
        assert X.bit_budget(x, shifts=(r, c)) <= 24, what


@pytest.mark.parametrize("d", (8, 120, 128, 136, 256, 384, 504, 512, 520))
def test_budget_tile128_family(d):
    x = X.int_rows(1000 + d, 16 * d + 257, d)           # the rows of _tile128_case
    for r in G.B_TAILS:
        n = 16 * d + r
        _assert_plain(x[:n], [n], d, "tile128", f"d={d} n={n}")
    _assert_plain(x[100:], [x.shape[0] - 100], d, "tile128", f"d={d} rows [100:]")


def test_budget_float64_kernel_family():
    """The float64 kernel sums float64 products: 53 bits against 961 n."""
    for d in G.A_DIMS:
        x = X.int_rows(100 + d, 16 * d - 1, d)
        assert X.bit_budget(x, rows_per_run=x.shape[0]) <= 24 < 53


@pytest.mark.parametrize("d,n,seed", [(8, 70001, 4008), (128, 200003, 4128), (128, 200003, 95)])
def test_budget_long_sets(d, n, seed):
    """The two-level reduce's rows and the host rows in pieces."""
    x = X.int_rows(seed, n, d)
    _assert_plain(x, [n], d, "tile128", f"d={d} n={n}")
    if seed == 95:                                      # update_any's pieces are updates of their own: 98 304 rows, then 101 699
        _assert_plain(x[:98304], [98304], d, "tile128", "first piece")
        _assert_plain(x[98304:], [n - 98304], d, "tile128", "second piece")


@pytest.mark.parametrize("d", (256, 512))
def test_budget_additivity_pieces(d):
    """The two updates of the additivity case, k on a seam and off one (a last split of 13 rows must not raise the flag)."""
    x = X.int_rows(97 + d, 32 * d + 50, d)
    for k in (16 * d, 16 * d + 13):
        _assert_plain(x[:k], [k], d, _kernel(d), f"d={d} rows [:{k}]")
        _assert_plain(x[k:], [x.shape[0] - k], d, _kernel(d), f"d={d} rows [{k}:]")


@pytest.mark.parametrize("d", (512, 520, 768))
def test_budget_slab_family(d):
    """The slab kernel's rows are drawn by torch on the device; the same generator on the host draws other numbers of the same
    family.  (|x| <= 31 -- asserted on the device rows as well -- carries the budget whatever the numbers.)"""
    n = 16 * d + 63
    x = X.int_rows_torch(d, n, d).double().numpy()
    for r in G.C_TAILS:
        _assert_plain(x[:16 * d + r], [16 * d + r], d, "slab", f"d={d} n=16d+{r}")
    lens = [8192 + 37 * i for i in range(32)]
    if d == 512:
        for n_cu in CUS:
            r = X.rows_per_split(lens, 512, "slab", n_cu)
            for i in (0, 31):
                xi = X.int_rows_torch(5000 + i, lens[i], 512).double().numpy()
                assert not X.guard_shifts(xi, r)[0].any() and X.bit_budget(xi) <= 24


def test_budget_indexed_and_segmented_rows():
    for d in (128, 512, 768):
        n_src = 8 * d + 64
        x = X.int_rows(80 + d, n_src, d)
        idx = G._index_lists(n_src, (16 * d + 1, 16 * d + 37, 2 * n_src + 5), 81 + d)
        ns = [i.size for i in idx]
        for i in idx:
            assert i.min() == 0 and i.max() == n_src - 1 and np.unique(i).size < i.size
            _assert_plain(x[i], ns, d, _kernel(d), f"indexed d={d}")
    assert 8193 * 31 < 2 ** 24                            # a file's float32 running column sums


@pytest.mark.parametrize("d", (128, 136))
def test_budget_tile128_sixteen_sets(d):
    """The sixteen sets of one launch of the 128 x 128 kernel.  The launch has sets shorter than 16 D, so a raised flag leads to the
    float64 redo, never to the second pass: the first-pass budget is all that is asked -- and the sets of at least 256 rows must
    not raise the flag under the launch's own plans (the shorter ones may: few rows, little variance)."""
    lens = [16 * d + 37, 0, 1, 5, 16 * d, 333, 32, 33, 255, 256, 257, 2, 16 * d + 1, 31, 1000, 64]
    live = [n for n in lens if n > 0]
    for i, n in enumerate(lens):
        x = X.int_rows(2000 + 16 * d + i, n, d)
        assert X.bit_budget(x) <= 24
        for n_cu in CUS:
            r = X.rows_per_split(live, d, "tile128", n_cu)
            hit, _ = X.guard_shifts(x, r)
            assert not hit[:n // r].any(), f"set {i}: a whole split of {r} rows would raise the flag"
    assert X.bit_budget(X.int_rows(7003, 300, d)) <= 24
    for dd in (64, 65):                                   # the sixteen sets of the float64 kernel: float64 sums, 53 bits
        for i, n in enumerate([0, 1, 2, 16 * dd - 1, 33, 15, 16, 17, 63, 64, 65, 5, 100, 257, 7, 300]):
            assert X.bit_budget(X.int_rows(500 + 16 * dd + i, n, dd), rows_per_run=max(n, 32)) <= 24


def test_budget_accumulate_reset_overwrite_rows():
    """n = 4097, 4104, 4111 at D = 256: the first has a last split of one row under the 256-row plan (see _assert_plain)."""
    for i in range(3):
        n = 16 * 256 + 7 * i + 1
        _assert_plain(X.int_rows(3000 + i, n, 256), [n], 256, "tile128", f"accumulate rows {i}")
    _assert_plain(X.int_rows(77, 16 * 256 + 33, 256), [16 * 256 + 33], 256, "tile128", "FORCE_GENERIC rows")


@pytest.mark.parametrize("d", (640, 1280, 1792, 2048))
def test_budget_slab_family_wide(d):
    """The wider slab shapes (5, 7 and 8 superblocks, and the ragged 640), 256 columns at a time (budget and guard are per column;
    the neighbour coupling is drawn on the whole matrix first), at the tails that differ in kind: one row over and the longest."""
    n = 16 * d + 63
    xt = X.int_rows_torch(d, n, d)
    for j0 in range(0, d, 256):
        x = xt[:, j0:j0 + 256].double().numpy()
        for r in (1, 63):
            _assert_plain(x[:16 * d + r], [16 * d + r], d, "slab", f"d={d} n=16d+{r} columns {j0}..")


@pytest.mark.parametrize("d", (520, 768))
def test_budget_slab_two_updates(d):
    for seed, n in ((9000 + d, 16 * d + 33), (9100 + d, 16 * d + 1)):
        _assert_plain(X.int_rows_torch(seed, n, d).double().numpy(), [n], d, "slab", f"two updates d={d} n={n}")


@pytest.mark.parametrize("d", (128, 768))
def test_budget_segmented_rows(d):
    """File-aligned splits have no second pass (a raised flag leads to the float64 redo): the first-pass budget over any run of at
    most 8192 + 64 rows is what is asked, with the guard on or off."""
    x = X.int_rows(90 + d, int(sum(G.SEG_LENS)), d)
    assert X.bit_budget(x) <= 24


# ------------------------------------------------------------------------------------------ bit budgets: guard families
def _assert_guard(x, ns, d, kernel, cols, what, flagged=True):
    """Rows of ``_guard_rows`` under both plans: the flag goes up, the plain columns get no shift (c = 0: mean^2 <= var), the shifted
    columns sit within 1.3 of a c on the 2^-5 grid, x - c is an error-free float16 difference (TwoSum's e = 0), and both what the
    second pass sums and -- FAD_MOMENTS_SHIFT_GUARD=0 -- what the first pass sums fit 24 bits."""
    budgets = []
    for n_cu in CUS:
        r = X.rows_per_split(ns, d, kernel, n_cu)
        hit, c = X.guard_shifts(x, r)
        assert hit.any() == flagged, what
        plain = np.setdiff1d(np.arange(d), cols)
        rows = np.minimum(r, x.shape[0] - r * np.arange(c.shape[0]))
        assert not c[rows > 1][:, plain].any(), f"{what}: a plain column would be shifted at {r} rows per split"
        assert all(np.array_equal(c[q], x[q * r]) for q in np.flatnonzero(rows == 1))      # (a split of one row: c = the row, x - c = 0)
        if flagged:
            assert np.all(c[:, cols] >= 47) and np.all(c[:, cols] <= 49) and np.array_equal(c * 32, np.rint(c * 32))
            for q in range(c.shape[0]):
                y = x[q * r:(q + 1) * r] - c[q]
                assert np.array_equal(y, y.astype(np.float16).astype(np.float64)) and np.abs(y[:, cols]).max() <= 1.3
            budgets.append(X.bit_budget(x, shifts=(r, c)))
            assert budgets[-1] <= 24, f"{what}: second pass needs {budgets[-1]:.2f} bits at {r} rows per split"
        off = X.bit_budget(x, rows_per_run=r)
        assert off <= 24, f"{what}: guard off, {off:.2f} bits at {r} rows per split"
    return budgets


@pytest.mark.parametrize("d,knob,variant,cols", G.GUARD_CASES)
def test_budget_guard_second_pass(d, knob, variant, cols):
    n = 16 * d + 33
    x = G._guard_rows(60 + d, n, d, cols)
    b = _assert_guard(x, [n], d, _kernel(d, knob), list(cols), f"d={d} cols={cols}")
    assert max(b) > 12                                    # (a fractional grid is in play: these are not integer sums)


def test_budget_guard_other_launches():
    x = G._guard_rows(61, 70001, 8, (1, 2, 5))
    _assert_guard(x, [70001], 8, "tile128", [1, 2, 5], "two-level un-shift")
    x = G._guard_rows(62, 16 * 256 + 33, 256, (126, 127, 128, 129, 131))
    assert X.bit_budget(x) <= 24                          # bfloat16: first pass and float64 redo only
    for d in (256, 768):
        ns = [16 * d + 32, 16 * d + 33, 16 * d + 63]
        cols = list(G._middle_cols(d))
        _assert_guard(G._guard_rows(66 + d, ns[1], d, cols), ns, d, _kernel(d), cols, f"middle set d={d}")
        for seed, n in ((65 + d, ns[0]), (67 + d, ns[2])):
            _assert_guard(X.int_rows(seed, n, d, -8, 8), ns, d, _kernel(d), [], f"outer sets d={d}", flagged=False)
    x = G._guard_rows(63, 16 * 256 + 33, 256, (2, 127, 128, 250, 255))
    assert X.bit_budget(x) <= 24                          # launch with a short set: float64 redo


def test_unshift_is_exact_in_float64():
    """The un-shift of reduce_body / moments_presum / moments_reduce256 per split: s += c_a s'_b + s'_a c_b + n_q c_a c_b and
    sum x = s' + n_q c.  c = k / 32 with k < 2^11, s' a multiple of 2^-5 below 1.3 x 8256 (19 bits), n_q <= 8256 (14 bits): the
    products are multiples of 2^-10 below 2^25 and need at most 36 bits, their sums over fewer than 2^10 splits stay below 2^53 of
    that grid -- every step is exact, fused or not.  Checked here with the kernel's own expression against rational arithmetic."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    for _ in range(200):
        ca, cb = (float(np.float16(48 + rng.uniform(-0.3, 0.3))) for _ in range(2))
        sa, sb = (float(rng.integers(-343000, 343000)) / 32 for _ in range(2))
        nq = float(rng.integers(256, 8257))
        got = ca * sb + sa * cb + nq * ca * cb
        want = Fraction(ca) * Fraction(sb) + Fraction(sa) * Fraction(cb) + Fraction(nq) * Fraction(ca) * Fraction(cb)
        assert Fraction(got) == want


# ------------------------------------------------------------------------------------------ what equality buys
def test_what_the_tolerance_admits_and_equality_does_not():
    """The existing moments tests hold sum x x^T of Gaussian rows to atol = 1e-6 max|M|.  At n = 16 x 2048 + 3000, D = 2048,
    standard-normal float16 rows (the largest slab fuzz shape; 256 of its columns here) max|M| is the largest diagonal entry (Cauchy-Schwarz), about n, and
    the bound admits an absolute error of 0.037 in EVERY entry: 2e-4 of a typical off-diagonal entry (sqrt(n) = 189).

    Measured here, because it decides what the exact tests add:
      * a dropped row changes M by x_k x_k^T, up to ~10 in magnitude: OUTSIDE the bound in most entries at this shape -- rows of unit
        variance lost whole are noticed by the tolerance tests as well (the bound only swallows one once 1e-6 n reaches x^2, n ~ 1e7);
      * adding 1 to a single entry changes one row and column of M by x_kj, up to ~4: outside the bound too;
      * but every fault below 0.037 per entry passes: one entry of one row off by an ulp of float16 (a wrong low bit in a fragment),
        one float32 partial sum of a split rounded away (8192 x 2^-24 x |sum|), a row lost from the columns where it is small.
    On integer rows each of these changes an integer and fails the equality."""
    n, d = 16 * 2048 + 3000, 256                          # (the bound follows n, not D: 256 of the 2048 columns show the same)
    rng = np.random.default_rng(2048)
    x = rng.standard_normal((n, d), dtype=np.float32).astype(np.float16).astype(np.float64)
    tol = 1e-6 * (x * x).sum(axis=0).max()               # = 1e-6 max|M|
    assert 0.03 < tol < 0.045 and tol / math.sqrt(n) > 1e-4
    run = (x[:8192] * x[:8192]).sum(axis=0).max()         # the largest float32 partial sum of one split of 8192 rows
    assert float(np.spacing(np.float32(run))) < 0.05 * tol                             # NOT noticed: its last bit rounded away
    k, j = n - 1, 5
    drop = np.outer(x[k], x[k])
    assert np.abs(drop).max() > 100 * tol and (np.abs(drop) > tol).mean() > 0.5        # noticed by the tolerance
    bump = np.abs(x[k]).copy(); bump[j] = abs(2 * x[k, j] + 1)
    assert bump.max() > 50 * tol
    ulp = float(np.spacing(np.float16(abs(x[k, j]))))
    low_bit = ulp * np.abs(x[k]); low_bit[j] = abs(2 * x[k, j] * ulp + ulp * ulp)
    assert low_bit.max() < 0.2 * tol                                                  # NOT noticed: inside the bound everywhere
    small = np.abs(x[k]) < 0.15
    assert small.sum() > 20 and np.abs(drop[np.ix_(small, small)]).max() < tol        # nor a row lost where it is small
    # the same changes on integer rows: every one of them changes integers
    xi = X.int_rows(7, 600, 24)
    _, s, m = X.exact_moments(xi)
    for y in (xi[:-1], np.vstack([xi, xi[-1:]])):                                     # a lost row, a doubled row
        _, s2, m2 = X.exact_moments(y)
        assert not np.array_equal(m2, m) and not np.array_equal(s2, s)
    y = xi.copy(); y[-1, j] += 1
    _, s2, m2 = X.exact_moments(y)
    assert not np.array_equal(m2, m) and (m2 != m).sum() >= 2 * np.count_nonzero(xi[-1]) - 1
    y = xi.copy(); y[-1] = 0                                                          # a range check that zeroes a split's last row
    assert not np.array_equal(X.exact_moments(y)[2], m)


def test_the_gpu_files_comparison_notices_one_wrong_number():
    """``check`` of the GPU file: one entry of sum x x^T off by one, one column sum, the count, a lost mirror image."""
    x = X.int_rows(11, 300, 24)
    ref = X.exact_moments(x)
    good = X.packed(*ref)
    G.check(good, ref, "unchanged")
    d = 24
    for pos in (0, 1 + 7, 1 + d + 5 * d + 9):
        bad = good.copy(); bad[pos] += 1.0
        with pytest.raises(AssertionError):
            G.check(bad, ref, "one number off by one")
    y = x.copy(); y[:, [3, 4]] = y[:, [4, 3]]                                          # two columns swapped
    with pytest.raises(AssertionError):
        G.check(X.packed(*X.exact_moments(y)), ref, "columns swapped")
    lost = X.exact_moments(x[:-1])
    with pytest.raises(AssertionError):
        G.check(X.packed(x.shape[0], lost[1], lost[2]), ref, "a row lost, the count right")
