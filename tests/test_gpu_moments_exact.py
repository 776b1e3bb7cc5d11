"""The moments kernels to the last bit, on integer-valued rows.

Rows of small integers make every quantity the kernels form exact in its format (tests/moments_exact_reference.py,
tests/test_moments_exact_host.py keeps the bit budgets), so what ``Moments.export()`` returns -- n, every column sum, every one of the
D^2 entries of sum x x^T -- must EQUAL the integer result: on the float64 kernel, the 128 x 128 tile kernel, the 256-column-slab
kernel, the one- and two-level reduce, the shift guard's second pass and its float64 redo, gathered rows, file-aligned splits and
host rows in pieces.  One wrong element in one tile of one set, a lost or doubled row, a stage read twice at a split seam: each
changes an integer.  Every case runs under the split plan of the whole chip and under that of 8 CUs (FAD_MOMENTS_CUS): exact sums
do not depend on the plan.

Everything goes through fadtk_amd.hip.Moments.  The variant (``last_timing()[2]``: 0 = 128 x 128 tiles, 1 = float64 kernel,
2 = slab kernel) is asserted where the case names it; the split count, the reduce's levels and whether the guard fired cannot be
observed from outside -- the comments say how they follow from ``plan_splits``.
"""
import numpy as np
import pytest

import moments_exact_reference as X

pytestmark = pytest.mark.gpu

PLANS = (None, "8")          # FAD_MOMENTS_CUS: unset (the chip's CUs) and 8
U = 2.0 ** -53               # unit roundoff of float64


@pytest.fixture(scope="module")
def T():
    import torch
    from fadtk_amd import _capi
    _capi.require_gpu(0)
    return torch


def _torch_dtype(T, name):
    return {"fp16": T.float16, "bf16": T.bfloat16, "fp32": T.float32, "fp64": T.float64}[name]


def dev(T, x, dtype="fp16", pitch=None, skew=0):
    """numpy rows -> device tensor view [n x d] with a row pitch of ``pitch`` elements (NaN in the padding) whose base sits ``skew``
    elements behind an allocation boundary."""
    n, d = x.shape
    dt = _torch_dtype(T, dtype)
    pitch = pitch or d
    buf = T.full((n * pitch + skew,), float("nan"), dtype=dt, device="cuda")
    v = buf[skew:].view(n, pitch)[:, :d]
    v.copy_(T.from_numpy(np.ascontiguousarray(x)).to("cuda"))
    return v


def pitched(T, xt, pitch):
    """A device tensor's rows on a wider pitch, NaN in the padding."""
    n, d = xt.shape
    buf = T.full((n, pitch), float("nan"), dtype=xt.dtype, device="cuda")
    buf[:, :d] = xt
    return buf[:, :d]


def check(p, ref, what):
    """All of export() against (n, sum x, sum x x^T): equality, and M == M^T."""
    n, s, m = ref
    d = s.shape[0]
    assert p.shape == (1 + d + d * d,), what
    assert p[0] == float(n), f"{what}: n = {p[0]}, want {n}"
    bad = np.flatnonzero(p[1:1 + d] != s)
    assert bad.size == 0, f"{what}: {bad.size} column sums differ, first at column {bad[:1]}: {p[1 + bad[:1]]} != {s[bad[:1]]}"
    mg = p[1 + d:].reshape(d, d)
    if not np.array_equal(mg, m):
        ij = np.argwhere(mg != m)
        raise AssertionError(f"{what}: {ij.shape[0]} of {d * d} entries of sum x x^T differ, first at {tuple(ij[0])}: "
                             f"{mg[tuple(ij[0])]!r} != {m[tuple(ij[0])]!r}; rows touched {np.unique(ij[:, 0])[:8]}")
    assert np.array_equal(mg, mg.T), f"{what}: sum x x^T is not symmetric"


def add(a, b):
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


def on_plans(monkeypatch, run):
    """run() -> list of exports, once per split plan; the plans must agree bit for bit.  -> the first plan's list."""
    outs = []
    for cus in PLANS:
        if cus is None:
            monkeypatch.delenv("FAD_MOMENTS_CUS", raising=False)
        else:
            monkeypatch.setenv("FAD_MOMENTS_CUS", cus)
        outs.append(run())
    monkeypatch.delenv("FAD_MOMENTS_CUS", raising=False)
    for o in outs[1:]:
        assert len(o) == len(outs[0])
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b), "the split plans of the whole chip and of 8 CUs disagree"
    return outs[0]


def one_update(rows, d, want_variant=None):
    from fadtk_amd.hip import Moments
    with Moments(d) as m:
        m.set_timing(True)
        m.update(rows)
        if want_variant is not None and rows.shape[0] > 0:
            assert m.last_timing()[2] == want_variant
        return m.export()


# ========================================================================================= A. float64 kernel (variant 1)
A_DIMS = (1, 7, 64, 65, 131, 200)


def _a_lengths(d):
    return sorted({1, 2, 15, 16, 17, 63, 64, 65, 16 * d - 1})


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32", "fp64"])
@pytest.mark.parametrize("d", A_DIMS)
def test_float64_kernel_exact(T, monkeypatch, d, dtype):
    """Fewer than 16 rows per column (or D % 8 != 0, or another dtype than the 16-bit ones): moments_tile_f64, device rows."""
    x = X.int_rows(100 + d, max(_a_lengths(d)), d)         # (D = 1: 65 rows -- 16 rows per column and more still take this kernel there)
    xt = dev(T, x, dtype)
    for n in _a_lengths(d):
        assert xt[:n].shape[0] == n == x[:n].shape[0]
        got = on_plans(monkeypatch, lambda: [one_update(xt[:n], d, 1)])
        check(got[0], X.exact_moments(x[:n]), f"d={d} n={n} {dtype}")


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32", "fp64"])
@pytest.mark.parametrize("d", (7, 64, 131))
def test_float64_kernel_pitch_and_misaligned_base(T, monkeypatch, d, dtype):
    """A pitch of D + 3 elements, NaN in the padding, and a base one element (2 bytes for the 16-bit types) off its allocation."""
    for n in (17, 16 * d - 1):
        x = X.int_rows(200 + d + n, n, d)
        xt = dev(T, x, dtype, pitch=d + 3, skew=1)
        assert xt.data_ptr() % 16 != 0 and xt.stride(0) == d + 3
        got = on_plans(monkeypatch, lambda: [one_update(xt, d, 1)])
        check(got[0], X.exact_moments(x), f"d={d} n={n} {dtype} pitch d+3")


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
@pytest.mark.parametrize("d", (1, 65, 200))
def test_float64_kernel_host_rows(T, monkeypatch, d, dtype):
    """Host rows (numpy), staged by the library; a non-contiguous host view keeps its pitch."""
    wide = X.int_rows(300 + d, max(17, 16 * d - 1), d + 3).astype(dtype)
    for n in (1, 17, 16 * d - 1):
        for rows in (np.ascontiguousarray(wide[:n, :d]), wide[:n, :d]):
            assert rows.shape == (n, d)
            got = on_plans(monkeypatch, lambda: [one_update(rows, d, 1)])
            check(got[0], X.exact_moments(wide[:n, :d]), f"d={d} n={n} host {np.dtype(dtype).name}")


def test_float64_kernel_host_bfloat16(T, monkeypatch):
    d, n = 65, 200
    x = X.int_rows(41, n, d)
    rows = T.from_numpy(x).to(T.bfloat16)          # host bfloat16: widened by the binding
    got = on_plans(monkeypatch, lambda: [one_update(rows, d, 1)])
    check(got[0], X.exact_moments(x), "host bfloat16")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("d", (64, 65))
def test_float64_kernel_sixteen_sets(T, monkeypatch, d, dtype):
    """One update_multi of 16 sets, none of 16 D rows: one launch of the float64 kernel.  Handles 0 (which gets no rows) and 3 hold
    earlier rows: the launch must add to them."""
    from fadtk_amd.hip import Moments
    lens = [0, 1, 2, 16 * d - 1, 33, 15, 16, 17, 63, 64, 65, 5, 100, 257, 7, 300]
    xs = [X.int_rows(500 + 16 * d + i, n, d) for i, n in enumerate(lens)]
    before = {0: X.int_rows(7001, 40, d), 3: X.int_rows(7002, 19, d)}
    blocks = [dev(T, x, dtype) for x in xs]
    pre = {k: dev(T, v, dtype) for k, v in before.items()}

    def run():
        accs = [Moments(d) for _ in lens]
        for k, v in pre.items():
            accs[k].update(v)
        accs[1].set_timing(True)                   # (the first handle that gets rows owns the launch's events)
        Moments.update_multi(accs, blocks)
        assert accs[1].last_timing()[2] == 1
        out = [a.export() for a in accs]
        for a in accs:
            a.close()
        return out
    got = on_plans(monkeypatch, run)
    for i, x in enumerate(xs):
        ref = X.exact_moments(x)
        if i in before:
            ref = add(ref, X.exact_moments(before[i]))
        check(got[i], ref, f"set {i} of 16, d={d} {dtype}")


def test_force_generic_exact(T, monkeypatch):
    d, n = 256, 16 * 256 + 33
    x = X.int_rows(77, n, d)
    xt = dev(T, x, "fp16")
    monkeypatch.setenv("FAD_MOMENTS_FORCE_GENERIC", "1")
    got = on_plans(monkeypatch, lambda: [one_update(xt, d, 1)])
    check(got[0], X.exact_moments(x), "FAD_MOMENTS_FORCE_GENERIC=1")


# ========================================================================================= B. 128 x 128 tile kernel (variant 0)
B_TAILS = (0, 1, 31, 32, 33, 255, 257)


def _tile128_case(T, monkeypatch, d):
    x = X.int_rows(1000 + d, 16 * d + 257, d)
    n0 = 16 * d
    base = X.exact_moments(x[:n0])
    for dtype in ("fp16", "bf16"):
        xt = dev(T, x, dtype)
        for r in B_TAILS:
            n = n0 + r
            got = on_plans(monkeypatch, lambda: [one_update(xt[:n], d, 0)])
            check(got[0], add(base, X.exact_moments(x[n0:n])), f"d={d} n=16d+{r} {dtype}")
        n = n0 + 33
        ref = add(base, X.exact_moments(x[n0:n]))
        for pitch in (d + 8, d + 264):             # NaN behind every row: a load past column d - 1 poisons the sums
            xp = pitched(T, xt[:n], pitch)
            got = on_plans(monkeypatch, lambda: [one_update(xp, d, 0)])
            check(got[0], ref, f"d={d} pitch {pitch} {dtype}")
        sl = xt[100:]                               # a row-sliced view: the base moves by 100 rows
        got = on_plans(monkeypatch, lambda: [one_update(sl, d, 0)])
        check(got[0], X.exact_moments(x[100:]), f"d={d} rows [100:] {dtype}")


@pytest.mark.parametrize("d", (8, 120, 128, 136, 256, 384, 504))
def test_tile128_exact(T, monkeypatch, d):
    """n = 16 D + r: whole stages of 32 rows, one row over, one short; D below, at and above the tile edge, ragged last tiles.
    (r = 1 and 257 in runs of 256 rows leave a last split of ONE row: no variance, so the shift flag goes up and the set takes the
    second pass with c = that row -- exact as well, see _assert_plain of the host file.)"""
    _tile128_case(T, monkeypatch, d)


@pytest.mark.parametrize("d", (512, 520))
def test_tile128_exact_above_512(T, monkeypatch, d):
    """FAD_MOMENTS_TILE256=0 keeps D >= 512 on the 128 x 128 kernel: four and five tiles a side."""
    monkeypatch.setenv("FAD_MOMENTS_TILE256", "0")
    _tile128_case(T, monkeypatch, d)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("d", (128, 136))
def test_tile128_sixteen_sets(T, monkeypatch, d, dtype):
    """One long set sends the whole launch to the tile kernel: the sets of 0, 1, 5 and 333 rows go through it as well (a set of one
    row raises its shift flag -- its variance is zero -- and, the launch having short sets, is redone by the float64 kernel)."""
    from fadtk_amd.hip import Moments
    lens = [16 * d + 37, 0, 1, 5, 16 * d, 333, 32, 33, 255, 256, 257, 2, 16 * d + 1, 31, 1000, 64]
    xs = [X.int_rows(2000 + 16 * d + i, n, d) for i, n in enumerate(lens)]
    before = X.int_rows(7003, 300, d)
    blocks = [dev(T, x, dtype) for x in xs]
    pre = dev(T, before, dtype)

    def run():
        accs = [Moments(d) for _ in lens]
        accs[4].update(pre)
        accs[0].set_timing(True)
        Moments.update_multi(accs, blocks)
        assert accs[0].last_timing()[2] == 0
        out = [a.export() for a in accs]
        for a in accs:
            a.close()
        return out
    got = on_plans(monkeypatch, run)
    for i, x in enumerate(xs):
        ref = X.exact_moments(x)
        if i == 4:
            ref = add(ref, X.exact_moments(before))
        check(got[i], ref, f"set {i} of 16, d={d} {dtype}")


def test_tile128_accumulate_reset_overwrite(T, monkeypatch):
    from fadtk_amd.hip import Moments
    d = 256
    xs = [X.int_rows(3000 + i, 16 * d + 7 * i + 1, d) for i in range(3)]
    ts = [dev(T, x, "fp16") for x in xs]

    def run():
        with Moments(d) as m:
            m.update(ts[0]); m.update(ts[1])
            two = m.export()
            m.reset()
            m.update(ts[2])                        # the reduce behind a reset stores instead of adding
            return [two, m.export()]
    got = on_plans(monkeypatch, run)
    check(got[0], add(X.exact_moments(xs[0]), X.exact_moments(xs[1])), "two updates")
    check(got[1], X.exact_moments(xs[2]), "update behind reset")


@pytest.mark.parametrize("d,n,dtype", [(8, 70001, "fp16"), (8, 70001, "bf16"), (128, 200003, "fp16")])
def test_tile128_two_level_reduce(T, monkeypatch, d, n, dtype):
    """More than 128 splits: moments_presum, then moments_reduce<double>.  plan_splits on 256 CUs (512 workgroup slots, one tile):
    the run that fills one round is ceil(n / 512) rows, below the minimum of 256 at D = 8 -> 256-row runs, ceil(70001 / 256) = 274
    splits; at D = 128 ceil(200003 / 512) = 391 -> 416 rows (a multiple of the 32-row stage), ceil(200003 / 416) = 481 splits.
    On the 8-CU plan the same rows make 16 and 32 splits and take the one-level reduce: both must give the same integers."""
    assert -(-n // X.rows_per_split([n], d, "tile128", 256)) > 128 >= -(-n // X.rows_per_split([n], d, "tile128", 8))
    x = X.int_rows(4000 + d, n, d)
    xt = dev(T, x, dtype)
    got = on_plans(monkeypatch, lambda: [one_update(xt, d, 0)])
    check(got[0], X.exact_moments(x), f"two-level reduce d={d} {dtype}")


# ========================================================================================= C. slab kernel (variant 2)
C_TAILS = (0, 1, 33, 63)


def _device_moments(T, xt, crosscheck):
    """(n, sum x, sum x x^T) of a device tensor with torch.float64 ON the device -- exact for these magnitudes like any float64
    product -- with a block of 64 columns (and the column sums) cross-checked against numpy on the host."""
    x64 = xt.double()
    m, s = (x64.T @ x64).cpu().numpy(), x64.sum(dim=0).cpu().numpy()
    if crosscheck:
        xh = xt.cpu().numpy().astype(np.float64)
        j0 = xt.shape[1] // 2 - 17
        assert np.array_equal(m[:, j0:j0 + 64], xh.T @ xh[:, j0:j0 + 64])
        assert np.array_equal(s, xh.sum(axis=0))
    return xt.shape[0], s, m


@pytest.mark.parametrize("d", (512, 520, 640, 768, 1280, 1536, 1792, 2040, 2048))
def test_slab_exact(T, monkeypatch, d):
    """2 .. 8 superblocks: P/Q pairs, a ragged last superblock (520, 640, 2040), a Z item at 3, 5 and 7 superblocks (768, 1280,
    1792).  The rows are drawn on the device; the reference of the first 16 D rows is numpy's below D = 1536 and torch.float64's
    on the device above (cross-checked on 64 columns), the tails are added on the host."""
    n0 = 16 * d
    xt = X.int_rows_torch(d, n0 + 63, d, device="cuda")
    assert float(xt.abs().max()) <= 31
    tail = xt[n0:].cpu().numpy().astype(np.float64)
    if d >= 1536:
        base = _device_moments(T, xt[:n0], crosscheck=True)
    else:
        base = X.exact_moments(xt[:n0].cpu().numpy())
    for r in C_TAILS:
        n = n0 + r
        got = on_plans(monkeypatch, lambda: [one_update(xt[:n], d, 2)])
        check(got[0], add(base, X.exact_moments(tail[:r])), f"d={d} n=16d+{r}")
    n = n0 + 33
    ref = add(base, X.exact_moments(tail[:33]))
    for pitch in (d + 8, d + 264):
        xp = pitched(T, xt[:n], pitch)
        got = on_plans(monkeypatch, lambda: [one_update(xp, d, 2)])
        check(got[0], ref, f"d={d} pitch {pitch}")


@pytest.mark.parametrize("d", (520, 768))
def test_slab_two_updates_accumulate(T, monkeypatch, d):
    from fadtk_amd.hip import Moments
    xa = X.int_rows_torch(9000 + d, 16 * d + 33, d, device="cuda")
    xb = X.int_rows_torch(9100 + d, 16 * d + 1, d, device="cuda")

    def run():
        with Moments(d) as m:
            m.set_timing(True)
            m.update(xa); m.update(xb)
            assert m.last_timing()[2] == 2
            return [m.export()]
    got = on_plans(monkeypatch, run)
    check(got[0], add(X.exact_moments(xa.cpu().numpy()), X.exact_moments(xb.cpu().numpy())), f"two slab updates d={d}")


@pytest.fixture(scope="module")
def thirty_two_sets(T):
    """32 sets at D = 512, n_i = 8192 + 37 i (each at least 16 D rows), drawn on the device, with their host references; given back
    when the file is done."""
    xs = [X.int_rows_torch(5000 + i, 8192 + 37 * i, 512, device="cuda") for i in range(32)]
    refs = [X.exact_moments(x.cpu().numpy()) for x in xs]
    yield xs, refs
    del xs[:], refs[:]
    T.cuda.empty_cache()


def test_slab_thirty_two_sets_one_call(T, monkeypatch, thirty_two_sets):
    """kMaxSets256 = 32 matrices in ONE launch of each kernel (more than 16: only the slab route carries that many)."""
    from fadtk_amd.hip import Moments
    xs, refs = thirty_two_sets

    def run():
        accs = [Moments(512) for _ in xs]
        accs[0].set_timing(True)
        Moments.update_multi(accs, xs)
        assert accs[0].last_timing()[2] == 2
        out = [a.export() for a in accs]
        for a in accs:
            a.close()
        return out
    got = on_plans(monkeypatch, run)
    for i, ref in enumerate(refs):
        check(got[i], ref, f"set {i} of 32")


def test_slab_twenty_sets_one_short(T, monkeypatch, thirty_two_sets):
    """20 sets, one of them 100 rows: not eligible for the slab kernel as a whole, so fad_moments_update_multi goes sixteen at a
    time (16 on the 128 x 128 kernel -- the short set is among them -- then 4, which are all long: the slab kernel)."""
    from fadtk_amd.hip import Moments
    xs, refs = thirty_two_sets
    xs, refs = list(xs[:20]), list(refs[:20])
    xs[7] = xs[7][:100]
    refs[7] = X.exact_moments(xs[7].cpu().numpy())

    def run():
        accs = [Moments(512) for _ in xs]
        accs[0].set_timing(True); accs[16].set_timing(True)      # (the first handle of each batch owns its launch's events)
        Moments.update_multi(accs, xs)
        assert accs[0].last_timing()[2] == 0 and accs[16].last_timing()[2] == 2
        out = [a.export() for a in accs]
        for a in accs:
            a.close()
        return out
    got = on_plans(monkeypatch, run)
    for i, ref in enumerate(refs):
        check(got[i], ref, f"set {i} of 20")


def test_thirty_three_sets_refused_whole(T, thirty_two_sets):
    """The binding takes 1 .. 32 accumulators (fad_moments_update_multi itself answers FAD_ERR_INVALID above kMaxSets256): a longer
    list is refused before anything is enqueued, and no handle is left half-updated."""
    from fadtk_amd.hip import Moments
    xs, _ = thirty_two_sets
    blocks = list(xs) + [xs[0]]
    accs = [Moments(512) for _ in blocks]
    with pytest.raises(AssertionError):
        Moments.update_multi(accs, blocks)
    # ... and the C entry itself, with the very tables the binding would have passed
    import ctypes as C
    from fadtk_amd import _capi as K
    m = len(accs)
    views = [K.rows_view(b) for b in blocks]
    hs = (C.c_void_p * m)(*[a._h for a in accs])
    ptrs = (C.c_void_p * m)(*[v[0] for v in views])
    ns = (C.c_int64 * m)(*[v[1] for v in views])
    lds = (C.c_int64 * m)(*[v[3] for v in views])
    rc = K.load_library().fad_moments_update_multi(m, hs, ptrs, ns, lds, views[0][4], K.current_stream_ptr(0))
    assert rc == K.FAD_ERR_INVALID and "count=33" in K.last_error()
    for a in accs:
        assert not a.export().any()
        a.close()


# ========================================================================================= D. shift guard, still exact
def _guard_rows(seed, n, d, cols):
    """Plain columns in [-8, 8] (no shift: mean^2 <= var), offset columns 48 + {-1, 0, 1}, one constant column."""
    return X.offset_columns(X.int_rows(seed, n, d, -8, 8), cols, 48, 1, seed)


def _middle_cols(d):
    return (0, 255, 256, d - 2, d - 1) if d > 256 else (0, 127, 128, d - 2, d - 1)


GUARD_CASES = [                                    # (d, TILE256 knob, variant, offset columns ..., constant column)
    (256, "1", 0, (2, 5, 9)),                      # first tile
    (256, "1", 0, (126, 127, 128, 129, 131)),      # straddling the seam of tiles 0 and 1
    (520, "0", 0, (3, 511, 512, 517, 519)),        # the ragged fifth tile of the 128 x 128 kernel
    (520, "1", 2, (3, 255, 256, 513, 519)),        # the ragged last superblock of the slab kernel
    (768, "1", 2, (1, 511, 512, 700, 767)),        # the Z superblock
]


@pytest.mark.parametrize("guard", ["1", "0"])
@pytest.mark.parametrize("d,knob,variant,cols", GUARD_CASES)
def test_guard_second_pass_exact(T, monkeypatch, d, knob, variant, cols, guard):
    """float16 rows of at least 16 D rows with columns far from zero: the tile kernels' second pass over x - c and the float64
    un-shift in the reduce.  c sits on float16's 2^-5 grid near 48, x - c is a multiple of 2^-5 below 1.3 in magnitude, products
    are multiples of 2^-10 and every partial sum fits float32 (test_moments_exact_host.py).  With the guard switched off the same
    rows are exact as well (the runs of both plans stay below 2^24 / 49^2 = 6987 rows): the guard is right, it did not hide an error."""
    monkeypatch.setenv("FAD_MOMENTS_TILE256", knob)
    monkeypatch.setenv("FAD_MOMENTS_SHIFT_GUARD", guard)
    n = 16 * d + 33
    x = _guard_rows(60 + d, n, d, cols)
    xt = dev(T, x, "fp16")
    got = on_plans(monkeypatch, lambda: [one_update(xt, d, variant)])
    check(got[0], X.exact_moments(x), f"guard={guard} d={d} cols={cols}")


@pytest.mark.parametrize("guard", ["1", "0"])
def test_guard_two_level_unshift_exact(T, monkeypatch, guard):
    """274 splits at D = 8: the un-shift happens in moments_presum, split by split."""
    monkeypatch.setenv("FAD_MOMENTS_SHIFT_GUARD", guard)
    d, n = 8, 70001
    x = _guard_rows(61, n, d, (1, 2, 5))
    xt = dev(T, x, "fp16")
    got = on_plans(monkeypatch, lambda: [one_update(xt, d, 0)])
    check(got[0], X.exact_moments(x), f"guard={guard} two-level un-shift")


@pytest.mark.parametrize("guard", ["1", "0"])
def test_guard_float64_redo_bfloat16(T, monkeypatch, guard):
    """bfloat16 rows have no second pass: a flagged set is redone by the float64 kernel."""
    monkeypatch.setenv("FAD_MOMENTS_SHIFT_GUARD", guard)
    d, n = 256, 16 * 256 + 33
    x = _guard_rows(62, n, d, (126, 127, 128, 129, 131))
    xt = dev(T, x, "bf16")
    got = on_plans(monkeypatch, lambda: [one_update(xt, d, 0)])
    check(got[0], X.exact_moments(x), f"guard={guard} bfloat16 redo")


def _multi(T, monkeypatch, d, xs, dtype="fp16", variant=None):
    from fadtk_amd.hip import Moments
    blocks = [dev(T, x, dtype) for x in xs]

    def run():
        accs = [Moments(d) for _ in xs]
        accs[0].set_timing(True)
        Moments.update_multi(accs, blocks)
        if variant is not None:
            assert accs[0].last_timing()[2] == variant
        out = [a.export() for a in accs]
        for a in accs:
            a.close()
        return out
    return on_plans(monkeypatch, run)


@pytest.mark.parametrize("guard", ["1", "0"])
def test_guard_float64_redo_with_short_set(T, monkeypatch, guard):
    """One set of the launch is shorter than 16 D: no second pass for the whole launch, the flagged set takes the float64 redo."""
    monkeypatch.setenv("FAD_MOMENTS_SHIFT_GUARD", guard)
    d = 256
    xs = [_guard_rows(63, 16 * d + 33, d, (2, 127, 128, 250, 255)), X.int_rows(64, 100, d, -8, 8)]
    got = _multi(T, monkeypatch, d, xs, variant=0)
    for i, x in enumerate(xs):
        check(got[i], X.exact_moments(x), f"guard={guard} set {i} (launch with a short set)")


@pytest.mark.parametrize("guard", ["1", "0"])
@pytest.mark.parametrize("d,variant", [(256, 0), (768, 2)])
def test_guard_only_middle_set_flagged(T, monkeypatch, d, variant, guard):
    """Three sets, the gate of the second pass up for set 1 alone: sets 0 and 2 keep their first-pass sums."""
    monkeypatch.setenv("FAD_MOMENTS_SHIFT_GUARD", guard)
    xs = [X.int_rows(65 + d, 16 * d + 32, d, -8, 8), _guard_rows(66 + d, 16 * d + 33, d, _middle_cols(d)),
          X.int_rows(67 + d, 16 * d + 63, d, -8, 8)]
    got = _multi(T, monkeypatch, d, xs, variant=variant)
    for i, x in enumerate(xs):
        check(got[i], X.exact_moments(x), f"guard={guard} d={d} set {i} of 3")


# ========================================================================================= E. indexed rows
def _index_lists(n_src, lengths, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k, m in enumerate(lengths):
        run = min(500, n_src)
        head = np.concatenate([[0, n_src - 1, 0, n_src - 1, k % n_src, k % n_src],      # both ends, repeats
                               np.arange(run), np.arange(n_src - 1, n_src - 1 - run, -1)])   # a sorted run, a reversed run
        fill = rng.integers(0, n_src, size=m - head.size)
        out.append(np.concatenate([head, fill]).astype(np.int32))
        assert out[-1].size == m
    return out


@pytest.mark.parametrize("d,variant", [(512, 2), (768, 2), (128, 0)])
def test_indexed_rows_exact(T, monkeypatch, d, variant):
    """update_multi_indexed: the gather inside the slab kernel (every list at least 16 D long), and at D = 128 the fallback that
    gathers into the staging area and takes the ordinary route."""
    from fadtk_amd.hip import Moments
    n_src = 8 * d + 64                             # (2 n_src + 5 = 16 D + 133: no split of a handful of rows, whose flag would go up)
    x = X.int_rows(80 + d, n_src, d)
    xt = dev(T, x, "fp16")
    idx = _index_lists(n_src, (16 * d + 1, 16 * d + 37, 2 * n_src + 5), 81 + d)
    idx_t = [T.from_numpy(i).to("cuda") for i in idx]

    def run():
        accs = [Moments(d) for _ in idx]
        accs[0].set_timing(True)
        Moments.update_multi_indexed(accs, xt, idx_t)
        assert accs[0].last_timing()[2] == variant
        out = [a.export() for a in accs]
        for a in accs:
            a.close()
        return out
    got = on_plans(monkeypatch, run)
    for k, i in enumerate(idx):
        check(got[k], X.exact_moments(x[i]), f"indexed d={d} list {k}")


# ========================================================================================= F. segments
SEG_LENS = (1, 2, 255, 256, 257, 2250, 8193, 1)


@pytest.mark.parametrize("guard", ["1", "0"])
@pytest.mark.parametrize("ref_mean", [False, True])
@pytest.mark.parametrize("on_device", [True, False])
@pytest.mark.parametrize("d", (128, 768))
def test_segmented_exact(T, monkeypatch, d, on_device, ref_mean, guard):
    """update_segmented on file-aligned splits (aligned float16 rows, 1246 rows per run on average): the moments, every per-segment
    column sum, and -- with the reference mean carried -- numpy's float32 running sums, which are sequential float32 adds of
    integers below 2^24 (8193 x 31) and so equal the integer sums.  A split that holds only the files of one and two rows, or the
    last file of one row, raises the shift flag (no variance to speak of), and file-aligned splits have no second pass: with the
    guard on the moments are the float64 redo's, with FAD_MOMENTS_SHIFT_GUARD=0 the tile kernel's own."""
    from fadtk_amd.hip import Moments
    monkeypatch.setenv("FAD_MOMENTS_SHIFT_GUARD", guard)
    off = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int64)
    x = X.int_rows(90 + d, int(off[-1]), d)
    rows = dev(T, x, "fp16") if on_device else x.astype(np.float16)
    want = np.stack([x[a:b].sum(axis=0) for a, b in zip(off[:-1], off[1:])])

    def run():
        with Moments(d) as m:
            if ref_mean:
                m.set_reference_mean(True)
                sums, runs = m.update_segmented(rows, off, want_runsums=True)
                assert runs.dtype == np.float32 and np.array_equal(runs.astype(np.float64), want)
            else:
                sums = m.update_segmented(rows, off)
            assert np.array_equal(sums, want)
            return [m.export()]
    got = on_plans(monkeypatch, run)
    check(got[0], X.exact_moments(x), f"segmented d={d} device={on_device} ref_mean={ref_mean}")


# ========================================================================================= G. host rows in pieces
def test_host_rows_in_pieces_exact(T, monkeypatch):
    """A numpy float16 matrix of 200 003 x 128 (51 MB): update_any cuts it into pieces of 24 MiB -- 98 304 rows, then the remaining
    101 699 as one piece (no runt at the end) -- copied on the handle's copy stream while the previous piece is summed."""
    d, n = 128, 200003
    x = X.int_rows(95, n, d)
    rows = x.astype(np.float16)
    got = on_plans(monkeypatch, lambda: [one_update(rows, d, 0)])
    check(got[0], X.exact_moments(x), "host rows in pieces")


# ========================================================================================= H. additivity
@pytest.mark.parametrize("d,variant", [(256, 0), (512, 2)])
def test_additivity_merge_import_finalize(T, monkeypatch, d, variant):
    """update(x[:k]) + update(x[k:]) merged, and the export imported into a third handle, equal the moments of x bit for bit -- for
    k on a seam of every plan (16 D: a multiple of every run length's 32- and 64-row stage) and off one.  finalize() against the
    same formula in float64 on the exact integers."""
    from fadtk_amd.hip import Moments
    n = 32 * d + 50
    x = X.int_rows(97 + d, n, d)
    xt = dev(T, x, "fp16")
    ref = X.exact_moments(x)
    for k in (16 * d, 16 * d + 13):
        def run():
            with Moments(d) as a, Moments(d) as b, Moments(d) as c:
                a.set_timing(True); b.set_timing(True)
                a.update(xt[:k]); b.update(xt[k:])
                assert a.last_timing()[2] == variant and b.last_timing()[2] == variant
                a.merge(b)
                c.import_(a.export())
                mu, cov, cnt = c.finalize()
                return [a.export(), c.export(), mu, cov.ravel(), np.array([float(cnt)])]
        got = on_plans(monkeypatch, run)
        check(got[0], ref, f"merge d={d} k={k}")
        check(got[1], ref, f"import d={d} k={k}")
        # finalize (moments_finalize_kernel): mu = s / n -- one correctly rounded division of exact integers on either side, so the
        # two quotients may differ by the two roundings at most: |dmu| <= 2 u |mu|.  cov = (M - (s_a s_b) / n) / (n - 1): s_a s_b is
        # an exact integer below 2^53; the quotient t rounds once (u |t|), the difference once (u |M - t|), the last quotient once
        # (u |cov|): |dcov| <= u (|t| + 2 |M - t|) / (n - 1) per side, twice that between the two.
        _, s, m = ref
        mu_ref = s / n
        t = np.outer(s, s) / n
        cov_ref = (m - t) / (n - 1)
        assert got[4][0] == n
        assert np.all(np.abs(got[2] - mu_ref) <= 2 * U * np.abs(mu_ref))
        bound = 2 * U * (np.abs(t) + 2 * np.abs(m - t)) / (n - 1)
        cov = got[3].reshape(d, d)
        assert np.all(np.abs(cov - cov_ref) <= bound), f"finalize d={d}: {np.max(np.abs(cov - cov_ref) / np.maximum(bound, 1e-300))} of the bound"
        assert np.array_equal(cov, cov.T)
