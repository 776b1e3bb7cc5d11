"""The 256-column-slab moments kernel on 16x16x32 MFMAs (fadtk_amd/csrc/moments_tile256.h, tile256_layout.h): a lane holds eight
rows of a 32-row stage, a 32 x 32 block is four 16 x 16 sub-blocks, the one below the diagonal of a diagonal block is never issued.

Rows of small integers (tests/moments_exact_reference.py) make every sum exact in any order, so ``export()`` must EQUAL n, sum x and
every entry of sum x x^T -- at every row remainder around the eight-row groups (the plain tail, which the range check of the loads
fills with zeros, and the tail mask of the shifted pass), on a Z item, on a ragged last superblock and on indexed rows; every such
case under the split plan of the whole chip and under that of 8 CUs, which must agree bit for bit.  Two cases on Gaussian rows
check the guard's pick-up of sum x^2 from the new accumulator layout and a four-superblock launch (X items)."""
import numpy as np
import pytest

import moments_exact_reference as X
from oracle import fad_oracle as O

pytestmark = pytest.mark.gpu

PLANS = (None, "8")          # FAD_MOMENTS_CUS: unset (the chip's CUs) and 8


@pytest.fixture(scope="module")
def T():
    import torch
    from fadtk_amd import _capi
    _capi.require_gpu(0)
    return torch


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


def multi(monkeypatch, d, blocks):
    """One update_multi launch of the slab kernel over ``blocks`` -> exports (both plans, which must agree)."""
    from fadtk_amd.hip import Moments

    def run():
        accs = [Moments(d) for _ in blocks]
        accs[0].set_timing(True)
        Moments.update_multi(accs, blocks)
        assert accs[0].last_timing()[2] == 2
        out = [a.export() for a in accs]
        for a in accs:
            a.close()
        return out
    return on_plans(monkeypatch, run)


def with_tail(head_ref, tail):
    """Exact moments of (the rows behind ``head_ref``) + ``tail`` rows."""
    n, s, m = head_ref
    t = np.asarray(tail, dtype=np.float64)
    return n + t.shape[0], s + t.sum(axis=0), m + t.T @ t


# ----------------------------------------------------------------------------------------- row remainders, plain set and guard set
REMAINDERS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 31)
# offset columns 48 + {-1, 0, 1} of the guard set, one in every 32-column fragment (low and high sub-fragment in turn), so that a row
# the shifted pass fails to mask -- it would enter as -c -- shows in the blocks of every wave; the last one is constant
GUARD_COLS = tuple(32 * k + (5 if k % 2 == 0 else 21) for k in range(16))


def _guard_set(n0, tail, d):
    """Plain columns in [-8, 8], offset columns near 48.  The last ``tail`` rows are +v_j, -v_j, +v_j, ... in the plain columns: under
    the whole-chip plan they are a split of their own, and rows drawn at random there would have column means with many fractional
    bits as shifts (mean^2 > var happens easily on a handful of rows), outside the float32 budget that makes equality legitimate.
    Alternating rows keep mean^2 <= var (no shift) from two rows on, and a single row is its own integer mean."""
    x = X.int_rows(7101, n0 + tail, d, -8, 8)
    v = 1.0 + (np.arange(d) * 5) % 8
    x[n0:] = np.where(np.arange(tail)[:, None] % 2 == 0, v, -v)
    return X.offset_columns(x, GUARD_COLS, 48, 1, 7101)


@pytest.fixture(scope="module")
def remainder_sets(T):
    """A plain set and a guard set of 16 * 512 + 31 rows on the device, and the exact moments of their first 16 * 512 rows."""
    d, n0 = 512, 16 * 512
    plain = X.int_rows(7100, n0 + 31, d)
    guard = _guard_set(n0, 31, d)
    dev = [T.from_numpy(v.astype(np.float16)).to("cuda") for v in (plain, guard)]
    yield d, n0, (plain, guard), dev, [X.exact_moments(v[:n0]) for v in (plain, guard)]
    del dev[:]


@pytest.mark.parametrize("r", REMAINDERS)
def test_row_remainders_plain_and_guard_set(T, monkeypatch, remainder_sets, r):
    """n = 16 * 512 + r: the last stage of the last split holds r % 32 rows -- none, part or all of a lane's eight-row group.  The
    plain set's missing rows are zeros from the range check; the guard set's second pass (x - c) has to mask exactly the rows the
    lane holds, or the missing rows would enter as -c."""
    d, n0, host, dev, head = remainder_sets
    for cus in (256, 8):                             # the condition under which the second pass sums exactly, on both plans' splits
        rps = X.rows_per_split([n0 + r, n0 + r], d, "slab", cus)
        hit, c = X.guard_shifts(host[1][:n0 + r], rps)
        assert hit.all() and X.bit_budget(host[1][:n0 + r], shifts=(rps, c)) <= 24
    got = multi(monkeypatch, d, [v[:n0 + r] for v in dev])
    for k, name in enumerate(("plain", "guard")):
        check(got[k], with_tail(head[k], host[k][n0:n0 + r]), f"{name} set, n = 16 * 512 + {r}")


# ----------------------------------------------------------------------------------------- Z item, ragged last superblock
@pytest.mark.parametrize("d,extra", [(768, (1, 33, 63)), (520, (5,))])
def test_z_item_and_ragged_superblock(T, monkeypatch, d, extra):
    """D = 768: a Z item, whose quartets take alternate 32-row halves of a 64-row stage (the remainders put the last rows into the
    first half only, into both, and one short of both).  D = 520: eight live columns in the last superblock."""
    n0 = 16 * d
    x = X.int_rows(7200 + d, n0 + max(extra), d)
    xt = T.from_numpy(x.astype(np.float16)).to("cuda")
    head = X.exact_moments(x[:n0])
    for r in extra:
        got = multi(monkeypatch, d, [xt[:n0 + r]])
        check(got[0], with_tail(head, x[n0:n0 + r]), f"d = {d}, n = 16 d + {r}")


# ----------------------------------------------------------------------------------------- indexed rows
def test_indexed_rows(T, monkeypatch):
    """update_multi_indexed at D = 512: 8 192 + 17 indices with repeats into a source of 9 000 rows, against numpy on the
    gathered rows."""
    from fadtk_amd.hip import Moments
    d, n_src, m = 512, 9000, 8192 + 17
    x = X.int_rows(7300, n_src, d)
    xt = T.from_numpy(x.astype(np.float16)).to("cuda")
    rng = np.random.default_rng(7301)
    idx = np.concatenate([[0, n_src - 1, 0, n_src - 1, 5, 5], np.arange(300), np.arange(n_src - 1, n_src - 301, -1),
                          rng.integers(0, n_src, size=m - 606)]).astype(np.int32)
    assert idx.size == m and np.unique(idx).size < m
    idx_t = T.from_numpy(idx).to("cuda")

    def run():
        with Moments(d) as a:
            a.set_timing(True)
            Moments.update_multi_indexed([a], xt, [idx_t])
            assert a.last_timing()[2] == 2
            return [a.export()]
    got = on_plans(monkeypatch, run)
    check(got[0], X.exact_moments(x[idx]), "indexed rows")


# ----------------------------------------------------------------------------------------- the guard's pick-up of sum x^2
def test_guard_pick_up_from_the_new_layout(T, monkeypatch):
    """Gaussian float16 rows, D = 512, n = 9 000, columns 5..69 and 300..339 at 40 + 0.05 z: the guard reads sum x^2 off the diagonal
    of the diagonal blocks' accumulators.  With it the covariance of each outlier block is within 1e-6 of the oracle's RELATIVE TO
    THAT BLOCK (the bound and the form of test_moments_tile256_two_sets_one_launch_and_guard_second_pass); a handle created with
    FAD_MOMENTS_SHIFT_GUARD=0 misses it by more than 1e-7 (test_moments_shift_guard_large_mean_small_std at D = 256) -- so a pick-up
    that named the wrong element, and left the flag down, fails the first bound."""
    from fadtk_amd.hip import Moments
    rng = np.random.default_rng(7400)
    n, d = 9000, 512
    x = rng.standard_normal((n, d))
    x[:, 5:70] = 40.0 + 0.05 * x[:, 5:70]
    x[:, 300:340] = 40.0 + 0.05 * x[:, 300:340]
    x = x.astype(np.float16)
    xt = T.from_numpy(x).to("cuda")
    _, cov_o = O.embd_statistics(x)
    blocks = [np.ix_(range(5, 70), range(5, 70)), np.ix_(range(300, 340), range(300, 340))]
    with Moments(d) as m:
        m.set_timing(True)
        m.update(xt)
        assert m.last_timing()[2] == 2
        _, cov, n_got = m.finalize()
    assert n_got == n
    err = [np.abs(cov[b] - cov_o[b]).max() / np.abs(cov_o[b]).max() for b in blocks]
    print("guard on: error relative to the block", err)
    assert np.abs(cov - cov_o).max() <= 1e-6 * np.abs(cov_o).max()
    for e in err:
        assert e < 1e-6
    monkeypatch.setenv("FAD_MOMENTS_SHIFT_GUARD", "0")            # (read when a handle is created)
    with Moments(d) as m:
        m.update(xt)
        _, cov_fast, _ = m.finalize()
    gap = [np.abs(cov_fast[b] - cov_o[b]).max() for b in blocks]
    print("guard off: absolute error on the blocks", gap)
    for g in gap:
        assert g > 1e-7


# ----------------------------------------------------------------------------------------- four superblocks: X items
def test_gaussian_rows_four_superblocks(T):
    """D = 1024, n = 20 000 Gaussian float16 rows against float64 numpy at 1e-6 max|sum x x^T|: two P/Q pairs and four X items, whose
    eight XR waves walk the slots differently from a P/Q item's."""
    from fadtk_amd.hip import Moments
    rng = np.random.default_rng(7500)
    n, d = 20000, 1024
    x = (rng.standard_normal((n, d)) * (0.5 + np.arange(d) / d)).astype(np.float16)
    x[:, 1:] += (0.25 * x[:, :-1]).astype(np.float16)
    x64 = x.astype(np.float64)
    exact = x64.T @ x64
    with Moments(d) as m:
        m.set_timing(True)
        m.update(T.from_numpy(x).to("cuda"))
        assert m.last_timing()[2] == 2
        p = m.export()
    M = p[1 + d:].reshape(d, d)
    assert p[0] == n
    print("max |M - exact| / max |exact| =", np.abs(M - exact).max() / np.abs(exact).max())
    np.testing.assert_allclose(M, exact, rtol=0, atol=1e-6 * np.abs(exact).max())
    np.testing.assert_array_equal(M, M.T)
    np.testing.assert_allclose(p[1:1 + d], x64.sum(0), rtol=1e-7, atol=1e-5)
