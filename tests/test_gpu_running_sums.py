"""np.mean's float32 running column sums (fad_moments_set_reference_mean) on every route that walks them, bit for bit
against the plain loop of running_sum_reference.py, on rows whose sum depends on the order (test_running_sum_host.py proves that of
these very rows): the float16 walk on the side stream (plain, indexed, from a job table), moments_running_colsum<T, WIDE>,
segment_running_sums<T, WIDE>, the tile kernel's WALK, and the host code that picks among them, carries the sum across updates and
orders attached and detached walks.

Every comparison is of float32 values with assert_array_equal (NaN equals NaN): finalize()'s mean float64(float32(float64(run) / n))
against the same quotient of the reference's sum, or update_segmented's raw float32 sums.  Padding columns hold NaN, so a read past d
shows.  Covariances are not asserted on these rows: their kernels have tests and tolerances of their own."""
import functools

import numpy as np
import pytest

import running_sum_reference as RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from fadtk_amd import _capi, hip
    _capi.require_gpu(0)
    return hip


def place(rows, placement):
    """As in test_gpu_songs.py: host rows as stored; device rows contiguous (`dev`), with an aligned base and ld % 8 == 0 (`pitch8`), or
    starting one column in with ld = d + 2 (`odd`: neither base nor pitch 16-byte aligned).  Padding columns hold NaN."""
    import torch
    if placement == "host":
        return rows
    t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(rows)
    if placement == "dev":
        return t.cuda()
    n, d = t.shape
    if placement == "pitch8":
        ld = 8 * ((d + 8) // 8)
        big = torch.full((n, ld), float("nan"), dtype=t.dtype, device="cuda")
        big[:, :d] = t.cuda()
        return big[:, :d]
    big = torch.full((n, d + 2), float("nan"), dtype=t.dtype, device="cuda")
    big[:, 1:d + 1] = t.cuda()
    return big[:, 1:d + 1]


def walk_of(rows):
    """The walk moments.hip: running_sums should launch for these rows, re-derived HERE from the conditions it tests: element type,
    d % (16 / element size), base and pitch 16-byte aligned (host rows: staged to ld = d on an aligned base; a host bfloat16 tensor goes
    in as float32).  The library offers no observation of the walk's route, so `assert walk_of(rows) == route` guards the case tables
    and the placement helper (a `pitch8` that lost its alignment would quietly test another kernel); it is no evidence of which kernel ran."""
    from fadtk_amd import _capi as K
    ptr, _, d, ld, code, on_dev, _ = K.rows_view(rows)
    if not on_dev:
        ptr, ld = 0, d
    es = 4 if code == K.FAD_F32 else 2
    wide = d % (16 // es) == 0 and ptr % 16 == 0 and (ld * es) % 16 == 0
    if code == K.FAD_F16:
        return "h16" if wide else "f16 narrow"
    return ("bf16" if code == K.FAD_BF16 else "f32") + (" wide" if wide else " narrow")


@functools.lru_cache(maxsize=None)
def reference_sum(dtype, d, n):
    return RS.running_sum(RS.as_f32(RS.rows_for(dtype, d, n)))


def mean_and_count(m):
    mu, _, n = m.finalize()
    assert m.count == n
    return mu, n


# --------------------------------------------------------------------------------- A: one plain update
@pytest.mark.parametrize("route,dtype,d,n,pl", RS.PLAIN_CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_one_update_returns_the_sequential_float32_sum(hip, route, dtype, d, n, pl):
    """h16: 192-row tiles, four in flight, three register sets of 16 rows, a partial last tile, clamped loads past the end, the XCD
    remap at d = 512, a half-filled last workgroup at d = 136 and d = 24.  Generic kernel: 1024-row tiles in two LDS buffers, the wide
    stage's surplus rows, the narrow stage's column guard.  `walk_of` is the test's own copy of the dispatch conditions: the assert
    says that the placement is what the case's route needs, not that the route was observed."""
    x = RS.rows_for(dtype, d, n)
    rows = place(x, pl)
    assert walk_of(rows) == route
    with hip.Moments(d) as m:
        m.set_reference_mean(True)
        m.update(rows)
        mu, cnt = mean_and_count(m)
    assert cnt == n
    np.testing.assert_array_equal(mu, RS.mean_of(reference_sum(dtype, d, n), n))


# --------------------------------------------------------------------------------- B: carry across updates
def test_pieces_carry_the_sum_like_the_concatenation(hip):
    """Pieces of 1, 16, 175 and 577 rows on the float16 walk (start_zero only for the first): after every piece the mean is that of the
    rows so far, walked in one go."""
    d, total = RS.MULTI_D, sum(RS.CARRY_PIECES)
    x = RS.rows_for("float16", d, total)
    xf = RS.as_f32(x)
    with hip.Moments(d) as m:
        m.set_reference_mean(True)
        at = 0
        for p in RS.CARRY_PIECES:
            rows = place(x[at:at + p], "dev")
            assert walk_of(rows) == "h16"
            m.update(rows)
            at += p
            assert m.count == at
            if at >= 2:
                mu, cnt = mean_and_count(m)
                assert cnt == at
                np.testing.assert_array_equal(mu, RS.mean_of(RS.running_sum(xf[:at]), at), err_msg=f"after {at} rows")


def _pieces(x, pieces):
    """The pieces of x, placed; with the placement asserted (walk_of: the test's own copy of the dispatch conditions)."""
    out, at = [], 0
    for p, pl in pieces:
        out.append(place(x[at:at + p], pl))
        assert walk_of(out[-1]) == ("h16" if pl == "dev" else "f16 narrow")
        at += p
    return out


def test_the_carry_passes_between_the_side_stream_and_the_callers_stream(hip):
    """float16 pieces placed dev / odd / dev: the float16 walk on the side stream, the generic kernel on the caller's stream, the float16
    walk again, each continuing the other's sum; attached, read after every piece."""
    d = RS.MULTI_D
    total = sum(p for p, _ in RS.ALTERNATING_PIECES)
    x = RS.rows_for("float16", d, total)
    xf = RS.as_f32(x)
    with hip.Moments(d) as m:
        m.set_reference_mean(True)
        at = 0
        for rows in _pieces(x, RS.ALTERNATING_PIECES):
            m.update(rows)
            at += rows.shape[0]
            mu, cnt = mean_and_count(m)
            assert cnt == at
            np.testing.assert_array_equal(mu, RS.mean_of(RS.running_sum(xf[:at]), at), err_msg=f"after {at} rows")
    assert at == total


def test_detached_walks_hand_the_carry_over_in_both_directions_and_readers_wait(hip):
    """set_reference_mean(True, detached=True), pieces of 80 000 (dev), 10 001 (odd) and 50 000 (dev) rows, all resident and complete
    before the first call (the caller's promise: one synchronize), then three updates back to back and finalize at once, nothing
    waited for in between.  Every walk is long (0.3, 0.04, 0.2 ms) against the microseconds the host needs to enqueue the next, so
    each hand-over is taken while the walk before it still runs:
    * the generic kernel on the caller's stream continues the detached walk of piece 1 (running_sums: the wait for rs_pending);
    * the detached walk of piece 3 continues the generic kernel's sums (the wait for rs_caller -- the side stream "waits for nothing"
      else, and read the sums of piece 1 alone before that wait existed);
    * finalize reads behind the walk of piece 3 (settle: rs_pending), while the caller's stream holds only the short moments kernels.
    A first round of the same updates lets the handle allocate its buffers, so that no allocation stands between the updates timed here."""
    import torch
    d = RS.MULTI_D
    total = sum(p for p, _ in RS.DETACHED_PIECES)
    x = RS.rows_for("float16", d, total)
    pieces = _pieces(x, RS.DETACHED_PIECES)             # (kept alive to the end: a detached walk reads them whenever it runs)
    want = RS.mean_of(reference_sum("float16", d, total), total)
    with hip.Moments(d) as m:
        m.set_reference_mean(True, detached=True)
        for rnd in range(2):
            m.reset()
            torch.cuda.synchronize()
            for rows in pieces:
                m.update(rows)
            mu, _, cnt = m.finalize()
            assert cnt == total and m.count == total
            np.testing.assert_array_equal(mu, want, err_msg=f"round {rnd}")


def test_reset_starts_the_sum_again(hip):
    d = RS.MULTI_D
    first, second = RS.RESET_FEEDS
    with hip.Moments(d) as m:
        m.set_reference_mean(True)
        m.update(place(RS.rows_for("float16", d, first), "dev"))
        mu, cnt = mean_and_count(m)
        assert cnt == first
        np.testing.assert_array_equal(mu, RS.mean_of(reference_sum("float16", d, first), first))
        m.reset()
        m.update(place(RS.rows_for("float16", d, second), "dev"))
        mu, cnt = mean_and_count(m)
    assert cnt == second
    np.testing.assert_array_equal(mu, RS.mean_of(reference_sum("float16", d, second), second))


def test_imported_statistics_fall_back_to_the_exact_mean(hip):
    """import_ (here of the handle's own export) loses the row order: finalize returns the exact mean again, to the tolerance
    test_calc_embd_statistics_returns_numpys_own_mean_for_frames_with_an_offset has for the switch off (Gaussian rows with an offset, as
    there: that tolerance was not set for columns that cancel)."""
    n, d = 2049, RS.MULTI_D
    x = RS.gaussian_rows(n, d, 0.5, np.float16)
    with hip.Moments(d) as m:
        m.set_reference_mean(True)
        m.update(place(x, "dev"))
        carried, cnt = mean_and_count(m)
        np.testing.assert_array_equal(carried, RS.mean_of(RS.running_sum(RS.as_f32(x)), n))
        m.import_(m.export())
        mu, cnt2 = mean_and_count(m)
    assert cnt == n and cnt2 == n
    exact = x.astype(np.float64).mean(axis=0)
    np.testing.assert_allclose(mu, exact, rtol=2e-6)
    assert (mu != carried).any(), "the exact mean has more than float32's bits: the carried one must be gone"


# --------------------------------------------------------------------------------- C: update_multi
def test_update_multi_of_seventeen_walks_splits_into_launches_of_sixteen(hip):
    """18 float16 handles at d = 136 with the switch on, one of them without rows: fad_moments_update_multi drops the empty one and
    sends the 17 left sixteen at a time (m > kMaxSets with a handle that wants the walk: the walk's launch table has 16 jobs).  Every
    handle has its own rows' sum."""
    import torch
    d = RS.MULTI_D
    assert sum(n > 0 for n in RS.MULTI_N) == 17
    accs = [hip.Moments(d) for _ in RS.MULTI_N]
    try:
        blocks = []
        for m, n in zip(accs, RS.MULTI_N):
            m.set_reference_mean(True)
            blocks.append(place(RS.rows_for("float16", d, n), "dev") if n else torch.empty((0, d), dtype=torch.float16, device="cuda"))
            assert n == 0 or walk_of(blocks[-1]) == "h16"
        hip.Moments.update_multi(accs, blocks)
        for m, n in zip(accs, RS.MULTI_N):
            assert m.count == n
            if n:
                mu, cnt = mean_and_count(m)
                np.testing.assert_array_equal(mu, RS.mean_of(reference_sum("float16", d, n), n), err_msg=f"n={n}")
    finally:
        for m in accs:
            m.close()


def test_update_multi_with_the_switch_on_two_handles_of_four(hip):
    """The two handles without the switch return the exact mean (Gaussian rows with an offset: the tolerance of the switch-off case of
    test_calc_embd_statistics_returns_numpys_own_mean_for_frames_with_an_offset), the two with it their running sums: the walk's jobs
    are packed past the handles that do not want it."""
    d = RS.MULTI_D
    ns = (385, 769, 193, 961)
    on = (False, True, False, True)
    xs = [RS.rows_for("float16", d, n) if o else RS.gaussian_rows(n, d, 0.5, np.float16) for n, o in zip(ns, on)]
    accs = [hip.Moments(d) for _ in ns]
    try:
        for m, o in zip(accs, on):
            m.set_reference_mean(o)
        hip.Moments.update_multi(accs, [place(x, "dev") for x in xs])
        for m, n, o, x in zip(accs, ns, on, xs):
            mu, cnt = mean_and_count(m)
            assert cnt == n
            if o:
                np.testing.assert_array_equal(mu, RS.mean_of(reference_sum("float16", d, n), n), err_msg=f"n={n}")
            else:
                np.testing.assert_allclose(mu, x.astype(np.float64).mean(axis=0), rtol=2e-6, err_msg=f"n={n}")
    finally:
        for m in accs:
            m.close()


def test_update_multi_of_three_bfloat16_handles(hip):
    """moments_running_colsum<raw_bf16, true> with three jobs of different lengths in one launch (grid y = 3)."""
    d = RS.MULTI_D
    accs = [hip.Moments(d) for _ in RS.MULTI_BF16_N]
    try:
        blocks = [place(RS.rows_for("bfloat16", d, n), "dev") for n in RS.MULTI_BF16_N]
        for m, b in zip(accs, blocks):
            m.set_reference_mean(True)
            assert walk_of(b) == "bf16 wide"
        hip.Moments.update_multi(accs, blocks)
        for m, n in zip(accs, RS.MULTI_BF16_N):
            mu, cnt = mean_and_count(m)
            assert cnt == n
            np.testing.assert_array_equal(mu, RS.mean_of(reference_sum("bfloat16", d, n), n), err_msg=f"n={n}")
    finally:
        for m in accs:
            m.close()


# --------------------------------------------------------------------------------- D: update_multi_indexed
def _indexed(hip, d, n_src, lengths, want_variant):
    import torch
    src = RS.rows_for("float16", d, n_src)
    srcf = RS.as_f32(src)
    rows = place(src, "dev")
    idx = [RS.index_list(length, n_src, k) for k, length in enumerate(lengths)]
    accs = [hip.Moments(d) for _ in lengths]
    try:
        for m in accs:
            m.set_reference_mean(True)
        accs[0].set_timing(True)
        hip.Moments.update_multi_indexed(accs, rows, [torch.from_numpy(i).cuda() for i in idx])
        assert accs[0].last_timing()[2] == want_variant
        for m, i in zip(accs, idx):
            mu, cnt = mean_and_count(m)
            assert cnt == len(i)
            np.testing.assert_array_equal(mu, RS.mean_of(RS.running_sum(srcf[i]), len(i)), err_msg=f"list of {len(i)}")
    finally:
        for m in accs:
            m.close()


def test_indexed_walk_follows_the_index_lists_order(hip):
    """moments_running_colsum_h16<.., IDX>: three lists drawn with replacement from 300 rows at d = 512, each at least 16 d long (what the
    256-column-slab kernel asks for, and the indexed walk rides with it: last_timing's variant 2 says that route was taken), of 8192,
    8257 and 8448 entries: whole tiles, a partial tile of one row more than 16, 44 whole tiles.  The reference walks rows[idx] in idx's order."""
    _indexed(hip, RS.INDEXED_D, RS.INDEXED_SRC, RS.INDEXED_LENGTHS, want_variant=2)


def test_indexed_update_that_gathers_first(hip):
    """d = 136, a list of 193: not the slab kernel's shape, so the rows are gathered into the handle's staging area and walked as a plain
    (attached) update -- the float64 kernel takes the moments (variant 1)."""
    _indexed(hip, RS.GATHER_D, RS.GATHER_SRC, (RS.GATHER_LENGTH,), want_variant=1)


# --------------------------------------------------------------------------------- E: per-segment raw sums
@pytest.mark.parametrize("route,dtype,d,sizes,pl", RS.SEGMENT_CASES, ids=lambda v: str(v).replace(" ", "_") if isinstance(v, str) else f"{len(v)}seg" if isinstance(v, tuple) else str(v))
def test_segment_running_sums_are_the_sequential_sums(hip, route, dtype, d, sizes, pl):
    """update_segmented(want_runsums=True) returns the raw float32 sums.  Which kernel walks them (moments.hip):
    * job table h16 -- segment_running_sums_launch: float16, d % 8 == 0, d >= 256, aligned, mean segment >= 256 rows; the tile kernel does
      not walk because the file of 8200 rows is two runs (n_runs != n_segments).  The empty segment's workgroups write zeros.
    * thread per 8 columns -- the same function's fallback, 16-bit rows, d % 8 == 0, aligned: loops of 32, 4 and 1 rows
      (mean segment 52 rows: update_segmented_impl does not fuse, nothing else walks).
    * thread per column -- float32 (always), d % 8 != 0, or the `odd` placement: loops of 8 and 1 rows.
    * tile kernel WALK -- update_segmented_impl: aligned 16-bit rows, segments that cover the rows, every file one run of <= 8192 rows,
      mean run >= 256 rows: tr_kernel_walk leaves the sums, no second pass."""
    x = RS.segment_rows(dtype, d, sizes)
    xf = RS.as_f32(x)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = place(x, pl)
    aligned16 = walk_of(rows) in ("h16", "bf16 wide")
    assert aligned16 == (route != "thread per column")
    with hip.Moments(d) as m:
        sums, runs = m.update_segmented(rows, off, want_runsums=True)
        assert m.count == int(off[-1])
    want = np.stack([RS.running_sum(xf[off[s]:off[s + 1]]) for s in range(len(sizes))])
    assert runs.dtype == np.float32 and runs.shape == want.shape
    for s, n in enumerate(sizes):
        np.testing.assert_array_equal(runs[s], want[s], err_msg=f"segment {s} of {n} rows")
    assert not runs[[s for s, n in enumerate(sizes) if n == 0]].any()


# --------------------------------------------------------------------------------- F: non-finite entries on the generic routes
@pytest.mark.parametrize("route,dtype,d,n,pl", RS.NONFINITE_CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_non_finite_entries_propagate_like_in_the_reference(hip, route, dtype, d, n, pl):
    """A column with +Inf, one with NaN, one with +Inf in the last row of the first 1024-row tile and -Inf in the first row of the next
    (Inf - Inf = NaN across the tile edge): the walk carries what the sequential sum carries, every other column its finite sum."""
    x = RS.rows_for(dtype, d, n)
    x = x.clone() if dtype == "bfloat16" else x.copy()
    x[n // 3, 1] = float("inf")
    x[n // 2, d // 2] = float("nan")
    x[1023, d - 1] = float("inf")
    x[1024, d - 1] = float("-inf")
    want = RS.mean_of(RS.running_sum(RS.as_f32(x)), n)
    assert np.isposinf(want[1]) and np.isnan(want[d // 2]) and np.isnan(want[d - 1]) and np.isfinite(want).sum() == d - 3
    rows = place(x, pl)
    assert walk_of(rows) == route
    with hip.Moments(d) as m:
        m.set_reference_mean(True)
        m.update(rows)
        mu, cnt = mean_and_count(m)
    assert cnt == n
    np.testing.assert_array_equal(mu, want)
