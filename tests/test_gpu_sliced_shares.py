"""Every row's share of the sliced Wasserstein distance on the GPU (fad_sliced_shares; csrc/kad.hip and csrc/sliced_sort_pairs.h,
DESIGN.md 4.19) against tests/sliced_shares_reference.py, stage by stage:

(a) the sort, through index_x / index_y: every segment a permutation; sorted_x / sorted_y with the bits of the plain call; equal keys
    (equal float32 bits) carry ascending row indices; the float64 projections read along the returned order are non-decreasing up to
    2 delta (two neighbours each off by at most delta = sliced_reference.projection_bound).
(b) the match: the shares recomputed on the host in float64 FROM THE RETURNED sorted arrays, indices and q_l, in the documented order,
    equal the returned ones to the last bit.
(c) end to end: against float64 shares evaluated ALONG THE DEVICE'S ORDER (at near-ties a free float64 ordering may legitimately pair
    rows differently, and shares are discontinuous there: no bound holds against a free ordering).  A device difference is d* + e,
    |e| <= delta' = delta_x + delta_y, so per term |d^2 - d*^2| <= 2 |d*| delta' + delta'^2 and per row
        |share - reference| <= (sum_l sum_partners w_ij (2 |d*| delta' + delta'^2) / (n m q_l)) / L
    (sliced_shares_reference.share_bound; derived, computed per case, never taken from a GPU figure).  The worst ratio is printed as a
    [shares-err] line, with the difference to the free stable-argsort reference beside it (printed, not asserted).
(d) the sum: |sum share_x - sw2_squared| <= (n + L + 8) 2^-52 sw2_squared (non-negative terms, sequential sums), and m for y.
(e) the result fields and values: the bits of fad_sliced_wasserstein on the same inputs.
(f) exact rows (integers x 2^e, integer directions, many ties): indices and shares equal the stable-argsort reference in the
    documented order bit for bit.
Measured on an MI355X over this file's cases (the [shares-err] lines, profiles/sliced_shares_gpu_tail.txt): the worst share error is
0.052 of its bound; the free ordering differs by up to 1.7e-3 of the largest share (a near-tie at 2047 rows), by under 3e-6 elsewhere.
No bound here comes from those figures.
Then the bitwise invariants (again, swapped, chunked, identical sets, scaling by 2^e), the sort's edges read from
fad_sliced_last_plan, the refusals and the command line."""
import ctypes as C
import functools

import numpy as np
import pytest

import sliced_reference as SR
import sliced_shares_reference as SS

pytestmark = pytest.mark.gpu
TOO_FEW, NOT_FINITE, INVALID = -6, -7, -1
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16", "fp32": "float32"}
SHAPES = ((1, 1, 5, 1), (1, 300, 37, 3), (300, 1, 37, 3), (2, 3, 1, 2), (255, 257, 128, 33), (257, 130, 64, 5), (129, 127, 2047, 2))
EXACT_SHAPES = ((1, 300, 37, 3), (2, 3, 1, 2), (255, 257, 128, 33), (257, 130, 64, 5), (129, 127, 2047, 2))
PITCHED = ((255, 257), (1, 300), (2, 3))
RESULT_FIELDS = ("sw2_squared", "std_error", "max_sliced", "max_index", "n", "m", "projections")


def _dev(a, dt, ld=None):
    """float32 values -> a torch CUDA tensor of dtype dt; with ld, a view of a wider buffer (row pitch ld > D) whose pitch entries are 7"""
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, TORCH_DT[dt]))
    if ld is None:
        return t
    wide = torch.full((t.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _inputs(x, y, dt, ldx=None, host=False):
    if host:
        npdt = {"fp16": np.float16, "fp32": np.float32}[dt]
        return x.astype(npdt), y.astype(npdt)
    return _dev(x, dt, ldx), _dev(y, dt)


def _run(x, y, t, dt, ldx=None, host=False):
    from fadtk_amd import hip
    xs, ys = _inputs(x, y, dt, ldx, host)
    return hip.sliced_shares(xs, ys, t, values=True, sorted_projections=True, indices=True)


def _plain(x, y, t, dt, ldx=None, host=False):
    from fadtk_amd import hip
    xs, ys = _inputs(x, y, dt, ldx, host)
    return hip.sliced_wasserstein(xs, ys, t, values=True, sorted_projections=True)


@functools.lru_cache(maxsize=None)
def _case(n, m, d, L, dt):
    x, y = SR.rows(n, m, d, dt)
    return x, y, SR.directions(L, d)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_result(got, plain, tag):
    for k in RESULT_FIELDS:
        assert _same_bits(np.float64(got[k]), np.float64(plain[k])), (tag, k, got[k], plain[k])
    for k in ("values", "sorted_x", "sorted_y"):
        assert _same_bits(got[k], plain[k]), (tag, k)


def _check_sort(got, x, y, t, dt, tag):
    """(a) -> the float64 projections of both sets [L x n], [L x m], q and the two projection bounds"""
    tr = SR.round_to_dtype(t, dt)
    px, q = SS.projections(x, t, dt)
    py, _ = SS.projections(y, t, dt)
    dx, dy = SR.projection_bound(x, tr, dt), SR.projection_bound(y, tr, dt)
    for side, p, delta in (("x", px, dx), ("y", py, dy)):
        idx, s = got[f"index_{side}"], got[f"sorted_{side}"]
        rows = p.shape[1]
        assert idx.dtype == np.int32 and idx.shape == s.shape == (len(t), rows), (tag, side)
        assert np.array_equal(np.sort(idx, axis=1), np.broadcast_to(np.arange(rows, dtype=np.int32), idx.shape)), (tag, side)
        tie = s.view(np.uint32)[:, 1:] == s.view(np.uint32)[:, :-1]
        assert np.all(np.diff(idx, axis=1)[tie] > 0), (tag, side)                      # equal keys: ascending rows
        along = np.take_along_axis(p, idx.astype(np.int64), 1)
        assert np.all(np.diff(along, axis=1) >= -2.0 * delta[:, None]), (tag, side)
        assert np.all(np.abs(s.astype(np.float64) - along) <= delta[:, None]), (tag, side)          # sorted[r] IS row index[r]'s projection
    return px, py, q, dx, dy


def _check_match(got, q, tag):
    """(b)"""
    ix, iy = got["index_x"].astype(np.int64), got["index_y"].astype(np.int64)
    hx, hy = SS.shares_from_sorted(got["sorted_x"].astype(np.float64), got["sorted_y"].astype(np.float64), ix, iy, q, ordered=True)
    assert got["share_x"].dtype == np.float64 and _same_bits(got["share_x"], hx), (tag, got["share_x"], hx)
    assert _same_bits(got["share_y"], hy), (tag, got["share_y"], hy)


def _check_sums(got, tag):
    """(d)"""
    L, sw2 = got["projections"], got["sw2_squared"]
    for k, rows in (("share_x", got["n"]), ("share_y", got["m"])):
        assert np.all(got[k] >= 0), (tag, k)
        total = SS.sequential_sum(got[k])
        assert abs(total - sw2) <= (rows + L + 8) * 2.0 ** -52 * sw2, (tag, k, total, sw2)


def _check(got, plain, x, y, t, dt, tag):
    n, m, L = len(x), len(y), len(t)
    assert (got["n"], got["m"], got["projections"]) == (n, m, L) and got["share_x"].shape == (n,) and got["share_y"].shape == (m,)
    _same_result(got, plain, tag)                                                      # (e)
    px, py, q, dx, dy = _check_sort(got, x, y, t, dt, tag)                             # (a)
    _check_match(got, q, tag)                                                          # (b)
    ix, iy = got["index_x"].astype(np.int64), got["index_y"].astype(np.int64)          # (c)
    ax, ay = np.take_along_axis(px, ix, 1), np.take_along_axis(py, iy, 1)
    rx, ry = SS.shares_from_sorted(ax, ay, ix, iy, q)
    bx, by = SS.share_bound(ax, ay, q, dx, dy)
    free = SS.shares(x, y, t, dt)
    for k, ref, b, idx in (("share_x", rx, bx, ix), ("share_y", ry, by, iy)):
        bound = np.zeros(b.shape[1])
        for l in range(L):
            row_b = np.zeros(b.shape[1])
            row_b[idx[l]] = b[l]
            bound = bound + row_b
        bound = bound / L
        err = np.abs(got[k] - ref)
        print(f"[shares-err] {tag} {k}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}; "
              f"worst difference to the free ordering / largest share {float(np.abs(got[k] - free[k]).max() / max(ref.max(), 1e-300)):.3g}")
        assert np.all(err <= bound), (tag, k, err, bound)
    _check_sums(got, tag)                                                              # (d)


# ----------------------------------------------------------------------------------------------------- (a) .. (e)
@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("n,m,d,L", SHAPES)
def test_against_reference(n, m, d, L, dt):
    x, y, t = _case(n, m, d, L, dt)
    ldx = d + 3 if (n, m) in PITCHED else None
    _check(_run(x, y, t, dt, ldx=ldx), _plain(x, y, t, dt, ldx=ldx), x, y, t, dt, f"{n}x{m}x{d} L={L} {dt}")


def test_host_rows():
    x, y, t = _case(257, 130, 64, 5, "fp16")
    got = _run(x, y, t, "fp16", host=True)
    _check(got, _plain(x, y, t, "fp16", host=True), x, y, t, "fp16", "host rows fp16")
    dev = _run(x, y, t, "fp16")
    for k in ("share_x", "share_y", "index_x", "index_y"):
        assert _same_bits(got[k], dev[k]), k


def test_python_layer():
    from fadtk_amd import calc_sliced_wasserstein, calc_sliced_wasserstein_shares, sliced_directions
    x, y, _ = _case(257, 130, 64, 5, "fp32")
    xo, yo = [0, 100, 100, 257], [0, 130]
    res = calc_sliced_wasserstein_shares(x, y, projections=16, seed=4, x_offsets=xo, y_offsets=yo)
    plain = calc_sliced_wasserstein(x, y, projections=16, seed=4)
    for k, v in plain.items():
        assert _same_bits(np.float64(res[k]), np.float64(v)), k
    low = _run(x, y, sliced_directions(64, 16, 4), "fp32", host=True)
    assert _same_bits(res["share_x"], low["share_x"]) and _same_bits(res["share_y"], low["share_y"])
    sx = res["share_x"]
    assert np.array_equal(res["file_share_x"], [float(np.sum(sx[:100])), 0.0, float(np.sum(sx[100:]))])
    assert res["file_share_y"].shape == (1,) and res["file_share_y"][0] == float(np.sum(res["share_y"]))
    assert res["file_lift_x"][0] == (res["file_share_x"][0] / res["sw2_squared"]) / (100 / 257) and np.isnan(res["file_lift_x"][1])
    assert abs(res["file_lift_y"][0] - 1.0) <= (130 + 16 + 8) * 2.0 ** -52
    assert "file_share_x" not in calc_sliced_wasserstein_shares(x, y, projections=16, seed=4)
    mixed = calc_sliced_wasserstein_shares(x.astype(np.float16), y, projections=16, seed=4)       # mixed dtypes go to float32
    assert _same_bits(mixed["share_y"], calc_sliced_wasserstein_shares(x.astype(np.float16).astype(np.float32), y, projections=16,
                                                                       seed=4)["share_y"])
    own = calc_sliced_wasserstein_shares(_dev(x, "fp32"), _dev(y, "fp32"), directions=sliced_directions(64, 16, 4))
    assert _same_bits(own["share_x"], res["share_x"]) and own["seed"] is None


# ----------------------------------------------------------------------------------------------------- (f) exact cases
def _exact_check(got, x, y, t, tag):
    want = SS.shares(x, y, t, "fp32", ordered=True)
    assert np.array_equal(got["index_x"], want["index_x"]) and np.array_equal(got["index_y"], want["index_y"]), tag
    assert _same_bits(got["share_x"], want["share_x"]), (tag, got["share_x"], want["share_x"])
    assert _same_bits(got["share_y"], want["share_y"]), (tag, got["share_y"], want["share_y"])
    _check_sums(got, tag)


@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("n,m,d,L", EXACT_SHAPES)
def test_exact_rows_bit_for_bit(n, m, d, L, dt):
    x, y = SR.exact_rows(n, m, d)
    t = SR.exact_directions(L, d)
    got = _run(x, y, t, dt)
    _exact_check(got, x, y, t, f"exact {n}x{m}x{d} L={L} {dt}")
    if dt == "fp16":
        _same_result(got, _plain(x, y, t, dt), "exact")


def test_exact_rows_at_size():
    from fadtk_amd import hip
    n, m, d, L = 70001, 33333, 16, 8
    x, y = SR.exact_rows(n, m, d)
    t = SR.exact_directions(L, d)
    got = _run(x, y, t, "fp16")
    assert hip.sliced_last_plan() == {"chunks": 1, "directions_per_chunk": 8, "sort_passes": 4, "share": 35}
    _exact_check(got, x, y, t, "exact at size")
    _same_result(got, _plain(x, y, t, "fp16"), "exact at size")
    swapped = _run(y, x, t, "fp16")
    assert hip.sliced_last_plan()["share"] == 17
    assert _same_bits(swapped["share_x"], got["share_y"]) and _same_bits(swapped["share_y"], got["share_x"])
    assert _same_bits(swapped["index_x"], got["index_y"])


# ----------------------------------------------------------------------------------------------------- the sort's edges
@pytest.mark.parametrize("n,L,share", ((2047, 2, 1), (2048, 2, 1), (2049, 2, 2), (4100, 3, 3), (100, 20, -8), (256, 3, -3), (257, 3, 1)))
def test_sort_edges(n, L, share):
    from fadtk_amd import hip
    m, d = 300, 8
    x, y = SR.exact_rows(n, m, d, seed=1)
    t = SR.exact_directions(L, d, seed=1)
    got = _run(x, y, t, "fp16")
    plan = hip.sliced_last_plan()
    assert plan["share"] == share and plan["sort_passes"] == 4 and plan["chunks"] == 1 and plan["directions_per_chunk"] == L
    _exact_check(got, x, y, t, f"sort edge n={n} L={L}")
    xr, yr, tr = _case(n, m, d, L, "fp32")
    _check(_run(xr, yr, tr, "fp32"), _plain(xr, yr, tr, "fp32"), xr, yr, tr, "fp32", f"sort edge n={n} L={L} normal rows")


# ----------------------------------------------------------------------------------------------------- special inputs
def test_repeated_rows_and_a_zero_row():
    x, y = SR.exact_rows(300, 257, 16, seed=4)
    x[17] = 0
    x[100:200] = x[:100]                                                               # every row of the first hundred twice: ties in every direction
    y[5] = y[200]
    t = SR.exact_directions(3, 16)
    got = _run(x, y, t, "bf16")
    _exact_check(got, x, y, t, "repeated rows")
    _check_match(got, SR.direction_norms(t), "repeated rows")
    first = np.argsort(got["index_x"], axis=1)                                         # the rank of every row
    assert np.all(first[:, 100:200] > first[:, :100])                                  # a copy stands behind its original
    same = np.repeat(SR.exact_rows(1, 1, 16)[0], 300, axis=0)                          # all rows identical: the identity
    got = _run(same, y, t, "fp16")
    assert np.array_equal(got["index_x"], np.broadcast_to(np.arange(300, dtype=np.int32), (3, 300)))
    _exact_check(got, same, y, t, "identical rows")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_identical_sets_give_zero_shares(dt):
    x, _, t = _case(255, 257, 128, 33, dt)
    got = _run(x, x.copy(), t, dt)
    assert np.all(got["share_x"] == 0) and np.all(got["share_y"] == 0) and got["sw2_squared"] == 0
    assert _same_bits(got["index_x"], got["index_y"])


@pytest.mark.parametrize("dt,e", (("fp16", 3), ("bf16", -20), ("fp32", 40)))
def test_scaling_by_a_power_of_two(dt, e):
    x, y, t = _case(257, 130, 64, 5, dt)
    x, y = x * np.float32(0.25), y * np.float32(0.25)                                  # away from float16's limits
    x, y = SR.round_to_dtype(x, dt), SR.round_to_dtype(y, dt)
    one = _run(x, y, t, dt)
    s = np.float32(2.0 ** e)
    two = _run(x * s, y * s, t, dt)
    assert _same_bits(two["share_x"], one["share_x"] * 4.0 ** e) and _same_bits(two["share_y"], one["share_y"] * 4.0 ** e)
    assert _same_bits(two["index_x"], one["index_x"]) and _same_bits(two["index_y"], one["index_y"])


# ----------------------------------------------------------------------------------------------------- repeatability, symmetry, chunks
KEYS = ("share_x", "share_y", "index_x", "index_y", "values", "sorted_x", "sorted_y")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_same_bits_again_swapped_and_in_chunks(dt, monkeypatch):
    from fadtk_amd import hip
    x, y, t = _case(255, 257, 128, 33, dt)
    one = _run(x, y, t, dt)
    assert hip.sliced_last_plan()["chunks"] == 1
    two = _run(x, y, t, dt)
    for k in KEYS:
        assert _same_bits(one[k], two[k]), k
    swapped = _run(y, x, t, dt)
    assert _same_bits(swapped["share_x"], one["share_y"]) and _same_bits(swapped["share_y"], one["share_x"])
    assert _same_bits(swapped["index_x"], one["index_y"]) and swapped["sw2_squared"] == one["sw2_squared"]
    monkeypatch.setenv("FAD_SLICED_WORKSPACE", "170000")                               # 15 376 bytes per direction here: 11 per chunk
    cut = _run(x, y, t, dt)
    plan = hip.sliced_last_plan()
    assert plan["chunks"] == 3 and plan["directions_per_chunk"] == 11
    for k in KEYS:
        assert _same_bits(one[k], cut[k]), k
    assert cut["sw2_squared"] == one["sw2_squared"] and cut["max_index"] == one["max_index"]
    monkeypatch.setenv("FAD_SLICED_WORKSPACE", "1")                                    # never less than one direction per chunk
    single = _run(x, y, t, dt)
    assert hip.sliced_last_plan()["chunks"] == 33
    for k in KEYS:
        assert _same_bits(one[k], single[k]), k


def test_equal_sizes_swapped():
    x, y, t = _case(129, 127, 2047, 2, "fp16")
    y2 = np.concatenate([y, y[:2]])
    one, two = _run(x, y2, t, "fp16"), _run(y2, x, t, "fp16")
    assert _same_bits(one["share_x"], two["share_y"]) and _same_bits(one["share_y"], two["share_x"])
    assert _same_bits(one["values"], two["values"]) and _same_bits(one["index_x"], two["index_y"])
    _check_match(one, SR.direction_norms(SR.round_to_dtype(t, "fp16")), "equal sizes")


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(130, 70, 37, "fp32")
    t = SR.directions(4, 37)
    res = _capi.FadSlicedResult()
    res.sw2_squared, res.max_index = -7.0, 99
    vals, sx, sy = np.full(4, -7.0), np.full((4, 130), -7.0, np.float32), np.full((4, 70), -7.0, np.float32)
    ix, iy = np.full((4, 130), -7, np.int32), np.full((4, 70), -7, np.int32)
    shx, shy = np.full(130, -7.0), np.full(70, -7.0)
    det = _capi.FadSlicedSharesDetail(vals.ctypes.data, sx.ctypes.data, sy.ctypes.data, ix.ctypes.data, iy.ctypes.data)

    def call(xa=x, ya=y, n=130, m=70, d=37, dt=_capi.FAD_F32, th=t, L=4, out=C.byref(res), ld=37, a=shx, b=shy):
        return lib.fad_sliced_shares(xa.ctypes.data, n, ld, ya.ctypes.data, m, ld, d, dt, 0, th.ctypes.data if th is not None else None, L,
                                     out, a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None,
                                     C.byref(det), 0, None)
    assert call(dt=_capi.FAD_F64) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID and call(ld=36) == INVALID
    assert call(L=0) == INVALID and call(L=65537) == INVALID
    assert call(out=None) == INVALID and call(th=None) == INVALID and call(a=None) == INVALID and call(b=None) == INVALID
    assert call(n=0) == TOO_FEW and call(m=0) == TOO_FEW
    assert call(n=2 ** 27, m=2 ** 26) == INVALID
    for bad in (np.nan, -np.inf):
        tb = t.copy()
        tb[3, 36] = bad
        assert call(th=tb) == INVALID
    tz = t.copy()
    tz[2] = 0
    assert call(th=tz) == INVALID
    tz[2, 0] = 70000.0
    assert call(th=tz, dt=_capi.FAD_F16) == INVALID                                    # infinite once rounded to float16
    bad_rows = y.copy()
    bad_rows[69, 36] = np.inf
    assert call(ya=bad_rows) == NOT_FINITE
    bad_rows[69, 36] = np.nan
    assert call(xa=np.concatenate([bad_rows, bad_rows]), n=130) == NOT_FINITE
    big = np.full((130, 37), 1e18, np.float32)                                         # finite norms, projections beyond float32
    tb = t.copy()
    tb[3] = 1e25
    assert call(xa=big, th=tb) == NOT_FINITE
    assert res.sw2_squared == -7.0 and res.max_index == 99
    assert np.all(vals == -7.0) and np.all(sx == -7.0) and np.all(sy == -7.0) and np.all(ix == -7) and np.all(iy == -7)
    assert np.all(shx == -7.0) and np.all(shy == -7.0)
    assert call() == 0 and res.sw2_squared > 0 and np.all(vals > 0) and np.all(sx != -7.0) and np.all(sy != -7.0)
    assert np.all(ix >= 0) and np.all(iy >= 0) and np.all(shx >= 0) and np.all(shy >= 0)


# ----------------------------------------------------------------------------------------------------- the command line
def test_command_line_on_two_cached_directories(tmp_path):
    from fadtk_amd import calc_sliced_wasserstein_shares, sliced
    rng = np.random.default_rng(3)
    base, evl = tmp_path / "base", tmp_path / "evl"
    sizes = {base: (40, 41, 42), evl: (25, 31, 1)}
    for d, shift in ((base, 0.0), (evl, 0.5)):
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i, rows in enumerate(sizes[d]):
            (d / f"f{i}.wav").write_bytes(b"")                  # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"f{i}.npy", (rng.standard_normal((rows, 128)) + shift * (i + 1)).astype(np.float32))
    foreign = tmp_path / "sliced.csv"
    foreign.write_text(sliced.CSV_HEADER)
    with pytest.raises(ValueError, match="another file"):
        sliced.main(["vggish", str(base), str(evl), str(foreign), "--shares", "--projections", "16", "--seed", "2", "-w", "2"])
    assert foreign.read_text() == sliced.CSV_HEADER
    csv = tmp_path / "out" / "shares.csv"
    sliced.main(["vggish", str(base), str(evl), str(csv), "--shares", "--projections", "16", "--seed", "2", "-w", "2"])
    lines = csv.read_text().splitlines()
    assert lines[0] + "\n" == sliced.SHARES_CSV_HEADER and len(lines) == 7
    cells = [dict(zip(sliced.SHARES_CSV_HEADER.strip().split(","), ln.split(","))) for ln in lines[1:]]
    assert [c["side"] for c in cells] == ["baseline"] * 3 + ["eval"] * 3
    x = np.concatenate([np.load(base / "embeddings" / "vggish" / f"f{i}.npy") for i in range(3)])
    y = np.concatenate([np.load(evl / "embeddings" / "vggish" / f"f{i}.npy") for i in range(3)])
    want = calc_sliced_wasserstein_shares(x, y, projections=16, seed=2, x_offsets=[0, 40, 81, 123], y_offsets=[0, 25, 56, 57])
    for side, d, rows, k in (("baseline", base, 123, "x"), ("eval", evl, 57, "y")):
        mine = [c for c in cells if c["side"] == side]
        shares = [float(c["share"]) for c in mine]
        assert shares == sorted(shares, reverse=True)
        assert sorted(c["file"] for c in mine) == sorted(str(d / f"f{i}.wav") for i in range(3))
        for c in mine:
            i = int(c["file"][-5])
            assert int(c["rows"]) == sizes[d][i] and c["share"] == repr(float(want[f"file_share_{k}"][i]))
            assert c["lift"] == repr(float(want[f"file_lift_{k}"][i]))
            assert float(c["fraction"]) == float(c["share"]) / want["sw2_squared"]
        assert abs(sum(float(c["fraction"]) for c in mine) - 1.0) <= (rows + 16 + 8) * 2.0 ** -52
