"""The sliced Wasserstein distance on the GPU (fad_sliced_wasserstein; csrc/kad.hip and csrc/sliced_sort.h) against the
float64 reference of tests/sliced_reference.py, stage by stage -- an end-to-end tolerance alone is too loose to see a wrong weight:

(a) projections, through sorted_x / sorted_y: non-decreasing, and elementwise within delta of np.sort of the float64 projections
    (sorting is 1-Lipschitz in the sup norm); delta = gamma_k max_i sum_d |x_id theta_ld|, gamma_k = k u / (1 - k u), u = 2^-23 (one ulp,
    not half: DESIGN 4.16 measured that the matrix cores' sum inside a k step is not plain round-to-nearest), k = D for 16-bit rows
    (exact products) and D + 1 for float32 rows.  Derived, computed per case, never taken from a GPU figure.
(b) the match: W_l recomputed on the host in float64 by the reference's formula FROM THE RETURNED sorted float32 arrays and q_l equals
    values[l] to a relative (n + m) 2^-52 (float64 summation order only) -- what catches a wrong weight or a lost interval at n != m --
    and, summed in the order the library documents, to the last bit.
(c) end to end: |W_l - reference| <= (2 sqrt(W_ref q_l) delta' + delta'^2) / q_l, delta' = delta_x + delta_y; sw2_squared, std_error,
    max_sliced and max_index follow from values exactly as the reference forms them.
(d) exact cases: rows (integers in [-8, 8]) x 2^e_i, integer directions: every projection is exact, so both sorted arrays equal the
    reference bit for bit, and values equal the reference summed in the documented order bit for bit.  (With row exponents from -8 to 8
    the float64 partial sums of S are NOT all exact integers -- at 70 001 x 33 333 rows S is near 2^58 units of 2^-16 -- so a reference in
    another summation order differs in the last bits; where S stays below 2^52 units the plain-order reference is asserted too.)

Measured on an MI355X over this file's cases (the [sliced-err] lines, profiles/sliced_gpu_tail.txt): the worst projection error is
0.14 delta, the worst value error 0.05 of its bound.  No bound here comes from those figures.

The sort's own edges are read from fad_sliced_last_plan, so a test asserts that it hit them: a segment of one workgroup's share - 1, the
share and the share + 1 (2047, 2048, 2049 keys), three workgroups per segment (4100), several segments per workgroup (100 keys)."""
import ctypes as C
import functools

import numpy as np
import pytest

import sliced_reference as SR

pytestmark = pytest.mark.gpu
TOO_FEW, NOT_FINITE, INVALID = -6, -7, -1
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16", "fp32": "float32"}
SHAPES = ((1, 1, 5, 1), (1, 300, 37, 3), (300, 1, 37, 3), (2, 3, 1, 2), (255, 257, 128, 33), (257, 130, 64, 5), (129, 127, 2047, 2))
EXACT_SHAPES = ((1, 300, 37, 3), (2, 3, 1, 2), (255, 257, 128, 33), (257, 130, 64, 5), (129, 127, 2047, 2))


def _dev(a, dt, ld=None):
    """float32 values -> a torch CUDA tensor of dtype dt; with ld, a view of a wider buffer (row pitch ld > D) whose pitch entries are 7"""
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, TORCH_DT[dt]))
    if ld is None:
        return t
    wide = torch.full((t.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _run(x, y, t, dt, ldx=None, host=False):
    from fadtk_amd import hip
    if host:
        npdt = {"fp16": np.float16, "fp32": np.float32}[dt]
        xs, ys = x.astype(npdt), y.astype(npdt)
    else:
        xs, ys = _dev(x, dt, ldx), _dev(y, dt)
    return hip.sliced_wasserstein(xs, ys, t, values=True, sorted_projections=True)


@functools.lru_cache(maxsize=None)
def _case(n, m, d, L, dt):
    x, y = SR.rows(n, m, d, dt)
    t = SR.directions(L, d)
    return x, y, t, SR.sliced(x, y, t, dt)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_statistics(got):
    mean, se, mx, k = SR.statistics(got["values"])
    assert got["sw2_squared"] == mean and got["max_sliced"] == mx and got["max_index"] == k
    assert (np.isnan(se) and np.isnan(got["std_error"])) if len(got["values"]) == 1 else got["std_error"] == se


def _check(got, x, y, t, dt, want, tag):
    n, m = len(x), len(y)
    tr = SR.round_to_dtype(t, dt)
    q = want["q"]
    assert got["n"] == n and got["m"] == m and got["projections"] == len(t)
    # (a)
    dx, dy = SR.projection_bound(x, tr, dt), SR.projection_bound(y, tr, dt)
    for k, delta in (("sorted_x", dx), ("sorted_y", dy)):
        s = got[k]
        assert s.dtype == np.float32 and np.all(np.isfinite(s)) and np.all(np.diff(s, axis=1) >= 0), (tag, k)
        err = np.abs(s.astype(np.float64) - want[k]).max(axis=1)
        print(f"[sliced-err] {tag} {k}: worst error / delta {float((err / np.maximum(delta, 1e-300)).max()):.3f}")
        assert np.all(err <= delta), (tag, k, err, delta)
    # (b)
    sa, sb = got["sorted_x"].astype(np.float64), got["sorted_y"].astype(np.float64)
    host = SR.values_from_sorted(sa, sb, q)
    assert np.all(np.abs(got["values"] - host) <= (n + m) * 2.0 ** -52 * host), (tag, got["values"], host)
    assert _same_bits(got["values"], SR.values_from_sorted(sa, sb, q, ordered=True)), tag
    # (c)
    bound = SR.value_bound(want["values"], q, dx, dy)
    print(f"[sliced-err] {tag} values: worst error / bound {float((np.abs(got['values'] - want['values']) / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(np.abs(got["values"] - want["values"]) <= bound), (tag, got["values"], want["values"], bound)
    _check_statistics(got)


# ----------------------------------------------------------------------------------------------------- (a), (b), (c)
@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("n,m,d,L", SHAPES)
def test_against_reference(n, m, d, L, dt):
    x, y, t, want = _case(n, m, d, L, dt)
    got = _run(x, y, t, dt, ldx=d + 3 if (n, m) in ((255, 257), (1, 300), (2, 3)) else None)
    _check(got, x, y, t, dt, want, f"{n}x{m}x{d} L={L} {dt}")


@pytest.mark.parametrize("dt", ("fp16", "fp32"))
def test_host_rows(dt):
    x, y, t, want = _case(257, 130, 64, 5, dt)
    got = _run(x, y, t, dt, host=True)
    _check(got, x, y, t, dt, want, f"host rows {dt}")
    assert _same_bits(got["values"], _run(x, y, t, dt)["values"])


def test_python_layer():
    from fadtk_amd import calc_sliced_wasserstein, sliced_directions
    x, y, _, _ = _case(257, 130, 64, 5, "fp32")
    res = calc_sliced_wasserstein(x, y, projections=16, seed=4, per_direction=True)
    want = SR.sliced(x, y, sliced_directions(64, 16, 4), "fp32")
    assert abs(res["sw2_squared"] - want["sw2_squared"]) <= 1e-4 * want["sw2_squared"] and res["values"].shape == (16,)
    assert res["sliced_w2"] == np.sqrt(res["sw2_squared"]) and res["fad_scale"] == 64 * res["sw2_squared"]
    assert (res["n"], res["m"], res["projections"], res["seed"]) == (257, 130, 16, 4)
    mixed = calc_sliced_wasserstein(x.astype(np.float16), y, projections=16, seed=4)      # mixed dtypes go to float32
    assert mixed["sw2_squared"] == calc_sliced_wasserstein(x.astype(np.float16).astype(np.float32), y, projections=16, seed=4)["sw2_squared"]
    own = calc_sliced_wasserstein(_dev(x, "fp32"), _dev(y, "fp32"), directions=sliced_directions(64, 16, 4))
    assert own["sw2_squared"] == res["sw2_squared"] and own["seed"] is None


# ----------------------------------------------------------------------------------------------------- (d) exact cases
def _exact_check(got, x, y, t, tag):
    want = SR.sliced(x, y, t, "fp32", ordered=True)
    assert _same_bits(got["sorted_x"], want["sorted_x"].astype(np.float32)), tag
    assert _same_bits(got["sorted_y"], want["sorted_y"].astype(np.float32)), tag
    assert np.array_equal(want["sorted_x"], want["sorted_x"].astype(np.float32).astype(np.float64))        # the projections are exact
    assert _same_bits(got["values"], want["values"]), (tag, got["values"], want["values"])
    plain = SR.sliced(x, y, t, "fp32")["values"]
    S = plain * want["q"] * float(len(x) * len(y))
    small = S * 2.0 ** 16 < 2.0 ** 52            # every term and partial sum is then an exact integer in units of 2^-16
    assert np.array_equal(got["values"][small], plain[small]), tag
    _check_statistics(got)
    return int(small.sum())


@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("n,m,d,L", EXACT_SHAPES)
def test_exact_rows_bit_for_bit(n, m, d, L, dt):
    x, y = SR.exact_rows(n, m, d)
    t = SR.exact_directions(L, d)
    _exact_check(_run(x, y, t, dt), x, y, t, f"exact {n}x{m}x{d} L={L} {dt}")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_small_integer_rows_equal_the_plain_reference(dt):
    """integers proper (no row exponents): S is an exact integer below 2^53, so any summation order gives the reference's bits"""
    rng = np.random.default_rng(5)
    x, y = rng.integers(-8, 9, (257, 64)).astype(np.float32), rng.integers(-8, 9, (130, 64)).astype(np.float32)
    t = SR.exact_directions(5, 64)
    got = _run(x, y, t, dt)
    assert _exact_check(got, x, y, t, f"integers {dt}") == 5


def test_exact_rows_at_size():
    from fadtk_amd import hip
    n, m, d, L = 70001, 33333, 16, 8
    x, y = SR.exact_rows(n, m, d)
    t = SR.exact_directions(L, d)
    got = _run(x, y, t, "fp16")
    plan = hip.sliced_last_plan()
    assert plan == {"chunks": 1, "directions_per_chunk": 8, "sort_passes": 4, "share": 35}
    _exact_check(got, x, y, t, "exact at size")
    swapped = _run(y, x, t, "fp16")
    assert hip.sliced_last_plan()["share"] == 17 and _same_bits(swapped["values"], got["values"])
    assert _same_bits(swapped["sorted_x"], got["sorted_y"])


# ----------------------------------------------------------------------------------------------------- the sort's edges
@pytest.mark.parametrize("n,L,share", ((2047, 2, 1), (2048, 2, 1), (2049, 2, 2), (4100, 3, 3), (100, 5, -5), (100, 20, -8), (256, 3, -3),
                                      (257, 3, 1)))
def test_sort_edges(n, L, share):
    from fadtk_amd import hip
    m, d = 300, 8
    x, y = SR.exact_rows(n, m, d, seed=1)
    t = SR.exact_directions(L, d, seed=1)
    got = _run(x, y, t, "fp16")
    plan = hip.sliced_last_plan()
    assert plan["share"] == share and plan["sort_passes"] == 4 and plan["chunks"] == 1 and plan["directions_per_chunk"] == L
    _exact_check(got, x, y, t, f"sort edge n={n} L={L}")
    xr, yr, tr, want = _case(n, m, d, L, "fp32")
    _check(_run(xr, yr, tr, "fp32"), xr, yr, tr, "fp32", want, f"sort edge n={n} L={L} normal rows")


# ----------------------------------------------------------------------------------------------------- special inputs
def _e0(L, d, seed=2):
    t = SR.exact_directions(L, d, seed=seed)
    t[0] = 0
    t[0, 0] = 1.0
    return t


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_all_rows_identical(dt):
    row = SR.exact_rows(1, 1, 37)[0]
    x, y = np.repeat(row, 300, axis=0), np.repeat(row * 2, 257, axis=0)
    t = SR.exact_directions(4, 37)
    got = _run(x, y, t, dt)
    _exact_check(got, x, y, t, "identical rows")
    assert np.all(got["sorted_x"] == got["sorted_x"][:, :1])                           # every key of a segment equal
    p = (row.astype(np.float64) @ t.T.astype(np.float64))[0]
    assert np.array_equal(got["values"], p * p / SR.direction_norms(t))                # (p - 2 p)^2 / q


def test_sorted_against_reversed():
    n = 2500
    x, y = SR.exact_rows(n, n, 8, seed=3)
    x, y = x[np.argsort(x[:, 0], kind="stable")], y[np.argsort(-y[:, 0], kind="stable")]
    t = _e0(3, 8)
    got = _run(x, y, t, "fp32")
    assert np.array_equal(got["sorted_x"][0], x[:, 0]) and np.array_equal(got["sorted_y"][0], y[::-1, 0])
    _exact_check(got, x, y, t, "sorted against reversed")


def test_zero_row_and_two_valued_columns():
    rng = np.random.default_rng(9)
    x, y = SR.exact_rows(300, 257, 16, seed=4)
    x[17] = 0
    got = _run(x, y, SR.exact_directions(3, 16), "bf16")
    _exact_check(got, x, y, SR.exact_directions(3, 16), "zero row")
    x2 = np.where(rng.random((2100, 16)) < 0.5, -0.0, 3.0).astype(np.float32)           # -0 and 3: the keys take two or three values
    y2 = np.where(rng.random((300, 16)) < 0.3, 1.0, -2.0).astype(np.float32)
    t = _e0(2, 16)
    got = _run(x2, y2, t, "fp16")
    _exact_check(got, x2, y2, t, "two-valued columns")
    assert set(np.unique(got["sorted_x"][0])) == {0.0, 3.0} and set(np.unique(got["sorted_y"][0])) == {-2.0, 1.0}


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_identical_sets_give_zero_and_translation_is_exact(dt):
    x, _, _, _ = _case(255, 257, 128, 33, dt)
    t = SR.directions(33, 128)
    got = _run(x, x.copy(), t, dt)
    assert np.all(got["values"] == 0) and got["sw2_squared"] == 0 and got["std_error"] == 0 and got["max_index"] == 0
    xi = np.random.default_rng(6).integers(-8, 9, (300, 16)).astype(np.float32)
    yi = xi.copy()
    yi[:, 0] += 4.0                                                                    # c = 4: W_0 = c^2 exactly along e_0
    got = _run(xi, yi, _e0(3, 16), dt)
    assert got["values"][0] == 16.0


@pytest.mark.parametrize("dt,e", (("fp16", 3), ("bf16", -20), ("fp32", 40)))
def test_scaling_by_a_power_of_two(dt, e):
    x, y, t, _ = _case(257, 130, 64, 5, dt)
    x, y = x * np.float32(0.25), y * np.float32(0.25)                                  # away from float16's limits
    x, y = SR.round_to_dtype(x, dt), SR.round_to_dtype(y, dt)
    one = _run(x, y, t, dt)
    s = np.float32(2.0 ** e)
    two = _run(x * s, y * s, t, dt)
    assert _same_bits(two["values"], one["values"] * 4.0 ** e) and _same_bits(two["sorted_x"], one["sorted_x"] * s)


# ----------------------------------------------------------------------------------------------------- repeatability, symmetry, chunks
@pytest.mark.parametrize("dt", SR.DTYPES)
def test_same_bits_again_swapped_and_in_chunks(dt, monkeypatch):
    from fadtk_amd import hip
    x, y, t, _ = _case(255, 257, 128, 33, dt)
    one = _run(x, y, t, dt)
    assert hip.sliced_last_plan()["chunks"] == 1
    two = _run(x, y, t, dt)
    for k in ("values", "sorted_x", "sorted_y"):
        assert _same_bits(one[k], two[k]), k
    swapped = _run(y, x, t, dt)
    assert _same_bits(swapped["values"], one["values"]) and _same_bits(swapped["sorted_x"], one["sorted_y"])
    assert swapped["sw2_squared"] == one["sw2_squared"] and swapped["std_error"] == one["std_error"]
    monkeypatch.setenv("FAD_SLICED_WORKSPACE", "70000")                                # 6160 bytes per direction here: 11 per chunk
    cut = _run(x, y, t, dt)
    plan = hip.sliced_last_plan()
    assert plan["chunks"] >= 3 and plan["chunks"] * plan["directions_per_chunk"] >= 33 > (plan["chunks"] - 1) * plan["directions_per_chunk"]
    for k in ("values", "sorted_x", "sorted_y"):
        assert _same_bits(one[k], cut[k]), k
    assert cut["sw2_squared"] == one["sw2_squared"] and cut["max_index"] == one["max_index"]
    monkeypatch.setenv("FAD_SLICED_WORKSPACE", "1")                                    # never less than one direction per chunk
    assert _same_bits(_run(x, y, t, dt)["values"], one["values"]) and hip.sliced_last_plan()["chunks"] == 33


def test_equal_sizes_swapped():
    x, y, t, _ = _case(129, 127, 2047, 2, "fp16")
    y2 = np.concatenate([y, y[:2]])
    one, two = _run(x, y2, t, "fp16"), _run(y2, x, t, "fp16")
    assert _same_bits(one["values"], two["values"])


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(130, 70, 37, "fp32")
    t = SR.directions(4, 37)
    res = _capi.FadSlicedResult()
    res.sw2_squared, res.max_index = -7.0, 99
    vals, sx, sy = np.full(4, -7.0), np.full((4, 130), -7.0, np.float32), np.full((4, 70), -7.0, np.float32)
    det = _capi.FadSlicedDetail(vals.ctypes.data, sx.ctypes.data, sy.ctypes.data)

    def call(xa=x, ya=y, n=130, m=70, d=37, dt=_capi.FAD_F32, th=t, L=4, out=C.byref(res), ld=37):
        return lib.fad_sliced_wasserstein(xa.ctypes.data, n, ld, ya.ctypes.data, m, ld, d, dt, 0, th.ctypes.data if th is not None else None, L,
                                          out, C.byref(det), 0, None)
    assert call(dt=_capi.FAD_F64) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID and call(ld=36) == INVALID
    assert call(L=0) == INVALID and call(L=65537) == INVALID
    assert call(out=None) == INVALID and call(th=None) == INVALID
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
    assert np.all(vals == -7.0) and np.all(sx == -7.0) and np.all(sy == -7.0)
    assert call() == 0 and res.sw2_squared > 0 and np.all(vals > 0) and np.all(sx != -7.0) and np.all(sy != -7.0)


# ----------------------------------------------------------------------------------------------------- the command line
def test_command_line_on_two_cached_directories(tmp_path, capsys):
    from fadtk_amd import SlicedWasserstein, calc_sliced_wasserstein, sliced
    from fadtk_amd.model_loader import get_all_models
    rng = np.random.default_rng(3)
    base, evl = tmp_path / "base", tmp_path / "evl"
    for d, sizes, shift in ((base, (40, 41, 42), 0.0), (evl, (25, 31, 1), 0.5)):
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i, rows in enumerate(sizes):
            (d / f"f{i}.wav").write_bytes(b"")                  # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"f{i}.npy", (rng.standard_normal((rows, 128)) + shift).astype(np.float32))
    csv = tmp_path / "out" / "sliced.csv"
    for _ in range(2):
        sliced.main(["vggish", str(base), str(evl), str(csv), "--projections", "16", "--seed", "2", "-w", "2"])
    printed = capsys.readouterr().out.split()
    lines = csv.read_text().splitlines()
    assert lines[0] + "\n" == sliced.CSV_HEADER and len(lines) == 3 and lines[1] == lines[2]
    cells = dict(zip(sliced.CSV_HEADER.strip().split(","), lines[1].split(",")))
    assert (cells["model"], cells["n"], cells["m"], cells["projections"], cells["seed"]) == ("vggish", "123", "57", "16", "2")
    assert printed[-1] == cells["sw2_squared"]
    ml = {m.name: m for m in get_all_models()}["vggish"]
    res = SlicedWasserstein(ml, audio_load_worker=2, projections=16, seed=2).score(base, evl)
    assert repr(res["sw2_squared"]) == cells["sw2_squared"] and repr(res["fad_scale"]) == cells["fad_scale"]
    x = np.concatenate([np.load(base / "embeddings" / "vggish" / (f.stem + ".npy")) for f in base.glob("*.*")])
    y = np.concatenate([np.load(evl / "embeddings" / "vggish" / (f.stem + ".npy")) for f in evl.glob("*.*")])
    whole = calc_sliced_wasserstein(x, y, projections=16, seed=2)
    assert whole["sw2_squared"] == res["sw2_squared"]           # the sorted projections do not depend on the order of the rows
    want = SR.sliced(x, y, sliced.sliced_directions(128, 16, 2), "fp32")
    assert abs(res["sw2_squared"] - want["sw2_squared"]) <= 1e-4 * want["sw2_squared"]
