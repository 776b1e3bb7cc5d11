"""The polynomial-kernel distance on the GPU (fad_kid, fad_kid_subsets; csrc/kad.hip) against the float64 reference of
tests/kid_reference.py on the same values, upcast: an integer fixture on which every sum is exact (any padding contribution, diagonal
slip, gather error or unit-map error shows as a wrong bit), Gaussian rows within max(4e-7, 4 A_poly) of float64, the subsets against the
full sets, determinism, the groups through the workspace, the refusals, and the Python layer.  The shapes are the smallest that reach a
diagonal tile, an off-diagonal tile, a padding row, a ragged k step and a second group."""
import ctypes as C
import functools

import numpy as np
import pytest

import kid_reference as KR

pytestmark = pytest.mark.gpu
TOO_FEW, NOT_FINITE, INVALID = -6, -7, -1
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16", "fp32": "float32"}


def _dev(a, dt, ld=None):
    """float32 values -> a torch CUDA tensor of dtype dt; with ld, a view of a wider zero-filled buffer (row pitch ld > D)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(getattr(torch, TORCH_DT[dt]))
    if ld is None:
        return t
    wide = torch.full((t.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")             # the pitch bytes are not zeros: never read
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _exact_dev(dt):
    x, y = KR.exact_rows()
    return _dev(x, dt, KR.EXACT_LD), _dev(y, dt, KR.EXACT_LD)


def _scale(want_terms):
    return float(np.abs(want_terms).sum(axis=-1).max())


# ---------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("dt", KR.DTYPES)
@pytest.mark.parametrize("subsets", KR.EXACT_SUBSETS)
@pytest.mark.parametrize("s", KR.EXACT_SIZES)
def test_subsets_exact_on_integer_rows(s, subsets, dt):
    """Every Sxx, Syy, Sxy equals the float64 reference exactly (the means are the exact sums over exact counts, formed alike)."""
    from fadtk_amd import hip
    x, y = KR.exact_rows()
    xd, yd = _exact_dev(dt)
    assert xd.stride(0) == KR.EXACT_LD > KR.EXACT_D
    ix, iy = KR.exact_indices(KR.EXACT_N, KR.EXACT_M, subsets, s, seed=s + subsets)
    got = hip.kid_subsets(xd, yd, ix, iy)
    terms, mmd2, mean, std = KR.subset_stats(KR.kid_subsets(x, y, ix, iy), s)
    assert got["subsets"] == subsets and got["subset_size"] == s
    assert np.array_equal(got["terms"], terms), np.abs(got["terms"] - terms).max()
    tol = 1e-14 * _scale(terms)
    assert np.abs(got["mmd2"] - mmd2).max() <= tol and abs(got["mean"] - mean) <= tol and abs(got["std"] - std) <= tol
    if subsets == 1:
        assert got["std"] == 0.0


@pytest.mark.parametrize("dt", KR.DTYPES)
@pytest.mark.parametrize("n,m", KR.EXACT_FULL)
def test_full_exact_on_integer_rows(n, m, dt):
    from fadtk_amd import hip
    x, y = KR.exact_rows()
    xd, yd = _exact_dev(dt)
    got = hip.kid(xd[:n], yd[:m])
    want = KR.kid_full(x[:n], y[:m])
    for k in KR.MEANS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["mmd2"] - want["mmd2"]) <= 1e-14 * (want["abs_kxx_mean"] + want["abs_kyy_mean"] + 2 * want["abs_kxy_mean"])
    assert got["gamma"] == 1.0 / 16 and got["coef0"] == 1.0 and got["degree"] == 3 and got["n"] == n and got["m"] == m


# ------------------------------------------------------------------------------------------------------------- Gaussian
def _check(got, want, tol, label):
    err = KR.mean_errors(got, want)
    print(f"[kid-err] {label}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()) + f" tol={tol:.2e}")
    for k in KR.MEANS + ("mmd2",):
        assert err[k] <= tol, (label, k, err[k], tol, got[k], want[k])


@pytest.mark.parametrize("dt", KR.DTYPES)
@pytest.mark.parametrize("d,off,degree", KR.GAUSS_CASES)
def test_gaussian_rows_against_float64(d, off, degree, dt):
    """Each mean within max(4e-7, 4 A_poly) of float64, relative to the mean of |k| of its block; MMD^2 within the same bound on
    |Kxx| + |Kyy| + 2 |Kxy|.  The full sets, and two subsets of 129 rows (a ragged second tile) through the gather."""
    from fadtk_amd import hip
    c = KR.gauss_case(d, off, degree, dt)
    tol = KR.gpu_tolerance(dt)
    xd, yd = _dev(c["x"], dt), _dev(c["y"], dt)
    _check(hip.kid(xd, yd, degree=degree), c["want"], tol, f"full {dt} D={d} off={off} degree={degree}")
    ix, iy = KR.exact_indices(KR.GAUSS_N, KR.GAUSS_M, 2, 129, seed=d + off)
    got = hip.kid_subsets(xd, yd, ix, iy, degree=degree)
    for q in range(2):
        want = KR.kid_full(c["x"][ix[q]], c["y"][iy[q]], degree)
        g = {"kxx_mean": got["terms"][q, 0], "kyy_mean": got["terms"][q, 1], "kxy_mean": got["terms"][q, 2], "mmd2": got["mmd2"][q]}
        _check(g, want, tol, f"subset {q} {dt} D={d} off={off} degree={degree}")


def test_degrees_one_and_four_and_explicit_parameters():
    from fadtk_amd import hip
    c = KR.gauss_case(17, 0, 2, "fp16")
    xd, yd = _dev(c["x"], "fp16"), _dev(c["y"], "fp16")
    for degree, gamma, coef0 in ((1, 0.3, 0.0), (4, None, 1.0), (3, 0.011, 2.5)):
        got = hip.kid(xd, yd, degree=degree, gamma=gamma, coef0=coef0)
        want = KR.kid_full(c["x"], c["y"], degree, gamma, coef0)
        assert got["gamma"] == want["gamma"] and got["coef0"] == want["coef0"] and got["degree"] == degree
        _check(got, want, KR.gpu_tolerance("fp16"), f"full fp16 D=17 degree={degree} gamma={gamma} coef0={coef0}")


# ---------------------------------------------------------------------------------------------------------- consistency
def test_identity_subset_is_the_full_set_and_calls_repeat():
    from fadtk_amd import hip
    c = KR.gauss_case(128, 4, 3, "bf16")
    n = 255
    xd, yd = _dev(c["x"], "bf16"), _dev(c["y"][:n], "bf16")
    full = hip.kid(xd, yd)
    ident = np.arange(n, dtype=np.int32)[None, :]
    ix, iy = KR.exact_indices(n, n, 5, n, seed=9)                      # subsets of all rows in other orders
    ix, iy = np.concatenate([ident, ix]), np.concatenate([ident, iy])
    a, b = hip.kid_subsets(xd, yd, ix, iy), hip.kid_subsets(xd, yd, ix, iy)
    for k in ("mmd2", "terms"):
        assert np.array_equal(a[k], b[k])                             # the same bits on every run
    assert a["mean"] == b["mean"] and a["std"] == b["std"]
    for j, k in enumerate(KR.MEANS):                                  # the walks are cut differently: float64 sums in another order
        assert a["terms"][0, j] == pytest.approx(full[k], rel=1e-14)
    assert abs(a["mmd2"][0] - full["mmd2"]) <= 1e-14 * np.abs(a["terms"][0]).sum()
    perm = np.array([3, 0, 5, 1, 4, 2])
    p = hip.kid_subsets(xd, yd, ix[perm], iy[perm])
    assert np.array_equal(p["mmd2"], a["mmd2"][perm]) and np.array_equal(p["terms"], a["terms"][perm])
    assert hip.kid(xd, yd) == full


def test_groups_do_not_show_in_the_result():
    """float32, D = 1280, s = 129: 51 subsets fill the entry point's 128 MiB of images (kid::plan, checked by kid_tiles_cover.cpp), so
    60 subsets go through the workspace in two groups; the same subsets in two calls split at the boundary give the same bits."""
    from fadtk_amd import hip
    d, s, S = 1280, 129, 60
    per_group = (128 << 20) // (2 * 256 * (d * 4 + 4))
    assert per_group == 51 < S
    rng = np.random.default_rng(60)
    x = rng.standard_normal((200, d)).astype(np.float32)
    y = (rng.standard_normal((190, d)) * 1.1 + 0.2).astype(np.float32)
    xd, yd = _dev(x, "fp32"), _dev(y, "fp32")
    ix, iy = KR.exact_indices(200, 190, S, s, seed=2)
    whole = hip.kid_subsets(xd, yd, ix, iy)
    first, second = hip.kid_subsets(xd, yd, ix[:per_group], iy[:per_group]), hip.kid_subsets(xd, yd, ix[per_group:], iy[per_group:])
    assert np.array_equal(whole["mmd2"], np.concatenate([first["mmd2"], second["mmd2"]]))
    assert np.array_equal(whole["terms"], np.concatenate([first["terms"], second["terms"]]))
    for q in (0, per_group - 1, per_group, S - 1):                    # and they are right on both sides of the boundary
        want = KR.kid_full(x[ix[q]], y[iy[q]])
        g = {"kxx_mean": whole["terms"][q, 0], "kyy_mean": whole["terms"][q, 1], "kxy_mean": whole["terms"][q, 2], "mmd2": whole["mmd2"][q]}
        _check(g, want, KR.gpu_tolerance("fp32"), f"group boundary, subset {q}")
    assert whole["mean"] == pytest.approx(whole["mmd2"].mean(), rel=1e-13) and whole["std"] == pytest.approx(whole["mmd2"].std(), rel=1e-10)


# ------------------------------------------------------------------------------------------------------------- refusals
SENTINEL = -12345.5


def _raw_subsets(x, y, ix, iy, s, subsets, degree=3, gamma=0.0, coef0=1.0, index_dev=None):
    """fad_kid_subsets through ctypes on host rows -> (status, outputs untouched?)"""
    from fadtk_amd import _capi
    lib = _capi.load_library()
    code = _capi.FAD_F32 if x.dtype == np.float32 else _capi.FAD_F16
    mmd2, terms = np.full(max(subsets, 1), SENTINEL), np.full((max(subsets, 1), 3), SENTINEL)
    mean, std = C.c_double(SENTINEL), C.c_double(SENTINEL)
    pix, piy, on_dev = (index_dev[0].data_ptr(), index_dev[1].data_ptr(), 1) if index_dev else (ix.ctypes.data, iy.ctypes.data, 0)
    st = lib.fad_kid_subsets(x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, y.shape[0], y.shape[1], x.shape[1], code, 0, degree, gamma,
                             coef0, pix, piy, subsets, s, on_dev, mmd2.ctypes.data, terms.ctypes.data, C.byref(mean), C.byref(std), 0, None)
    untouched = bool(np.all(mmd2 == SENTINEL) and np.all(terms == SENTINEL) and mean.value == SENTINEL and std.value == SENTINEL)
    return st, untouched


def test_refusals_leave_the_outputs_untouched():
    import torch
    from fadtk_amd import _capi
    rng = np.random.default_rng(4)
    n, m, d, s, S = 40, 30, 16, 10, 3
    x, y = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    ix, iy = KR.exact_indices(n, m, S, s, seed=1)
    assert _raw_subsets(x, y, ix, iy, s, S) == (0, False)              # the valid call writes every output

    def bad_index(which, value):
        jx, jy = ix.copy(), iy.copy()
        (jx if which == "x" else jy)[S - 1, s - 1] = value
        return jx, jy
    for which, value in (("x", n), ("y", m), ("x", -1), ("y", -1), ("x", 2 ** 31 - 1)):
        jx, jy = bad_index(which, value)
        assert _raw_subsets(x, y, jx, jy, s, S) == (INVALID, True), (which, value)
        dev = (torch.from_numpy(jx).cuda(), torch.from_numpy(jy).cuda())
        assert _raw_subsets(x, y, jx, jy, s, S, index_dev=dev) == (INVALID, True), (which, value, "device index")
    assert _raw_subsets(x, y, ix[:, :1].copy(), iy[:, :1].copy(), 1, S) == (TOO_FEW, True)
    big = np.zeros((S, m + 1), dtype=np.int32)
    assert _raw_subsets(x, y, big, big, m + 1, S) == (INVALID, True)                   # s > min(n, m)
    assert _raw_subsets(x, y, ix, iy, s, 0) == (INVALID, True)
    for degree in (0, 5):
        assert _raw_subsets(x, y, ix, iy, s, S, degree=degree) == (INVALID, True)
    for gamma, coef0 in ((float("nan"), 1.0), (float("inf"), 1.0), (0.0, float("nan")), (1e60, 1.0)):
        assert _raw_subsets(x, y, ix, iy, s, S, gamma=gamma, coef0=coef0) == (INVALID, True), (gamma, coef0)
    huge = np.full((n, d), 2.0 ** 30, dtype=np.float32)                               # u^3 = (2^60 + 1)^3 overflows float32
    assert _raw_subsets(huge, huge[:m], ix, iy, s, S) == (NOT_FINITE, True)
    assert _raw_subsets(huge, huge[:m], ix, iy, s, S, degree=1) == (0, False)          # degree 1 stays inside float32
    nan_row = x.copy()
    nan_row[ix[1, 2], 3] = np.nan
    assert _raw_subsets(nan_row, y, ix, iy, s, S) == (NOT_FINITE, True)
    inf_row = x.copy()
    inf_row[ix[0, 0], 0] = -np.inf                                                     # a dot product of -inf must not pass for padding
    assert _raw_subsets(inf_row, np.abs(y), ix, iy, s, S) == (NOT_FINITE, True)

    lib = _capi.load_library()
    res = _capi.FadKidResult()
    res.mmd2 = SENTINEL

    def full(a, b, degree=3, gamma=0.0, coef0=1.0):
        return lib.fad_kid(a.ctypes.data, a.shape[0], d, b.ctypes.data, b.shape[0], d, d, _capi.FAD_F32, 0, degree, gamma, coef0, C.byref(res), 0, None)
    assert full(x, y, degree=0) == INVALID and full(x, y, degree=5) == INVALID and full(x, y, gamma=float("nan")) == INVALID
    assert full(x[:1], y) == TOO_FEW and full(huge, huge[:m]) == NOT_FINITE and full(inf_row, np.abs(y)) == NOT_FINITE
    assert res.mmd2 == SENTINEL
    assert full(x, y) == 0 and res.mmd2 != SENTINEL


# --------------------------------------------------------------------------------------------------------------- Python
def test_python_layer_on_device_and_host_rows():
    import torch
    from fadtk_amd import calc_kernel_distance, calc_kernel_distance_full
    rng = np.random.default_rng(8)
    x = rng.standard_normal((150, 33)).astype(np.float16)
    y = (rng.standard_normal((140, 33)) * 1.2 + 0.1).astype(np.float16)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    a = calc_kernel_distance(x, y, subsets=4, subset_size=50, seed=3, return_indices=True)
    b = calc_kernel_distance(xd, yd, subsets=4, subset_size=50, seed=3)
    assert np.array_equal(a["values"], b["values"]) and a["kid_mean"] == b["kid_mean"] and a["kid_std"] == b["kid_std"]
    assert a["subsets"] == 4 and a["subset_size"] == 50 and a["degree"] == 3 and a["coef0"] == 1.0 and a["gamma"] == float(np.float32(1 / 33))
    assert a["kid_mean"] == pytest.approx(a["values"].mean(), rel=1e-13) and a["kid_std"] == pytest.approx(a["values"].std(), rel=1e-10)
    ix, iy = a["indices"]
    want = KR.subset_stats(KR.kid_subsets(x, y, ix, iy), 50)[1]
    assert np.abs(a["values"] - want).max() <= 4e-7 * 4
    other = calc_kernel_distance(x, y, subsets=4, subset_size=50, seed=4)
    assert not np.array_equal(other["values"], a["values"])
    given = calc_kernel_distance(xd, yd, seed=4, indices=(torch.from_numpy(ix).cuda(), torch.from_numpy(iy).cuda()))      # indices override the seed
    assert np.array_equal(given["values"], a["values"]) and given["subsets"] == 4 and given["subset_size"] == 50
    full = calc_kernel_distance_full(x, y)
    assert full == calc_kernel_distance_full(xd, yd) and full["kid"] == full["mmd2"]
    ref = KR.kid_full(x, y)
    assert abs(full["kid"] - ref["mmd2"]) <= 4e-7 * (ref["abs_kxx_mean"] + ref["abs_kyy_mean"] + 2 * ref["abs_kxy_mean"])
    with pytest.raises(ValueError):
        calc_kernel_distance(x, y, subsets=2, subset_size=141)
