"""Polynomial-kernel distance (fad_kid, fad_kid_subsets), host side (no GPU): the float64 reference against closed
forms, the float32 emulation against float64 (A_poly, from which the GPU tolerances are built), the exactness of the integer fixture, the
work units and groups (kid_tiles.h, checked with g++), the C ABI surface, the subsets a seed gives, the errors raised before any
library call, and the CSV."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kid_reference as KR

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------------- closed forms
def _sets(n, m, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)), rng.standard_normal((m, d)) * 1.2 + 0.3


@pytest.mark.parametrize("n,m,d", [(2, 3, 1), (40, 57, 5), (129, 130, 16)])
def test_reference_degree_one_closed_form(n, m, d):
    """degree 1, gamma 1, coef0 0: k = a.b, so Kxx = (|sum x|^2 - sum |x_i|^2) / (n (n - 1)), Kxy = (sum x).(sum y) / (n m), and MMD^2 is
    |xbar - ybar|^2 minus its bias terms (tr of the second moments over n - 1 and m - 1)."""
    x, y = _sets(n, m, d, seed=n + d)
    got = KR.kid_full(x, y, degree=1, gamma=1.0, coef0=0.0)
    sx, sy = x.sum(0), y.sum(0)
    kxx = (sx @ sx - (x * x).sum()) / (n * (n - 1))
    kyy = (sy @ sy - (y * y).sum()) / (m * (m - 1))
    kxy = sx @ sy / (n * m)
    scale = abs(kxx) + abs(kyy) + 2 * abs(kxy) + got["abs_kxx_mean"]
    assert abs(got["kxx_mean"] - kxx) <= 1e-12 * scale and abs(got["kyy_mean"] - kyy) <= 1e-12 * scale
    assert abs(got["kxy_mean"] - kxy) <= 1e-12 * scale
    xb, yb = x.mean(0), y.mean(0)
    bias = ((x * x).sum() / n - xb @ xb) / (n - 1) + ((y * y).sum() / m - yb @ yb) / (m - 1)
    assert abs(got["mmd2"] - ((xb - yb) @ (xb - yb) - bias)) <= 1e-12 * scale


@pytest.mark.parametrize("n,m,d", [(2, 3, 1), (40, 57, 5), (129, 130, 16)])
def test_reference_degree_two_second_moment_form(n, m, d):
    """degree 2: sum_ij (g a_i.b_j + c)^2 = g^2 <A, B> + 2 g c (sum a).(sum b) + c^2 n m with the second moments A = sum a a^T; the diagonal
    terms (g |a_i|^2 + c)^2 leave the same-set sums."""
    x, y = _sets(n, m, d, seed=2 * n + d)
    g, c = KR.params32(d, 0.37, 0.75)
    got = KR.kid_full(x, y, degree=2, gamma=0.37, coef0=0.75)

    def total(a, b):
        return g * g * ((a.T @ a) * (b.T @ b)).sum() + 2 * g * c * (a.sum(0) @ b.sum(0)) + c * c * len(a) * len(b)

    def diag(a):
        return ((g * (a * a).sum(1) + c) ** 2).sum()

    want = {"kxx_mean": (total(x, x) - diag(x)) / (n * (n - 1)), "kyy_mean": (total(y, y) - diag(y)) / (m * (m - 1)),
            "kxy_mean": total(x, y) / (n * m)}
    for k in KR.MEANS:
        assert abs(got[k] - want[k]) <= 1e-12 * got["abs_" + k], (k, got[k], want[k])
    assert abs(got["mmd2"] - (want["kxx_mean"] + want["kyy_mean"] - 2 * want["kxy_mean"])) <= 1e-12 * (got["abs_kxx_mean"] + got["abs_kyy_mean"])


def test_reference_subsets_are_full_sets_of_the_gathered_rows():
    x, y = _sets(30, 41, 7, seed=3)
    ix, iy = KR.exact_indices(30, 41, 4, 9, seed=1)
    sums = KR.kid_subsets(x, y, ix, iy)
    terms, mmd2, mean, std = KR.subset_stats(sums, 9)
    for q in range(4):
        r = KR.kid_full(x[ix[q]], y[iy[q]])
        assert terms[q, 0] == r["kxx_mean"] and terms[q, 1] == r["kyy_mean"] and terms[q, 2] == r["kxy_mean"] and mmd2[q] == r["mmd2"]
    assert mean == pytest.approx(mmd2.mean(), rel=1e-15) and std == pytest.approx(np.sqrt(((mmd2 - mmd2.mean()) ** 2).mean()), rel=1e-12)
    assert KR.subset_stats(sums[:1], 9)[3] == 0.0                                      # one subset: std 0


# ------------------------------------------------------------------------------------------------------- the emulation
@pytest.mark.parametrize("dt", KR.DTYPES)
def test_emulation_against_float64(dt):
    """The float32 chain at the GPU cases' shapes, against float64, relative to the mean of |k| of each block.  First order, a pair's
    k = u^p is off by at most p (B + p + 1) 2^-24 of the largest |u|^p its chain meets, B = ceil(D / step) the roundings of the MFMA
    chain; a mean over random rows stays well inside that.  A_poly is the worst over the cases and sets the GPU tolerance."""
    worst = 0.0
    for d, off, degree in KR.GAUSS_CASES:
        c = KR.gauss_case(d, off, degree, dt)
        bound = degree * (-(-d // KR.STEP[dt]) + degree + 1) * 2.0 ** -24
        err = c["chain_err"]
        print(f"[kid-chain] {dt} D={d} off={off} degree={degree}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()) + f" bound={bound:.2e}")
        for k in KR.MEANS + ("mmd2",):
            assert err[k] <= bound, (dt, d, off, degree, k, err[k], bound)
        worst = max(worst, max(err[k] for k in KR.MEANS))
    assert KR.poly_constant(dt) == worst
    print(f"[kid-chain] A_poly({dt}) = {worst:.3e}; GPU tolerance {KR.gpu_tolerance(dt):.3e}")
    assert KR.gpu_tolerance(dt) == max(4e-7, 4 * worst)


def test_emulation_is_exact_on_the_integer_fixture():
    x, y = KR.exact_rows(130, 131)
    want = KR.kid_full(x, y)
    for dt in KR.DTYPES:
        got = KR.chain32_poly_means(x, y, KR.STEP[dt])
        for k in KR.MEANS + ("mmd2",):
            assert got[k] == want[k], (dt, k)


def test_exact_fixture_sums_are_representable():
    """Every value of the exact GPU cases is a multiple of 2^-12 in [0, 8] (so 64 of them, at most 2^9, sum exactly in float32's 24
    bits), and every block sum stays below 2^53 2^-12: the float64 sums are exact in any order."""
    x, y = KR.exact_rows()
    assert set(np.unique(x)) <= {-1.0, 0.0, 1.0} and x.shape == (KR.EXACT_N, KR.EXACT_D) and y.shape == (KR.EXACT_M, KR.EXACT_D)
    g, c = KR.params32(KR.EXACT_D)
    assert g == 1.0 / 16 and c == 1.0
    for a, b in ((x, x), (y, y), (x, y)):
        k = KR.kmat(a, b, 3, g, c)
        assert np.all(k * 4096 == np.round(k * 4096)) and k.min() >= 0 and k.max() <= 8
        assert 64 * k.max() * 4096 < 2 ** 24 and k.sum() * 4096 < 2 ** 53
        u = g * (a @ b.T) + c
        assert np.all(u * 16 == np.round(u * 16)) and u.min() >= 0 and u.max() <= 2
        assert np.array_equal(KR.epilogue32_poly((a @ b.T).astype(np.float32), 3, g, c).astype(np.float64), k)
    assert max(KR.EXACT_SIZES) <= min(KR.EXACT_N, KR.EXACT_M)


# --------------------------------------------------------------------------------------------------- units and groups
def test_kid_tiles_cover(tmp_path):
    """kid_tiles.h: every (subset, block, tile) unit exactly once over the host's own launch cut, for s in {2, 128, 129, 300, 1000} and
    1, 3, 17, 100 subsets; kid::plan's groups cover the subsets exactly once for several budgets.  Plain C++, checked with g++."""
    exe = tmp_path / "kid_tiles_cover"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "native_cpu" / "kid_tiles_cover.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------------------ surface
def test_prototypes_present():
    import ctypes as C
    from fadtk_amd import _capi
    assert "fad_kid" in _capi.SIGNATURES and "fad_kid_subsets" in _capi.SIGNATURES
    res, args = _capi.SIGNATURES["fad_kid"]
    assert res is C.c_int and len(args) == 15 and args[9:12] == [C.c_int, C.c_double, C.c_double]
    res, args = _capi.SIGNATURES["fad_kid_subsets"]
    assert res is C.c_int and len(args) == 23 and args[9:12] == [C.c_int, C.c_double, C.c_double]
    names = [f for f, _ in _capi.FadKidResult._fields_]
    assert names == ["mmd2", "kxx_mean", "kyy_mean", "kxy_mean", "gamma", "coef0", "degree", "n", "m"]
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert "int fad_kid(" in header and "int fad_kid_subsets(" in header and "Repeated indices" in header


def test_exports_and_alias():
    import fadtk_amd
    import fadtk.kid as alias
    from fadtk_amd import kid
    assert fadtk_amd.calc_kernel_distance is kid.calc_kernel_distance and fadtk_amd.calc_kernel_distance_full is kid.calc_kernel_distance_full
    assert fadtk_amd.KernelDistance is kid.KernelDistance
    assert alias.calc_kernel_distance is kid.calc_kernel_distance and alias.main is kid.main


def test_subset_indices_are_reproducible_and_without_repeats():
    from fadtk_amd.kid import subset_indices
    ix, iy = subset_indices(50, 40, subsets=7, subset_size=33, seed=5)
    jx, jy = subset_indices(50, 40, subsets=7, subset_size=33, seed=5)
    assert ix.dtype == np.int32 and ix.shape == iy.shape == (7, 33)
    assert np.array_equal(ix, jx) and np.array_equal(iy, jy)
    kx, _ = subset_indices(50, 40, subsets=7, subset_size=33, seed=6)
    assert not np.array_equal(ix, kx)
    for q in range(7):
        assert len(set(ix[q])) == 33 and len(set(iy[q])) == 33
        assert ix[q].min() >= 0 and ix[q].max() < 50 and iy[q].min() >= 0 and iy[q].max() < 40
    rng = np.random.default_rng(5)                                                     # the documented order of the draws
    for q in range(7):
        assert np.array_equal(ix[q], rng.choice(50, 33, replace=False)) and np.array_equal(iy[q], rng.choice(40, 33, replace=False))
    fx, fy = subset_indices(33, 40, subsets=1, subset_size=33, seed=0)                 # a subset of the whole set: a permutation
    assert sorted(fx[0]) == list(range(33))


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, kid

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    x, y = np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32)
    with pytest.raises(ValueError, match="larger than the smaller set"):
        kid.calc_kernel_distance(x, y, subsets=3, subset_size=21)
    with pytest.raises(ValueError, match="at least 2 rows"):
        kid.calc_kernel_distance(x, y, subsets=3, subset_size=1)
    with pytest.raises(ValueError, match="at least 1 subset"):
        kid.calc_kernel_distance(x, y, subsets=0, subset_size=5)
    with pytest.raises(ValueError, match="degree"):
        kid.calc_kernel_distance(x, y, subsets=3, subset_size=5, degree=5)
    with pytest.raises(ValueError, match="degree"):
        kid.calc_kernel_distance_full(x, y, degree=0)
    with pytest.raises(ValueError, match="gamma"):
        kid.calc_kernel_distance(x, y, subsets=3, subset_size=5, gamma=float("nan"))
    with pytest.raises(ValueError, match="gamma"):
        kid.calc_kernel_distance_full(x, y, gamma=-1.0)
    with pytest.raises(ValueError, match="coef0"):
        kid.calc_kernel_distance_full(x, y, coef0=float("inf"))
    with pytest.raises(ValueError, match="different dimensions"):
        kid.calc_kernel_distance(x, np.zeros((30, 5), np.float32), subsets=3, subset_size=5)
    with pytest.raises(ValueError, match="2-D"):
        kid.calc_kernel_distance(x[0], y, subsets=3, subset_size=5)
    with pytest.raises(ValueError, match="at least 2 rows per set"):
        kid.calc_kernel_distance_full(x[:1], y)
    with pytest.raises(ValueError, match="one shape"):
        kid.calc_kernel_distance(x, y, indices=(np.zeros((2, 5), np.int32), np.zeros((2, 6), np.int32)))
    with pytest.raises(ValueError, match="larger than the smaller set"):
        kid.calc_kernel_distance(x, y, indices=(np.zeros((2, 21), np.int32), np.zeros((2, 21), np.int32)))


def test_csv_header_and_row(tmp_path):
    from fadtk_amd import kid
    assert kid.CSV_HEADER == "model,baseline,eval,n,m,kid_mean,kid_std,subsets,subset_size,degree,gamma,coef0,seed\n"
    res = {"kid_mean": 0.125, "kid_std": 0.5, "values": np.zeros(3), "subsets": 3, "subset_size": 10, "gamma": 0.0625, "coef0": 1.0, "degree": 3}
    row = kid.csv_row("vggish", "base", "evl", 20, 30, res, 7)
    assert row == "vggish,base,evl,20,30,0.125,0.5,3,10,3,0.0625,1.0,7"
    full = {"kid": 0.25, "mmd2": 0.25, "gamma": 0.0625, "coef0": 1.0, "degree": 2, "n": 20, "m": 30}
    assert kid.csv_row("vggish", "base", "evl", 20, 30, full, 7) == "vggish,base,evl,20,30,0.25,0.0,0,0,2,0.0625,1.0,"
    assert row.count(",") == kid.CSV_HEADER.count(",")
    target = tmp_path / "out" / "kid.csv"
    kid.append_csv(target, row)
    kid.append_csv(target, row)
    assert target.read_text() == kid.CSV_HEADER + row + "\n" + row + "\n"
    other = tmp_path / "other.csv"
    other.write_text("model,baseline,eval,kad\n")
    with pytest.raises(ValueError, match="another file"):
        kid.append_csv(other, row)
    assert other.read_text() == "model,baseline,eval,kad\n"


def test_command_line_refuses_bad_arguments_before_any_work(capsys):
    from fadtk_amd import kid
    for bad in (["--degree", "7"], ["--subset-size", "1"], ["--subsets", "0"], ["--gamma", "-2"]):
        with pytest.raises(SystemExit):
            kid.main(["vggish", "/nonexistent/base", "/nonexistent/eval", *bad])
    capsys.readouterr()
