"""The sliced Wasserstein permutation test without a GPU: the float64 reference of tests/sliced_permutation_reference.py
against what the definition implies -- the observed labelling is the plain distance, a stable split of the pooled stable argsort is the
sort of each group, a 6-row example by hand, the p-value counting with ties -- the statistic itself (its null rate and its power, in
the reference alone), and the surface: the Python refusals before the native library is touched, exports and aliases, the CSV, the
prototype, the library's argument checks (they come before any device call)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sliced_permutation_reference as PR
import sliced_reference as SR

ROOT = Path(__file__).resolve().parent.parent


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n,m", ((60, 45), (45, 60), (33, 33), (1, 7)))
def test_observed_labelling_is_the_plain_distance(n, m):
    x, y = SR.rows(n, m, 8, "fp32")
    t = SR.directions(5, 8)
    u = PR.labellings(n, m, 3)
    for ordered in (False, True):
        r = PR.permutation_test(x, y, t, "fp32", u, ordered)
        want = SR.sliced(x, y, t, "fp32", ordered)
        assert _same_bits(r["values"][0], want["values"])
        assert (r["sw2_squared"], r["max_sliced"], r["max_index"]) == (want["sw2_squared"], want["max_sliced"], want["max_index"])
        z = np.concatenate([x, y])
        for p in range(3):              # every labelling: the plain distance of its two groups (a float64 product of gathered rows may
            got = SR.sliced(z[u[p]], z[~u[p]], t, "fp32", ordered)["values"]               # differ in the last bits with the BLAS blocking)
            assert np.all(np.abs(r["values"][p + 1] - got) <= 1e-12 * got)


def test_stable_split_of_the_pooled_argsort_is_the_sort_of_each_group():
    rng = np.random.default_rng(3)
    keys = rng.integers(-5, 6, 500).astype(np.float64)                                 # many ties
    order = np.argsort(keys, kind="stable")
    for u in PR.labellings(300, 200, 8):
        bits = u[order]
        assert np.array_equal(keys[order][bits], np.sort(keys[u])) and np.array_equal(keys[order][~bits], np.sort(keys[~u]))
        assert np.array_equal(order[bits], np.flatnonzero(u)[np.argsort(keys[u], kind="stable")])        # ties in ascending row order
        assert np.array_equal(order[~bits], np.flatnonzero(~u)[np.argsort(keys[~u], kind="stable")])


def test_six_rows_by_hand():
    """x = 0, 1, 4, 5 and y = 2, 7 on a line: n = 4, m = 2, every overlap weighs 2 (of n m = 8).
    observed: a = 0 1 4 5, b = 2 7: S = 2 (4 + 1 + 9 + 4) = 36, W = 4.5
    u_1 = rows {0, 2, 4, 5}: a = 0 2 4 7, b = 1 5: S = 2 (1 + 1 + 1 + 4) = 14, W = 1.75
    u_2 = rows {1, 3, 4, 5}: a = 1 2 5 7, b = 0 4: S = 2 (1 + 4 + 1 + 9) = 30, W = 3.75
    u_3 = the observed labelling again: a tie, which counts.  The direction (2) has q = 4 and gives the same W."""
    x, y = np.array([[0.0], [1.0], [4.0], [5.0]], np.float32), np.array([[2.0], [7.0]], np.float32)
    u = np.array([[1, 0, 1, 0, 1, 1], [0, 1, 0, 1, 1, 1], [1, 1, 1, 1, 0, 0]], dtype=bool)
    for ordered in (False, True):
        r = PR.permutation_test(x, y, np.array([[1.0], [2.0]], np.float32), "fp32", u, ordered)
        assert np.array_equal(r["values"], [[4.5, 4.5], [1.75, 1.75], [3.75, 3.75], [4.5, 4.5]])
        assert np.array_equal(r["null"], [1.75, 3.75, 4.5]) and np.array_equal(r["null_max"], [1.75, 3.75, 4.5])
        assert r["p_value"] == 2 / 4 and r["p_value_max"] == 2 / 4 and r["sw2_squared"] == 4.5


def test_p_value_counting_with_ties():
    assert PR.p_values([3.0, 1.0, 2.0, 2.5], [9.0, 9.5, 1.0, 1.0]) == (1 / 4, 2 / 4)
    assert PR.p_values([3.0, 3.0, 3.0, 4.0, 2.0], [1.0, 1.0, 0.5, 0.5, 0.5]) == (4 / 5, 2 / 5)       # >= counts ties
    assert PR.p_values([0.0, 0.0], [0.0, 0.0]) == (1.0, 1.0)
    assert PR.p_values([5.0] + [1.0] * 199, [5.0] + [1.0] * 199) == (1 / 200, 1 / 200)


# ------------------------------------------------------------------------------------------------------------ the statistic itself
def _test_of(x, y, L, P, seed):
    t = SR.directions(L, x.shape[1], seed=seed).astype(np.float64)
    pz = np.concatenate([x, y]).astype(np.float64) @ t.T
    T, M = PR.null_statistics(pz, SR.direction_norms(t), PR.with_observed(PR.labellings(len(x), len(y), P, seed=seed), len(x)))
    return PR.p_values(T, M)


def test_null_rate():
    """100 null draws (x [60 x 8], y [45 x 8] standard normal), L = 16, P = 99: at most 12 may reject at 0.05 by either p-value --
    P(Binomial(100, 0.05) > 12) is about 0.0015.  With this file's directions and labellings: 7 by the mean, 6 by the maximum."""
    by_mean = by_max = 0
    for s in range(100):
        rng = np.random.default_rng([1000, s])
        x, y = rng.standard_normal((60, 8)), rng.standard_normal((45, 8))
        p, pmax = _test_of(x, y, 16, 99, s)
        by_mean += p <= 0.05
        by_max += pmax <= 0.05
    print(f"[sliced-perm-null] rejections at 0.05 of 100: {by_mean} by the mean, {by_max} by the maximum")
    assert by_mean <= 12 and by_max <= 12


def _mode_dropping(rng):
    centre = np.zeros(8)
    centre[0] = 3.0
    x = np.concatenate([rng.standard_normal((100, 8)) + centre, rng.standard_normal((100, 8)) - centre])
    return x, rng.standard_normal((150, 8)) + centre


POWER = {"shift": lambda rng: (rng.standard_normal((60, 8)), rng.standard_normal((45, 8)) + 0.5),
         "scale": lambda rng: (rng.standard_normal((200, 8)), 1.3 * rng.standard_normal((150, 8))),
         "mode dropping": _mode_dropping}


@pytest.mark.parametrize("case", list(POWER))
def test_power(case):
    """P = 199: a shift of 0.5 in every coordinate, a scale of 1.3, and a baseline of two clusters at +-3 on one axis against an
    evaluation set from one of them must each give p_value <= 0.05"""
    x, y = POWER[case](np.random.default_rng([2000, list(POWER).index(case)]))
    p, pmax = _test_of(x, y, 16, 199, 1)
    print(f"[sliced-perm-power] {case}: p = {p}, by the maximum {pmax}")
    assert p <= 0.05


# ------------------------------------------------------------------------------------------------------------ surface
def test_prototype_and_structures():
    from fadtk_amd import _capi
    res, args = _capi.SIGNATURES["fad_sliced_permutation_test"]
    assert res is C.c_int and len(args) == 20 and args[9:14] == [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int]
    assert _capi.SIGNATURES["fad_sliced_permutation_last_plan"] == (C.c_int, [C.POINTER(C.c_int64)])
    assert [f for f, _ in _capi.FadSlicedPermutationDetail._fields_] == ["values", "sorted_z", "index_z"]
    assert [f for f, _ in _capi.FadSlicedPermutationResult._fields_] == ["observed", "p_value", "p_value_max", "permutations"]
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert "int fad_sliced_permutation_test(" in header and "fad_sliced_permutation_detail_t" in header
    assert "int fad_sliced_permutation_last_plan(int64_t out[6]);" in header
    declared = header.split("int fad_sliced_permutation_test(")[1].split(");")[0]
    assert re.sub(r"/\*.*?\*/", "", declared).count(",") + 1 == len(args)


def test_library_exports_the_entries():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, "fad_sliced_permutation_test") and hasattr(lib, "fad_sliced_permutation_last_plan")
    assert lib.fad_version() == 2
    names = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "fadtk_amd" / "lib" / "libfad_hip.so")], capture_output=True, text=True,
                           check=True).stdout.split()
    assert "fad_sliced_permutation_test" in names and "fad_sliced_permutation_last_plan" in names


def test_exports_and_aliases():
    import fadtk_amd
    import fadtk.sliced as alias
    import fadtk.sliced_permutation as alias_cli
    from fadtk_amd import sliced, sliced_permutation
    assert fadtk_amd.calc_sliced_wasserstein_permutation_test is sliced.calc_sliced_wasserstein_permutation_test
    assert alias.calc_sliced_wasserstein_permutation_test is sliced.calc_sliced_wasserstein_permutation_test
    assert alias_cli.main is sliced_permutation.main and alias_cli.CSV_HEADER == sliced_permutation.CSV_HEADER
    assert hasattr(sliced.SlicedWasserstein, "score_permutation_test")
    assert sliced_permutation.CSV_HEADER == ("model,baseline,eval,n,m,sw2_squared,sliced_w2,std_error,max_sliced,p_value,p_value_max,"
                                             "permutations,projections,seed\n")


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, sliced

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    f = sliced.calc_sliced_wasserstein_permutation_test
    x, y = np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32)
    ok = np.zeros((3, 50), dtype=bool)
    for bad in (0, -3, 65537, 2.5, True):
        with pytest.raises(ValueError, match="projections"):
            f(x, y, projections=bad, labels=ok)
        with pytest.raises(ValueError, match="permutations"):
            f(x, y, permutations=bad)
    with pytest.raises(ValueError, match="seed"):
        f(x, y, seed=-1, labels=ok)
    with pytest.raises(ValueError, match="different dimensions"):
        f(x, np.zeros((30, 5), np.float32), labels=ok)
    with pytest.raises(ValueError, match="2-D"):
        f(x[0], y, labels=ok)
    with pytest.raises(ValueError, match="at least 1 row"):
        f(x[:0], y, labels=ok)
    with pytest.raises(ValueError, match="outside 1 .. 2048"):
        f(np.zeros((3, 2049), np.float32), np.zeros((3, 2049), np.float32), labels=np.zeros((3, 6), dtype=bool))
    with pytest.raises(ValueError, match=r"directions must be \[L x 4\]"):
        f(x, y, directions=np.ones((3, 5), np.float32), labels=ok)
    for bad in (np.zeros(50, dtype=bool), np.zeros((3, 49), dtype=bool), np.zeros((3, 51), np.uint8), np.zeros((3, 3), np.uint32),
                np.zeros((3, 50), np.int32), np.zeros((0, 50), dtype=bool), np.zeros((2, 3, 50), dtype=bool)):
        with pytest.raises(ValueError, match="labels|permutations"):
            f(x, y, labels=bad)


def test_csv_header_and_its_refusal(tmp_path):
    from fadtk_amd import sliced, sliced_permutation as sp
    res = {"n": 123, "m": 57, "sw2_squared": 0.25, "sliced_w2": 0.5, "std_error": 0.125, "max_sliced": 2.0, "p_value": 0.005,
           "p_value_max": 0.01, "permutations": 199, "projections": 16, "seed": 2}
    target = tmp_path / "sub" / "perm.csv"
    for _ in range(2):
        sp.append_csv(target, sp.csv_row("vggish", "base", "evl", res))
    lines = target.read_text().splitlines()
    assert lines[0] + "\n" == sp.CSV_HEADER and lines[1] == lines[2] == "vggish,base,evl,123,57,0.25,0.5,0.125,2.0,0.005,0.01,199,16,2"
    assert len(lines[1].split(",")) == len(sp.CSV_HEADER.split(","))
    other = tmp_path / "sliced.csv"
    other.write_text(sliced.CSV_HEADER)
    with pytest.raises(ValueError, match="another file"):
        sp.append_csv(other, sp.csv_row("vggish", "base", "evl", res))
    with pytest.raises(ValueError, match="another file"):                              # before any file is read or embedded
        sp.main(["vggish", str(tmp_path / "none"), str(tmp_path / "none2"), str(other)])
    assert other.read_text() == sliced.CSV_HEADER
    for bad in (["-p", "0"], ["-p", "65537"], ["--projections", "0"], ["--seed", "-1"]):
        with pytest.raises(SystemExit):
            sp.main(["vggish", "a", "b", *bad])


def test_without_a_gpu_the_entry_fails_loudly():
    import torch
    from fadtk_amd import _capi, sliced
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_sliced_permutation.py runs the entry")
    x, y = SR.rows(30, 20, 8, "fp32")
    with pytest.raises(_capi.FadHipUnavailable):
        sliced.calc_sliced_wasserstein_permutation_test(x, y, projections=4, labels=PR.labellings(30, 20, 5))


def test_argument_errors_before_any_device_call():
    """the library's own refusals need no GPU: they come before the device is opened (FAD_ERR_NO_DEVICE where there is none)"""
    import torch
    from fadtk_amd import _capi, hip
    lib = _capi.load_library()
    x, y = SR.rows(30, 20, 37, "fp32")
    t = SR.directions(4, 37)
    lab = hip.pack_labels(PR.labellings(30, 20, 5))
    res = _capi.FadSlicedPermutationResult()
    res.observed.sw2_squared, res.p_value = -7.0, -7.0
    null, null_max, vals = np.full(5, -7.0), np.full(5, -7.0), np.full((6, 4), -7.0)
    sz, iz = np.full((4, 50), -7.0, np.float32), np.full((4, 50), -7, np.int32)
    det = _capi.FadSlicedPermutationDetail(vals.ctypes.data, sz.ctypes.data, iz.ctypes.data)

    def call(n=30, m=20, d=37, dt=_capi.FAD_F32, th=t, L=4, out=C.byref(res), ld=37, lb=lab, P=5, nl=null, nx=null_max, xa=x):
        return lib.fad_sliced_permutation_test(xa.ctypes.data if xa is not None else None, n, ld, y.ctypes.data, m, ld, d, dt, 0,
                                               th.ctypes.data if th is not None else None, L, lb.ctypes.data if lb is not None else None, P, 0,
                                               out, nl.ctypes.data if nl is not None else None, nx.ctypes.data if nx is not None else None,
                                               C.byref(det), 0, None)
    INVALID, TOO_FEW = _capi.FAD_ERR_INVALID, _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(dt=_capi.FAD_F64) == INVALID and call(xa=None) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID and call(d=37, ld=36) == INVALID
    assert call(L=0) == INVALID and call(L=65537) == INVALID
    assert call(out=None) == INVALID and call(th=None) == INVALID and call(nl=None) == INVALID and call(nx=None) == INVALID
    assert call(lb=None) == INVALID and call(P=0) == INVALID and call(P=65537) == INVALID
    assert call(n=0) == TOO_FEW and call(m=0) == TOO_FEW
    assert call(n=2 ** 30, m=2 ** 30) == INVALID                                       # N = 2^31
    assert call(n=2 ** 31 - 148, m=20) == INVALID                                      # N = 2^31 - 128
    assert call(n=2 ** 27, m=2 ** 26) == INVALID                                       # n m = 2^53
    tb = t.copy()
    tb[2, 5] = np.nan
    assert call(th=tb) == INVALID
    tz = t.copy()
    tz[1] = 0
    assert call(th=tz) == INVALID                                                      # q = 0
    wrong = lab.copy()
    wrong[3, 0] ^= np.uint32(1)                                                        # one labelling with n - 1 or n + 1 ones
    assert call(lb=wrong) == INVALID
    assert "fad_sliced_permutation_test: labelling 3" in _capi.last_error()
    past = lab.copy()
    past[1, 1] |= np.uint32(1 << 20)                                                   # a bit at row 52 >= N = 50
    assert call(lb=past) == INVALID
    assert res.observed.sw2_squared == -7.0 and res.p_value == -7.0
    for a in (null, null_max, vals, sz):
        assert np.all(a == -7.0)
    assert np.all(iz == -7)
    plan = (C.c_int64 * 6)(9, 9, 9, 9, 9, 9)
    assert lib.fad_sliced_permutation_last_plan(plan) == 0 and list(plan) == [0] * 6
    assert lib.fad_sliced_permutation_last_plan(None) == INVALID
    if not torch.cuda.is_available():
        assert call() == _capi.FAD_ERR_NO_DEVICE
