"""Per-row shares of the sliced Wasserstein distance without a GPU: the float64 reference of tests/sliced_shares_reference.py checked
against what the definition implies -- both index formulas against replication to lcm(n, m), both sides summing to S,
the two summation orders, the tie rule -- and the Python layer of fadtk_amd/sliced.py: its refusals before the native library is
touched, the file sums from offsets, the CSV, the prototype.  The library's argument checks run here too: they come before any device
call."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import sliced_reference as SR
import sliced_shares_reference as SS

ROOT = Path(__file__).resolve().parent.parent


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n,m", SS.LCM_SIZES)
def test_index_formulas_equal_replication(n, m):
    rng = np.random.default_rng([n, m])
    a, b = np.sort(rng.integers(-50, 51, n)).astype(np.float64), np.sort(rng.integers(-50, 51, m)).astype(np.float64)
    want_a, want_b = SS.replicated_costs(a, b)                                         # integers: every sum is exact
    for ordered in (False, True):
        ca, cb = SS.rank_costs(a, b, ordered)
        assert np.array_equal(ca, want_a) and np.array_equal(cb, want_b), ordered
        assert ca.sum() == cb.sum() == SR.match_sum(a, b) == SR.replicated_sum(a, b)


@pytest.mark.parametrize("n,m", SS.LCM_SIZES + ((130, 257), (1, 300)))
def test_both_orders_agree_and_both_sides_sum_to_s(n, m):
    rng = np.random.default_rng([5, n, m])
    a, b = np.sort(rng.standard_normal(n)), np.sort(1.25 * rng.standard_normal(m) + 0.5)
    ca, cb = SS.rank_costs(a, b)
    oa, ob = SS.rank_costs(a, b, ordered=True)
    assert _same_bits(ca, oa) and _same_bits(cb, ob)                                   # the same terms in the same order, spelled twice
    s = SR.match_sum(a, b)
    assert abs(ca.sum() - s) <= (n + m) * 2.0 ** -52 * s and abs(cb.sum() - s) <= (n + m) * 2.0 ** -52 * s
    sa, sb = SS.rank_costs(b, a, ordered=True)                                         # swapped: the larger set leads either way
    assert _same_bits(sa, ob) and _same_bits(sb, oa)


def test_shares_sum_to_the_distance_and_follow_the_rows():
    x, y = SR.rows(257, 130, 16, "fp32")
    t = SR.directions(5, 16)
    r = SS.shares(x, y, t, "fp32", ordered=True)
    want = SR.sliced(x, y, t, "fp32")["sw2_squared"]
    assert abs(r["share_x"].sum() - want) <= 1e-13 * want and abs(r["share_y"].sum() - want) <= 1e-13 * want
    assert np.all(r["share_x"] >= 0) and np.all(r["share_y"] >= 0)
    perm = np.random.default_rng(1).permutation(257)                                   # no ties here: a share follows its row
    moved = SS.shares(x[perm], y, t, "fp32", ordered=True)
    assert _same_bits(moved["share_x"], r["share_x"][perm]) and _same_bits(moved["share_y"], r["share_y"])
    far = y.copy()
    far[7] += 40.0                                                                     # an outlier carries the distance
    out = SS.shares(x, far, t, "fp32")
    assert np.argmax(out["share_y"]) == 7 and out["share_y"][7] > 0.5 * out["share_y"].sum()


def test_ties_are_ranked_by_row_index():
    x = np.array([[2.0], [1.0], [1.0], [1.0]])                                         # rows 1, 2, 3 tie along e_0
    y = np.array([[0.0], [1.0], [5.0], [9.0]])
    r = SS.shares(x, y, np.array([[1.0]], np.float32), "fp32", ordered=True)
    assert np.array_equal(r["index_x"][0], [1, 2, 3, 0])
    assert np.array_equal(r["share_x"] * 16, [4 * 49.0, 4 * 1.0, 0.0, 4 * 16.0])        # row 1 meets 0, row 2 meets 1, row 3 meets 5, row 0 meets 9
    assert np.array_equal(r["share_y"] * 16, [4 * 1.0, 0.0, 4 * 16.0, 4 * 49.0])


def test_share_bound_is_zero_without_projection_error_and_grows_with_it():
    x, y = SR.rows(6, 4, 3, "fp32")
    t = SR.directions(2, 3)
    px, q = SS.projections(x, t, "fp32")
    py, _ = SS.projections(y, t, "fp32")
    bx, by = SS.share_bound(np.sort(px, 1), np.sort(py, 1), q, np.zeros(2), np.zeros(2))
    assert np.all(bx == 0) and np.all(by == 0)
    bx, by = SS.share_bound(np.sort(px, 1), np.sort(py, 1), q, np.full(2, 1e-6), np.full(2, 1e-6))
    assert np.all(bx > 0) and np.all(by > 0) and abs(bx.sum() - by.sum()) <= 1e-12 * bx.sum()


# ------------------------------------------------------------------------------------------------------------ surface
def test_prototype_and_structures():
    from fadtk_amd import _capi
    res, args = _capi.SIGNATURES["fad_sliced_shares"]
    assert res is C.c_int and len(args) == 17 and args[9:11] == [C.c_void_p, C.c_int] and args[12:14] == [C.c_void_p, C.c_void_p]
    assert [f for f, _ in _capi.FadSlicedSharesDetail._fields_] == ["values", "sorted_x", "sorted_y", "index_x", "index_y"]
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert "int fad_sliced_shares(" in header and "fad_sliced_shares_detail_t" in header


def test_library_exports_the_entry():
    from fadtk_amd import _capi
    assert hasattr(_capi.load_library(), "fad_sliced_shares")


def test_exports_and_alias():
    import fadtk_amd
    import fadtk.sliced as alias
    from fadtk_amd import sliced
    assert fadtk_amd.calc_sliced_wasserstein_shares is sliced.calc_sliced_wasserstein_shares
    assert alias.calc_sliced_wasserstein_shares is sliced.calc_sliced_wasserstein_shares
    assert alias.SHARES_CSV_HEADER == sliced.SHARES_CSV_HEADER == "side,file,rows,share,fraction,lift\n"


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, sliced

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    f = sliced.calc_sliced_wasserstein_shares
    x, y = np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32)
    for bad in (0, -3, 65537, 2.5, True):
        with pytest.raises(ValueError, match="projections"):
            f(x, y, projections=bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            f(x, y, seed=bad)
    with pytest.raises(ValueError, match="different dimensions"):
        f(x, np.zeros((30, 5), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        f(x[0], y)
    with pytest.raises(ValueError, match="at least 1 row"):
        f(x[:0], y)
    with pytest.raises(ValueError, match="outside 1 .. 2048"):
        f(np.zeros((3, 2049), np.float32), np.zeros((3, 2049), np.float32))
    with pytest.raises(ValueError, match=r"directions must be \[L x 4\]"):
        f(x, y, directions=np.ones((3, 5), np.float32))
    with pytest.raises(ValueError, match="not finite"):
        f(x, y, directions=np.array([[1.0, np.nan, 0.0, 0.0]]))
    for bad in ([0, 19], [1, 20], [0, 12, 11, 20], [0], [[0, 20]], [0.0, 20.0]):
        with pytest.raises(ValueError, match="x_offsets"):
            f(x, y, x_offsets=bad)
    with pytest.raises(ValueError, match="y_offsets"):
        f(x, y, x_offsets=[0, 20], y_offsets=[0, 20])


def test_without_a_gpu_the_entry_fails_loudly():
    import torch
    from fadtk_amd import _capi, sliced
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_sliced_shares.py runs the entry")
    x, y = SR.rows(30, 20, 8, "fp32")
    with pytest.raises(_capi.FadHipUnavailable):
        sliced.calc_sliced_wasserstein_shares(x, y, projections=4)


def test_file_sums_and_lift():
    from fadtk_amd import sliced
    share = np.array([0.5, 0.25, 0.125, 0.0625, 0.0625])
    off = np.array([0, 2, 2, 5])
    fs = sliced.file_sums(share, off)
    assert np.array_equal(fs, [0.75, 0.0, 0.25])
    lift = sliced.file_lift(fs, off, 1.0)
    assert lift[0] == 0.75 / 0.4 and np.isnan(lift[1]) and lift[2] == 0.25 / 0.6
    assert np.all(np.isnan(sliced.file_lift(np.zeros(3), off, 0.0)[[0, 2]]))


def test_shares_csv(tmp_path):
    from fadtk_amd import sliced
    xo, yo = np.array([0, 2, 5]), np.array([0, 1, 2, 4])
    res = {"sw2_squared": 2.0, "file_share_x": np.array([0.5, 1.5]), "file_share_y": np.array([0.25, 1.5, 0.25])}
    res["file_lift_x"] = sliced.file_lift(res["file_share_x"], xo, 2.0)
    res["file_lift_y"] = sliced.file_lift(res["file_share_y"], yo, 2.0)
    target = tmp_path / "sub" / "shares.csv"
    assert sliced.write_shares_csv(target, ["a.wav", "b,1.wav"], ["c.wav", "d.wav", "e.wav"], res, xo, yo) == 5
    lines = target.read_text().splitlines()
    assert lines[0] + "\n" == sliced.SHARES_CSV_HEADER
    assert lines[1:] == ["baseline,b_1.wav,3,1.5,0.75,1.25", "baseline,a.wav,2,0.5,0.25,0.625", "eval,d.wav,1,1.5,0.75,3.0",
                         "eval,c.wav,1,0.25,0.125,0.5", "eval,e.wav,2,0.25,0.125,0.25"]           # ties in the order of the files
    sliced.write_shares_csv(target, ["a.wav", "b.wav"], ["c.wav", "d.wav", "e.wav"], res, xo, yo)  # this header: replaced
    assert len(target.read_text().splitlines()) == 6
    other = tmp_path / "indiv.csv"
    other.write_text(sliced.INDIV_CSV_HEADER)
    with pytest.raises(ValueError, match="another file"):
        sliced.write_shares_csv(other, ["a.wav", "b.wav"], ["c.wav", "d.wav", "e.wav"], res, xo, yo)
    assert other.read_text() == sliced.INDIV_CSV_HEADER


def test_command_line_refuses_a_foreign_header_and_both_modes(tmp_path):
    from fadtk_amd import sliced
    other = tmp_path / "sliced.csv"
    other.write_text(sliced.CSV_HEADER)
    with pytest.raises(ValueError, match="another file"):                              # before any file is read or embedded
        sliced.main(["vggish", str(tmp_path / "none"), str(tmp_path / "none2"), str(other), "--shares"])
    with pytest.raises(SystemExit):
        sliced.main(["vggish", "a", "b", "--shares", "--indiv"])


def test_argument_errors_before_any_device_call():
    """the library's own refusals need no GPU: they come before the device is opened (FAD_ERR_NO_DEVICE where there is none)"""
    import torch
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(30, 20, 37, "fp32")
    t = SR.directions(4, 37)
    res = _capi.FadSlicedResult()
    res.sw2_squared = -7.0
    vals, shx, shy = np.full(4, -7.0), np.full(30, -7.0), np.full(20, -7.0)
    ix = np.full((4, 30), -7, np.int32)
    det = _capi.FadSlicedSharesDetail(vals.ctypes.data, None, None, ix.ctypes.data, None)

    def call(n=30, m=20, d=37, dt=_capi.FAD_F32, th=t, L=4, out=C.byref(res), ld=37, sx=shx, sy=shy):
        return lib.fad_sliced_shares(x.ctypes.data, n, ld, y.ctypes.data, m, ld, d, dt, 0, th.ctypes.data if th is not None else None, L,
                                     out, sx.ctypes.data if sx is not None else None, sy.ctypes.data if sy is not None else None,
                                     C.byref(det), 0, None)
    INVALID, TOO_FEW = _capi.FAD_ERR_INVALID, _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(dt=_capi.FAD_F64) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID and call(d=37, ld=36) == INVALID
    assert call(L=0) == INVALID and call(L=65537) == INVALID
    assert call(out=None) == INVALID and call(th=None) == INVALID and call(sx=None) == INVALID and call(sy=None) == INVALID
    assert call(n=0) == TOO_FEW and call(m=0) == TOO_FEW
    assert call(n=2 ** 27, m=2 ** 26) == INVALID                                       # n m = 2^53
    tb = t.copy()
    tb[2, 5] = np.nan
    assert call(th=tb) == INVALID
    tz = t.copy()
    tz[1] = 0
    assert call(th=tz) == INVALID                                                      # q = 0
    assert res.sw2_squared == -7.0 and np.all(vals == -7.0) and np.all(shx == -7.0) and np.all(shy == -7.0) and np.all(ix == -7)
    plan = (C.c_int64 * 4)(9, 9, 9, 9)
    assert lib.fad_sliced_last_plan(plan) == 0 and list(plan) == [0, 0, 0, 0]
    if not torch.cuda.is_available():
        assert call() == _capi.FAD_ERR_NO_DEVICE
