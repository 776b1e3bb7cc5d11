"""The Sinkhorn divergence without a GPU: the float64 reference of tests/sinkhorn_reference.py checked against what the definition
implies, and the Python layer of fadtk_amd/sinkhorn.py -- its refusals before the native library is touched, the CSV,
the command line, the alias module and the row subsample."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import sinkhorn_reference as SR

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------------ the reference
def test_one_row_each_is_half_the_squared_distance():
    x, y = SR.rows(1, 1, 5, "fp32")
    want = 0.5 * float(((x.astype(np.float64) - y) ** 2).sum())
    for eps in (0.01, 1.0, 100.0):
        for L in (1, 3):
            assert abs(SR.sinkhorn(x, y, eps, L)["divergence"] - want) <= 1e-13 * want


def test_large_blur_is_the_distance_of_the_means():
    x, y = SR.rows(300, 200, 37, "fp32")
    y = y + 0.25
    want = 0.5 * float(((x.mean(axis=0, dtype=np.float64) - y.mean(axis=0, dtype=np.float64)) ** 2).sum())
    got = SR.sinkhorn(x, y, 1e6 * SR.median_distance(x) ** 2, 5)["divergence"]
    assert abs(got - want) <= 1e-4 * want


def test_first_half_step_lies_between_the_minimum_and_eps_log_m():
    """f_i = softmin_j C_ij + eps log m after the first step (g = 0): 0 <= f_i - min_j C_ij <= eps log m, an identity."""
    x, y = SR.rows(300, 200, 37, "fp32")
    Cm = SR.cost(x, y)
    for factor in (0.02, 0.25, 1.0):
        eps = (factor * SR.median_distance(x)) ** 2
        gap = SR.f_step(Cm, np.zeros(200), eps) - Cm.min(axis=1)
        assert gap.min() >= -1e-12 * Cm.max() and gap.max() <= eps * np.log(200) + 1e-12 * Cm.max()


def test_the_plan_sums_to_one_after_every_g_step():
    x, y = SR.rows(129, 127, 128, "fp32")
    Cm = SR.cost(x, y)
    eps = (0.25 * SR.median_distance(x)) ** 2
    seen = []

    def check(f, g):
        seen.append(SR.plan_mass(Cm, f, g, eps))
    SR.ot(Cm, eps, 6, check=check)
    assert len(seen) == 6 and np.abs(np.array(seen) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("factor", (0.05, 0.25, 1.0))
def test_divergence_is_non_negative_and_the_potentials_add_up_to_it(factor):
    x, y = SR.rows(257, 130, 64, "fp32")
    r = SR.sinkhorn(x, y, (factor * SR.median_distance(x)) ** 2, 30)
    assert r["divergence"] >= 0
    assert abs(r["pot_x"].mean() + r["pot_y"].mean() - r["divergence"]) <= 1e-12 * max(1.0, abs(r["ot_xy"]))


def test_equal_sets_have_divergence_zero():
    x, _ = SR.rows(128, 128, 64, "fp32")
    r = SR.sinkhorn(x, x.copy(), (0.25 * SR.median_distance(x)) ** 2, 10)
    assert r["divergence"] == 0.0 and r["ot_xy"] == r["ot_xx"] == r["ot_yy"]


def test_marginal_error_falls_with_the_iterations():
    x, y = SR.rows(300, 200, 37, "fp32")
    eps = (0.25 * SR.median_distance(x)) ** 2
    errs = [SR.sinkhorn(x, y, eps, L)["marginal_error"] for L in (1, 5, 30)]
    assert errs[0] > errs[1] > errs[2] and errs[2] < 1e-12


def test_bf16_rounding_is_round_to_nearest_even():
    a = np.array([1.0, 1.00390625, 1.01171875, 1.0078125, -1.00390625, 1.005], np.float32)      # ties at 2^-8 go to even
    assert np.array_equal(SR.round_to(a, "bf16"), np.array([1.0, 1.0, 1.015625, 1.0078125, -1.0, 1.0078125], np.float32))


# --------------------------------------------------------------------------- the references of the edge tests (no GPU)
def _rel(got, want):
    """the worst difference of the compared quantities, relative to the size of the potentials"""
    scale = max(float(np.abs(want[k]).max()) for k in SR.POTS)
    keys = SR.POTS + SR.TERMS + ("marginal_error", "marginal_error_xx", "marginal_error_yy")
    return max(float(np.abs(np.asarray(got[k]) - np.asarray(want[k])).max()) for k in keys) / scale


@pytest.mark.parametrize("block", (77, 128))
def test_blocked_float64_equals_the_dense_reference(block):
    """neither block size divides 300 or 200: a ragged last block in both directions of all three problems"""
    x, y = SR.rows(300, 200, 37, "fp32")
    eps = (0.25 * SR.median_distance(x)) ** 2
    want = SR.sinkhorn(x, y, eps, 5)
    got = SR.sinkhorn_blocked(x, y, eps, 5, "cpu", block=block)
    assert set(got) == set(want) and got["f"].shape == (300,) and got["pot_y"].shape == (200,)
    assert _rel(got, want) <= 1e-12


@pytest.mark.parametrize("dt,L", (("fp16", 2), ("bf16", 2), ("fp32", 2), ("fp32", 30)))
def test_chain32_is_within_one_unit_of_float64_at_the_default_blur(dt, L):
    """f, g, F, G, the three OT terms and S -- what the GPU tests compare.  f and g of the self problems are not compared one by one:
    the diagonal pair dominates there, so f_i - g_i is nearly free and drifts with L while f + g does not."""
    x, y = SR.rows(129, 127, 128, dt)
    eps = (0.25 * SR.median_distance(x)) ** 2
    want, got = SR.sinkhorn(x, y, eps, L), SR.sinkhorn_chain32(x, y, eps, L, dt)
    r = SR.ratios(got, want, SR.unit(x, y, eps))
    assert max(r.values()) <= 1.0, r
    assert 0.0 < max(r.values()), "the emulation is float32: it cannot equal float64"
    assert abs(got["marginal_error"] - want["marginal_error"]) <= 1e-4 * (1.0 + want["marginal_error"])


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_chain32_gives_exactly_zero_for_identical_sets(dt):
    x, _ = SR.rows(129, 127, 128, dt)
    got = SR.sinkhorn_chain32(x, x.copy(), 3.0, 3, dt)
    assert got["divergence"] == 0.0 and got["ot_xy"] == got["ot_xx"] == got["ot_yy"]


def test_chain32_over_several_row_blocks_per_unit(monkeypatch):
    """The emulation's own unit loop (rr = 2, a ragged last range) against rr = 1 on the same rows: another merge order, the same
    soft-min within float32."""
    x, y = SR.rows(300, 200, 37, "fp32")
    eps = (0.25 * SR.median_distance(x)) ** 2
    one = SR.sinkhorn_chain32(x, y, eps, 2, "fp32")
    monkeypatch.setattr(SR, "CROSS_UNITS", 4)                                      # 3 x 2 blocks: rr = 2 for the 3, 1 for the 2
    assert SR.cross_plan(300, 200)[2:] == (2, 2) and SR.cross_plan(200, 300)[2:] == (1, 2)
    two = SR.sinkhorn_chain32(x, y, eps, 2, "fp32")
    r = SR.ratios(two, one, SR.unit(x, y, eps))
    assert max(r.values()) <= 1.0, r


def test_cross_plan_of_the_large_case_walks_two_row_blocks_per_unit():
    """kad::cross_rows_per_unit: nr = ceil(8192 / TJ) ranges at most, rr = ceil(TI / nr).  rr = 2 needs TI > ceil(8192 / TJ): 92 x 92
    blocks (n = m >= 11 649) is the smallest square shape.  11 800 x 11 700 is 93 x 92 blocks."""
    TI, TJ, rr, NR = SR.cross_plan(11800, 11700)
    assert (TI, TJ, rr, NR) == (93, 92, 2, 47) and TI - (NR - 1) * rr == 1         # the last range is a single block
    TI, TJ, rr, NR = SR.cross_plan(11700, 11800)
    assert (TI, TJ, rr, NR) == (92, 93, 2, 46) and TI - (NR - 1) * rr == 2
    assert SR.cross_plan(11648, 11648)[2] == 1 and SR.cross_plan(11649, 11649)[2] == 2
    assert SR.cross_plan(11800, 11700, depth=64, f32=True)[2] == 2                 # the default budget does not bind here
    assert SR.cross_plan(1200, 1100) == (10, 9, 1, 10)                             # the largest shape of test_gpu_sinkhorn.py: never
    assert SR.cross_plan(1, 300) == (1, 3, 1, 1) and SR.cross_plan(100000, 100000)[2] == 72


def test_cross_plan_restates_the_header():
    """the constants it restates, read from the headers"""
    import re
    song = (ROOT / "fadtk_amd" / "csrc" / "kad_song_tiles.h").read_text()
    tiles = (ROOT / "fadtk_amd" / "csrc" / "kad_tiles.h").read_text()
    assert int(re.search(r"kCrossUnits = (\d+);", song).group(1)) == SR.CROSS_UNITS
    assert int(re.search(r"kSoftminEpilogue = (\d+);", tiles).group(1)) == SR.SOFTMIN_EPILOGUE
    assert "kLaunchBudget = (int64_t)1 << 30;" in tiles and SR.LAUNCH_BUDGET == 1 << 30
    assert "int64_t rr = (TI + nr - 1) / nr;" in song and "I0 + rr < TI ? I0 + rr : TI" in song


def test_a_translated_copy_at_a_large_blur():
    """y = x + t, t a power of two so that it stays exact: S -> |t|^2 / 2 as the blur grows (the distance of the means), and the two self
    problems are the same problem.  Translation invariance is what a bug in the offset cases would break."""
    x, _ = SR.rows(129, 127, 16, "fp32")
    x = np.round(x * 8.0) / 8.0
    y = x + np.float32(2.0)
    assert np.array_equal(y - np.float32(2.0), x)
    r = SR.sinkhorn(x, y, (1000.0 * SR.median_distance(x)) ** 2, 5)
    assert abs(r["divergence"] - 0.5 * 16 * 4.0) <= 1e-4 * 32.0
    assert abs(r["ot_xx"] - r["ot_yy"]) <= 1e-12 * abs(r["ot_xx"])
    near = SR.sinkhorn(x, y, (0.25 * SR.median_distance(x)) ** 2, 30)              # and at the default blur: the same self problems
    assert abs(near["ot_xx"] - near["ot_yy"]) <= 1e-12 * abs(near["ot_xx"])


def test_edge_rows_round_after_the_addition():
    x0, y0 = SR.rows(129, 127, 128, "bf16")
    x, y = SR.edge_rows(129, 127, 128, "bf16", off=16.0, sep=2.0)
    assert np.array_equal(x, SR.round_to(x0 + np.float32(16), "bf16")) and np.array_equal(y, SR.round_to(y0 + np.float32(18), "bf16"))
    assert np.array_equal(SR.round_to(x, "bf16"), x) and not np.array_equal(x - np.float32(16), x0)
    assert np.array_equal(SR.edge_rows(129, 127, 128, "fp16")[0], SR.rows(129, 127, 128, "fp16")[0])       # no offset: rows() itself


# ------------------------------------------------------------------------------------------------------------ surface
def test_prototype_and_structures():
    from fadtk_amd import _capi
    res, args = _capi.SIGNATURES["fad_sinkhorn"]
    assert res is C.c_int and len(args) == 15 and args[9:11] == [C.c_double, C.c_int]
    assert [f for f, _ in _capi.FadSinkhornResult._fields_] == ["divergence", "ot_xy", "ot_xx", "ot_yy", "epsilon", "marginal_error",
                                                                "marginal_error_xx", "marginal_error_yy", "n", "m", "iterations"]
    assert [f for f, _ in _capi.FadSinkhornDetail._fields_] == ["f", "g", "pot_x", "pot_y"]
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert "int fad_sinkhorn(" in header and "fad_sinkhorn_detail_t" in header and "FAD_SINKHORN_BLUR_FACTOR 0.25" in header


def test_library_exports_the_entry():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, "fad_sinkhorn") and lib.fad_version() == 2


def test_exports_and_alias():
    import fadtk_amd
    import fadtk.sinkhorn as alias
    from fadtk_amd import sinkhorn
    assert fadtk_amd.calc_sinkhorn_divergence is sinkhorn.calc_sinkhorn_divergence
    assert fadtk_amd.SinkhornDivergence is sinkhorn.SinkhornDivergence
    assert alias.calc_sinkhorn_divergence is sinkhorn.calc_sinkhorn_divergence and alias.main is sinkhorn.main
    assert alias.SinkhornDivergence is sinkhorn.SinkhornDivergence and alias.CSV_HEADER == sinkhorn.CSV_HEADER


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, sinkhorn

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    x, y = np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32)
    with pytest.raises(ValueError, match="not both"):
        sinkhorn.calc_sinkhorn_divergence(x, y, blur=1.0, blur_factor=0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="blur must be"):
            sinkhorn.calc_sinkhorn_divergence(x, y, blur=bad)
        with pytest.raises(ValueError, match="blur_factor must be"):
            sinkhorn.calc_sinkhorn_divergence(x, y, blur_factor=bad)
    for bad in (0, -3, 100001, 2.5, True):
        with pytest.raises(ValueError, match="iterations"):
            sinkhorn.calc_sinkhorn_divergence(x, y, iterations=bad)
    with pytest.raises(ValueError, match="different dimensions"):
        sinkhorn.calc_sinkhorn_divergence(x, np.zeros((30, 5), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        sinkhorn.calc_sinkhorn_divergence(x[0], y)
    with pytest.raises(ValueError, match="at least 1 row"):
        sinkhorn.calc_sinkhorn_divergence(x[:0], y)
    with pytest.raises(ValueError, match="outside 1 .. 2048"):
        sinkhorn.calc_sinkhorn_divergence(np.zeros((3, 2049), np.float32), np.zeros((3, 2049), np.float32))
    with pytest.raises(ValueError, match="needs 2 rows"):
        sinkhorn.calc_sinkhorn_divergence(x[:1], y)                                    # the default blur needs a median
    with pytest.raises(ValueError, match="max_rows"):
        sinkhorn.subsample_rows(x, 0)


def test_hip_layer_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, hip
    monkeypatch.setattr(_capi, "load_library", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the native library was touched")))
    x = np.zeros((4, 3), np.float32)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="epsilon"):
            hip.sinkhorn(x, x, epsilon=bad)
    for bad in (0, 100001, 1.5):
        with pytest.raises(ValueError, match="iterations"):
            hip.sinkhorn(x, x, iterations=bad)
    assert hip.sinkhorn_params(None, 100) == (0.0, 100) and hip.sinkhorn_params(2, 7) == (2.0, 7)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from fadtk_amd import _capi, sinkhorn
    x, y = SR.rows(300, 200, 37, "fp32")
    with pytest.raises(_capi.FadHipUnavailable):
        sinkhorn.calc_sinkhorn_divergence(x, y)
    with pytest.raises(_capi.FadHipUnavailable):
        sinkhorn.calc_sinkhorn_divergence(x, y, blur=2.0, iterations=3, potentials=True)
    # argument errors come before any device call: they are told apart from the missing device
    lib = _capi.load_library()
    res = _capi.FadSinkhornResult()
    call = lambda n, m, d, dt, eps, it, out: lib.fad_sinkhorn(x.ctypes.data, n, 37, y.ctypes.data, m, 37, d, dt, 0, eps, it, out, None, 0, None)
    assert call(300, 200, 37, _capi.FAD_F32, 1.0, 10, C.byref(res)) == _capi.FAD_ERR_NO_DEVICE
    assert call(300, 200, 37, _capi.FAD_F64, 1.0, 10, C.byref(res)) == _capi.FAD_ERR_INVALID
    assert call(300, 200, 37, _capi.FAD_F32, 1.0, 0, C.byref(res)) == _capi.FAD_ERR_INVALID
    assert call(300, 200, 37, _capi.FAD_F32, 1.0, 100001, C.byref(res)) == _capi.FAD_ERR_INVALID
    assert call(300, 200, 37, _capi.FAD_F32, float("nan"), 10, C.byref(res)) == _capi.FAD_ERR_INVALID
    assert call(300, 200, 37, _capi.FAD_F32, 1.0, 10, None) == _capi.FAD_ERR_INVALID
    assert call(300, 200, 0, _capi.FAD_F32, 1.0, 10, C.byref(res)) == _capi.FAD_ERR_INVALID
    assert call(300, 200, 38, _capi.FAD_F32, 1.0, 10, C.byref(res)) == _capi.FAD_ERR_INVALID          # row pitch 37 < D
    assert call(0, 200, 37, _capi.FAD_F32, 1.0, 10, C.byref(res)) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(300, 0, 37, _capi.FAD_F32, 1.0, 10, C.byref(res)) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(1, 200, 37, _capi.FAD_F32, 0.0, 10, C.byref(res)) == _capi.FAD_ERR_TOO_FEW_ROWS       # no median of one row


# ---------------------------------------------------------------------------------------------------- CSV, command line
def test_csv_header_and_row(tmp_path):
    from fadtk_amd import sinkhorn
    assert sinkhorn.CSV_HEADER == "model,baseline,eval,n,m,divergence,w2_estimate,blur,epsilon,iterations,marginal_error,max_rows,seed\n"
    assert sinkhorn.INDIV_CSV_HEADER == "file,rows,mean_potential,share\n"
    res = {"divergence": 0.125, "w2_estimate": 0.5, "blur": 2.0, "epsilon": 4.0, "iterations": 100, "marginal_error": 0.25, "n": 20, "m": 30}
    row = sinkhorn.csv_row("vggish", "base", "evl", res, 1000, 7)
    assert row == "vggish,base,evl,20,30,0.125,0.5,2.0,4.0,100,0.25,1000,7"
    assert sinkhorn.csv_row("vggish", "base", "evl", res) == "vggish,base,evl,20,30,0.125,0.5,2.0,4.0,100,0.25,,"
    assert row.count(",") == sinkhorn.CSV_HEADER.count(",")
    target = tmp_path / "out" / "sinkhorn.csv"
    sinkhorn.append_csv(target, row)
    sinkhorn.append_csv(target, row)
    assert target.read_text() == sinkhorn.CSV_HEADER + row + "\n" + row + "\n"
    other = tmp_path / "other.csv"
    other.write_text("model,baseline,eval,kad\n")
    with pytest.raises(ValueError, match="another file"):
        sinkhorn.append_csv(other, row)
    with pytest.raises(ValueError, match="another file"):
        sinkhorn.check_csv(target, indiv=True)                                        # the summary CSV is no per-file CSV
    assert other.read_text() == "model,baseline,eval,kad\n"


def test_command_line_refuses_bad_arguments_before_any_work(tmp_path, capsys):
    from fadtk_amd import sinkhorn
    for bad in (["--blur", "0"], ["--blur-factor", "-1"], ["--blur", "1", "--blur-factor", "0.5"], ["--iterations", "0"],
                ["--iterations", "100001"], ["--max-rows", "0"], ["--indiv"]):
        with pytest.raises(SystemExit):
            sinkhorn.main(["vggish", "/nonexistent/base", "/nonexistent/eval", *bad])
    capsys.readouterr()
    other = tmp_path / "other.csv"
    other.write_text("model,baseline,eval,kad\n")
    with pytest.raises(ValueError, match="another file"):                              # before any file of the datasets is looked at
        sinkhorn.main(["vggish", "/nonexistent/base", "/nonexistent/eval", str(other)])


def test_warning_above_the_marginal_threshold(caplog):
    import logging
    from fadtk_amd import sinkhorn
    res = {"marginal_error": 2e-3, "iterations": 100, "blur": 1.5}
    with caplog.at_level(logging.WARNING, logger="fadtk_amd"):
        assert sinkhorn.warn_if_not_converged(res)
        assert not sinkhorn.warn_if_not_converged({**res, "marginal_error": 1e-3})
    text = " ".join(r.getMessage() for r in caplog.records)
    assert len(caplog.records) == 1 and "more iterations" in text and "larger" in text


def test_max_rows_is_repeatable_under_a_seed():
    from fadtk_amd.sinkhorn import subsample_rows
    x = np.arange(500 * 3, dtype=np.float32).reshape(500, 3)
    a, b = subsample_rows(x, 100, seed=4), subsample_rows(x, 100, seed=4)
    assert a.shape == (100, 3) and np.array_equal(a, b) and not np.array_equal(a, subsample_rows(x, 100, seed=5))
    idx = np.sort(np.random.default_rng(4).choice(500, 100, replace=False))           # the documented draw
    assert np.array_equal(a, x[idx]) and np.all(np.diff(a[:, 0]) > 0) and len(set(a[:, 0])) == 100
    assert subsample_rows(x, 500, seed=4) is x and subsample_rows(x, 900, seed=4) is x and subsample_rows(x, None) is x
