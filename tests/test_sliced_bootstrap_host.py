"""The sliced Wasserstein bootstrap without a GPU: the float64 reference of tests/sliced_bootstrap_reference.py on a
3 x 2 example by hand; ``bootstrap_counts`` (totals, files as blocks, empty files, streams, seeds); the interval statistics against
numpy; and the surface: the Python refusals before the native library is touched, exports and aliases, the CSV, the prototype, the
library's argument checks (they come before any device call)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sliced_bootstrap_reference as BR
import sliced_reference as SR

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------------------ the reference
def test_three_by_two_by_hand():
    """x = 0, 2, 5 and y = 1, 3 on the direction 1.  As given, the quantile functions differ by 1, 1, 1, 2 on [0, 1/3), [1/3, 1/2),
    [1/2, 2/3), [2/3, 1): W = 1/3 + 1/6 + 1/6 + 4/3 = 2.  With the counts 2, 0, 1 of x the resample is 0, 0, 5: differences 1, 1, 3, 2,
    W = 1/3 + 1/6 + 9/6 + 4/3 = 10/3.  With y resampled to 3, 3 as well: 0, 0, 5 against 3, 3 gives 9 (2/3) + 4 (1/3) = 22/3."""
    x, y = np.array([[0.0], [2.0], [5.0]], np.float32), np.array([[1.0], [3.0]], np.float32)
    t = np.ones((1, 1), np.float32)
    cx, cy = np.array([[2, 0, 1], [2, 0, 1]], np.uint8), np.array([[1, 1], [0, 2]], np.uint8)
    for ordered in (False, True):
        ref = BR.bootstrap(x, y, t, "fp32", cx, cy, ordered)
        assert ref["values"].shape == (3, 1) and ref["totals"].tolist() == [[3, 2], [3, 2], [3, 2]]
        assert np.allclose(ref["values"][:, 0], [2.0, 10.0 / 3.0, 22.0 / 3.0], rtol=1e-15)
        assert ref["sw2_squared"] == ref["values"][0, 0] and np.array_equal(ref["boot"], ref["values"][1:, 0])
        assert np.array_equal(ref["boot_max"], ref["boot"])
    same = BR.bootstrap(x, x, t, "fp32", cx, cx)
    assert np.all(same["values"] == 0)


def test_the_reference_is_repeat_then_the_plain_reference():
    x, y = SR.rows(40, 25, 6, "fp32")
    t = SR.directions(3, 6)
    cx, cy = BR.row_counts(40, 4), BR.row_counts(25, 4, seed=1)
    ref = BR.bootstrap(x, y, t, "fp32", cx, cy)
    assert np.array_equal(ref["values"][0], SR.sliced(x, y, t, "fp32")["values"])
    for b in range(4):
        one = SR.sliced(np.repeat(x, cx[b], axis=0), np.repeat(y, cy[b], axis=0), t, "fp32")
        assert np.array_equal(ref["values"][b + 1], one["values"]) and ref["boot"][b] == one["sw2_squared"]
        assert ref["totals"][b + 1].tolist() == [int(cx[b].sum()), int(cy[b].sum())]


# ------------------------------------------------------------------------------------------------------------ bootstrap_counts
def test_row_level_counts_sum_to_the_rows():
    from fadtk_amd.sliced import bootstrap_counts
    c = bootstrap_counts(np.ones(137, dtype=int), 25, seed=3, stream=0)
    assert c.dtype == np.uint8 and c.shape == (25, 137) and np.all(c.sum(axis=1) == 137)
    rng = np.random.default_rng([3, 0])
    for b in range(25):                                                                # the documented generator, replicate by replicate
        assert np.array_equal(c[b], np.bincount(rng.integers(0, 137, size=137), minlength=137))


def test_files_move_as_blocks_and_empty_files_are_never_drawn():
    from fadtk_amd.sliced import bootstrap_counts
    sizes = np.array([5, 0, 3, 1, 0, 7])
    c = bootstrap_counts(sizes, 40, seed=1, stream=2)
    assert c.shape == (40, 16)
    off = np.concatenate([[0], np.cumsum(sizes)])
    units = np.zeros((40, 4), dtype=int)
    for k, f in enumerate((0, 2, 3, 5)):
        block = c[:, off[f]:off[f + 1]]
        assert np.all(block == block[:, :1])                                           # one count per file
        units[:, k] = block[:, 0]
    assert np.all(units.sum(axis=1) == 4)                                              # 4 files in the pool, 4 draws
    assert len({int(t) for t in c.sum(axis=1)}) > 1                                    # the row totals differ from replicate to replicate
    rng = np.random.default_rng([1, 2])
    assert np.array_equal(units[0], np.bincount(rng.integers(0, 4, size=4), minlength=4))


def test_streams_and_seeds():
    from fadtk_amd.sliced import bootstrap_counts
    ones = np.ones(60, dtype=int)
    a, b, c = bootstrap_counts(ones, 10, 5, 0), bootstrap_counts(ones, 10, 5, 1), bootstrap_counts(ones, 10, 6, 0)
    assert np.array_equal(a, bootstrap_counts(ones, 10, 5, 0))                         # fixed by seed and stream
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    assert abs(np.corrcoef(a.ravel().astype(float), b.ravel().astype(float))[0, 1]) < 0.2     # 600 pairs: |r| < 0.2 is 4.9 sigma
    assert np.array_equal(a[:4], bootstrap_counts(ones, 4, 5, 0))                      # replicate by replicate, in order
    for bad in (dict(sizes=np.zeros(3, dtype=int)), dict(sizes=[[1, 2]]), dict(sizes=[1, -1]), dict(sizes=[1.5, 2]), dict(replicates=0),
                dict(replicates=65537), dict(seed=-1), dict(stream=-1), dict(stream=1.5)):
        with pytest.raises(ValueError):
            bootstrap_counts(**{"sizes": ones, "replicates": 3, "seed": 0, "stream": 0, **bad})


def test_the_baseline_stream_does_not_depend_on_the_evaluation_sets(monkeypatch):
    """compare draws the baseline once (stream 0) and hands the same array to every call; set k draws from stream 1 + k"""
    from fadtk_amd import sliced
    seen = []

    def fake(x, y, cx, cy, directions, device=0, per_replicate=False, stages=False):
        seen.append((cx.copy(), cy.copy(), np.array(directions)))
        B = len(cx)
        return {"sw2_squared": 1.0 + len(seen), "std_error": 0.0, "max_sliced": 2.0, "max_index": 0, "n": len(x), "m": len(y),
                "projections": len(directions), "replicates": B, "boot": np.arange(B) * float(len(seen)), "boot_max": np.zeros(B)}
    from fadtk_amd import hip
    monkeypatch.setattr(hip, "sliced_bootstrap", fake)
    x = np.zeros((30, 4), np.float32)
    ya, yb = np.zeros((20, 4), np.float32), np.zeros((45, 4), np.float32)
    xo = np.array([0, 10, 10, 30])
    res = sliced.calc_sliced_wasserstein_bootstrap_compare(x, [ya, yb], replicates=7, projections=3, seed=4, x_offsets=xo,
                                                           ys_offsets=[None, np.array([0, 40, 45])])
    assert len(seen) == 2 and np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][2], seen[1][2])
    assert np.array_equal(seen[0][0], sliced.bootstrap_counts(np.diff(xo), 7, 4, 0))
    assert np.array_equal(seen[0][1], sliced.bootstrap_counts(np.ones(20, dtype=int), 7, 4, 1))
    assert np.array_equal(seen[1][1], sliced.bootstrap_counts([40, 5], 7, 4, 2))
    assert [r["unit_y"] for r in res["sets"]] == ["row", "file"] and all(r["unit_x"] == "file" and r["unit"] == "file" for r in res["sets"])
    assert set(res["pairs"]) == {(0, 1)} and np.array_equal(res["pairs"][(0, 1)]["diff"], res["sets"][0]["boot"] - res["sets"][1]["boot"])
    assert res["pairs"][(0, 1)]["diff_observed"] == -1.0 and res["seed"] == 4 and res["sets"][0]["seed"] == 4


# ------------------------------------------------------------------------------------------------------------ statistics
def test_interval_statistics_against_numpy():
    from fadtk_amd.sliced import bootstrap_difference, bootstrap_statistics
    rng = np.random.default_rng(8)
    boot, other, obs = 2.0 + rng.gamma(3.0, 0.1, 400), 2.1 + rng.gamma(3.0, 0.1, 400), 2.2
    for c in (0.95, 0.5):
        got, want = bootstrap_statistics(boot, obs, c), BR.intervals(boot, obs, c)
        assert got["boot_mean"] == np.mean(boot) and got["boot_std"] == np.std(boot, ddof=1) and got["bias"] == np.mean(boot) - obs
        lo, hi = np.quantile(boot, [(1 - c) / 2, (1 + c) / 2])
        assert got["ci_percentile"] == (lo, hi) == tuple(want["ci_percentile"])
        assert got["ci_basic"] == (2 * obs - hi, 2 * obs - lo) == tuple(want["ci_basic"])
        assert got["ci_basic"][0] < got["ci_basic"][1]
        d, dw = bootstrap_difference(boot, other, obs, 2.5, c), BR.difference(boot, other, obs, 2.5, c)
        assert np.array_equal(d["diff"], boot - other) and d["diff_observed"] == obs - 2.5 == dw["diff_observed"]
        assert d["ci_diff"] == tuple(np.quantile(boot - other, [(1 - c) / 2, (1 + c) / 2])) == tuple(dw["ci_diff"])
        assert d["prob_closer"] == np.mean(boot < other) == dw["prob_closer"]
    assert np.isnan(bootstrap_statistics([1.0], 1.0)["boot_std"])
    for bad in (0.0, 1.0, -0.1, 1.5, True):
        with pytest.raises(ValueError, match="confidence"):
            bootstrap_statistics(boot, obs, bad)


# ------------------------------------------------------------------------------------------------------------ surface
def test_prototype_and_structures():
    from fadtk_amd import _capi
    res, args = _capi.SIGNATURES["fad_sliced_bootstrap"]
    assert res is C.c_int and len(args) == 20 and args[9:14] == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    assert _capi.SIGNATURES["fad_sliced_bootstrap_last_plan"] == (C.c_int, [C.POINTER(C.c_int64)])
    assert [f for f, _ in _capi.FadSlicedBootstrapDetail._fields_] == ["values", "sorted_x", "index_x", "sorted_y", "index_y", "totals"]
    assert [f for f, _ in _capi.FadSlicedBootstrapResult._fields_] == ["observed", "replicates"]
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert "int fad_sliced_bootstrap(" in header and "} fad_sliced_bootstrap_detail_t;" in header and "} fad_sliced_bootstrap_result_t;" in header
    assert "int fad_sliced_bootstrap_last_plan(int64_t out[6]);" in header
    declared = header.split("int fad_sliced_bootstrap(")[1].split(");")[0]
    assert re.sub(r"/\*.*?\*/", "", declared).count(",") + 1 == len(args)
    fields = header.split("typedef struct fad_sliced_bootstrap_detail {")[1].split("}")[0]
    assert re.findall(r"(\w+);", fields) == [f for f, _ in _capi.FadSlicedBootstrapDetail._fields_]


def test_library_exports_the_entries():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, "fad_sliced_bootstrap") and hasattr(lib, "fad_sliced_bootstrap_last_plan")
    names = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "fadtk_amd" / "lib" / "libfad_hip.so")], capture_output=True, text=True,
                           check=True).stdout.split()
    assert "fad_sliced_bootstrap" in names and "fad_sliced_bootstrap_last_plan" in names


def test_exports_and_aliases():
    import fadtk_amd
    import fadtk.sliced as alias
    import fadtk.sliced_bootstrap as alias_cli
    from fadtk_amd import sliced, sliced_bootstrap
    for name in ("calc_sliced_wasserstein_bootstrap", "calc_sliced_wasserstein_bootstrap_compare", "bootstrap_counts"):
        assert getattr(fadtk_amd, name) is getattr(sliced, name) and getattr(alias, name) is getattr(sliced, name)
    assert alias_cli.main is sliced_bootstrap.main and alias_cli.CSV_HEADER == sliced_bootstrap.CSV_HEADER
    assert hasattr(sliced.SlicedWasserstein, "score_bootstrap")
    assert sliced_bootstrap.CSV_HEADER == ("kind,model,baseline,eval,other,unit,n,m,sw2_squared,std_error,boot_mean,boot_std,bias,ci_lo,ci_hi,"
                                           "ci_basic_lo,ci_basic_hi,prob_closer,replicates,confidence,projections,seed\n")
    assert (sliced_bootstrap.SET_KIND, sliced_bootstrap.PAIR_KIND) == ("set", "pair")
    doc = sliced.calc_sliced_wasserstein_bootstrap.__doc__
    assert "biased UPWARD" in doc and "1/n + 1/m" in doc and "ci_basic" in doc
    assert "does NOT cancel" in sliced.calc_sliced_wasserstein_bootstrap_compare.__doc__


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, sliced

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    f = sliced.calc_sliced_wasserstein_bootstrap
    x, y = np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32)
    okx, oky = np.ones((3, 20), np.uint8), np.ones((3, 30), np.uint8)
    for bad in (0, -3, 65537, 2.5, True):
        with pytest.raises(ValueError, match="projections"):
            f(x, y, projections=bad, replicates=3)
        with pytest.raises(ValueError, match="replicates"):
            f(x, y, replicates=bad)
    for bad in (0.0, 1.0, 2):
        with pytest.raises(ValueError, match="confidence"):
            f(x, y, confidence=bad)
    with pytest.raises(ValueError, match="seed"):
        f(x, y, seed=-1, replicates=3)
    with pytest.raises(ValueError, match="different dimensions"):
        f(x, np.zeros((30, 5), np.float32), replicates=3)
    with pytest.raises(ValueError, match="at least 1 row"):
        f(x[:0], y, replicates=3)
    with pytest.raises(ValueError, match=r"directions must be \[L x 4\]"):
        f(x, y, directions=np.ones((3, 5), np.float32), replicates=3)
    with pytest.raises(ValueError, match="x_offsets"):
        f(x, y, x_offsets=[0, 5, 19], replicates=3)
    with pytest.raises(ValueError, match="y_offsets"):
        f(x, y, y_offsets=[1, 30], replicates=3)
    for bad in (np.ones(20, np.uint8), np.ones((3, 19), np.uint8), np.ones((3, 20), np.int32), np.ones((3, 20), bool),
                np.ones((0, 20), np.uint8), np.ones((2, 3, 20), np.uint8), [[1] * 20] * 3):
        with pytest.raises(ValueError, match="counts_x|replicates"):
            f(x, y, counts_x=bad, counts_y=oky)
    with pytest.raises(ValueError, match="counts_y"):
        f(x, y, counts_x=okx, counts_y=np.ones((3, 31), np.uint8))
    with pytest.raises(ValueError, match="3 replicates, counts_y has 4"):
        f(x, y, counts_x=okx, counts_y=np.ones((4, 30), np.uint8))
    g = sliced.calc_sliced_wasserstein_bootstrap_compare
    with pytest.raises(ValueError, match="at least 1 evaluation set"):
        g(x, [])
    with pytest.raises(ValueError, match="2 sets, 1 offsets"):
        g(x, [y, y], ys_offsets=[None])
    with pytest.raises(ValueError, match="different dimensions"):
        g(x, [y, np.zeros((30, 5), np.float32)], replicates=3)


def _set_result(sw2, boot, unit="file", m=57):
    from fadtk_amd.sliced import bootstrap_statistics
    return {"n": 123, "m": m, "sw2_squared": sw2, "std_error": 0.125, "unit": unit, "replicates": len(boot), "confidence": 0.5,
            "projections": 16, "seed": 2, "boot": np.array(boot), **bootstrap_statistics(boot, sw2, 0.5)}


def test_csv_header_and_its_refusal(tmp_path):
    from fadtk_amd import sliced, sliced_bootstrap as sb
    a, b = _set_result(0.25, [0.5, 0.25, 0.75, 1.0, 0.5]), _set_result(0.5, [0.75, 0.75, 0.5, 1.5, 1.0], m=60)
    res = {"sets": [a, b], "pairs": {(0, 1): sliced.bootstrap_difference(a["boot"], b["boot"], 0.25, 0.5, 0.5)}}
    rows = sb.csv_rows("vggish", "base", ["evA", "evB"], res)
    target = tmp_path / "sub" / "boot.csv"
    for _ in range(2):
        sb.append_csv(target, rows)
    lines = target.read_text().splitlines()
    assert lines[0] + "\n" == sb.CSV_HEADER and len(lines) == 7 and lines[1:4] == lines[4:7]
    assert all(len(ln.split(",")) == len(sb.CSV_HEADER.split(",")) for ln in lines)
    cells = [dict(zip(sb.CSV_HEADER.strip().split(","), ln.split(","))) for ln in lines[1:4]]
    assert [c["kind"] for c in cells] == ["set", "set", "pair"] and [c["eval"] for c in cells] == ["evA", "evB", "evA"]
    assert cells[2]["other"] == "evB" and cells[0]["other"] == "" and cells[0]["prob_closer"] == ""
    std = repr(float(np.std(a["boot"], ddof=1)))                                       # sqrt(0.08125), not a short decimal
    assert lines[1] == f"set,vggish,base,evA,,file,123,57,0.25,0.125,0.6,{std},0.35,0.5,0.75,-0.25,0.0,,5,0.5,16,2"
    assert lines[3] == "pair,vggish,base,evA,evB,file,123,,-0.25,,,,,-0.5,-0.25,,,0.8,5,0.5,16,2"
    other = tmp_path / "sliced.csv"
    other.write_text(sliced.CSV_HEADER)
    with pytest.raises(ValueError, match="another file"):
        sb.append_csv(other, rows)
    with pytest.raises(ValueError, match="another file"):                              # before any file is read or embedded
        sb.main(["vggish", str(tmp_path / "none"), str(tmp_path / "none2"), "--csv", str(other)])
    assert other.read_text() == sliced.CSV_HEADER


def test_argument_errors_of_the_command_line():
    from fadtk_amd import sliced_bootstrap as sb
    for bad in (["-b", "0"], ["-b", "65537"], ["--projections", "0"], ["--seed", "-1"], ["--confidence", "1"], ["--confidence", "0"],
                ["--confidence", "x"], ["--rows", "3", "--bogus"]):
        with pytest.raises(SystemExit):
            sb.main(["vggish", "a", "b", *bad])
    with pytest.raises(SystemExit):
        sb.main(["vggish", "a"])                                                       # no evaluation directory
    with pytest.raises(SystemExit):
        sb.main(["no-such-model", "a", "b"])


def test_without_a_gpu_the_entry_fails_loudly():
    import torch
    from fadtk_amd import _capi, sliced
    x, y = SR.rows(30, 20, 8, "fp32")
    if torch.cuda.is_available():                                                      # tests/test_gpu_sliced_bootstrap.py has the rest
        assert sliced.calc_sliced_wasserstein_bootstrap(x, y, replicates=5, projections=4)["replicates"] == 5
        return
    with pytest.raises(_capi.FadHipUnavailable):
        sliced.calc_sliced_wasserstein_bootstrap(x, y, replicates=5, projections=4)


def test_argument_errors_before_any_device_call():
    """the library's own refusals need no GPU: they come before the device is opened (FAD_ERR_NO_DEVICE where there is none)"""
    import torch
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(30, 20, 37, "fp32")
    t = SR.directions(4, 37)
    cx, cy = BR.row_counts(30, 5), BR.row_counts(20, 5, seed=1)
    res = _capi.FadSlicedBootstrapResult()
    res.observed.sw2_squared, res.replicates = -7.0, 99
    boot, boot_max, vals, tot = np.full(5, -7.0), np.full(5, -7.0), np.full((6, 4), -7.0), np.full((6, 2), -7, np.int64)
    sx, ix = np.full((4, 30), -7.0, np.float32), np.full((4, 30), -7, np.int32)
    sy, iy = np.full((4, 20), -7.0, np.float32), np.full((4, 20), -7, np.int32)
    det = _capi.FadSlicedBootstrapDetail(vals.ctypes.data, sx.ctypes.data, ix.ctypes.data, sy.ctypes.data, iy.ctypes.data, tot.ctypes.data)
    ptr = lambda a: a.ctypes.data if a is not None else None                           # noqa: E731

    def call(n=30, m=20, d=37, dt=_capi.FAD_F32, th=t, L=4, out=C.byref(res), ld=37, ca=cx, cb=cy, B=5, bt=boot, bm=boot_max, xa=x):
        return lib.fad_sliced_bootstrap(ptr(xa), n, ld, y.ctypes.data, m, ld, d, dt, 0, ptr(th), L, ptr(ca), ptr(cb), B, out, ptr(bt), ptr(bm),
                                        C.byref(det), 0, None)
    INVALID, TOO_FEW = _capi.FAD_ERR_INVALID, _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(dt=_capi.FAD_F64) == INVALID and call(xa=None) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID and call(d=37, ld=36) == INVALID
    assert call(L=0) == INVALID and call(L=65537) == INVALID
    assert call(out=None) == INVALID and call(th=None) == INVALID and call(bt=None) == INVALID and call(bm=None) == INVALID
    assert call(ca=None) == INVALID and call(cb=None) == INVALID and call(B=0) == INVALID and call(B=65537) == INVALID
    assert call(n=0) == TOO_FEW and call(m=0) == TOO_FEW
    assert call(n=2 ** 31 - 128, m=20) == INVALID                                      # more rows than a set may have
    assert call(n=2 ** 27, m=2 ** 26) == INVALID                                       # n m = 2^53
    tb = t.copy()
    tb[2, 5] = np.nan
    assert call(th=tb) == INVALID
    tz = t.copy()
    tz[1] = 0
    assert call(th=tz) == INVALID                                                      # q = 0
    none = cx.copy()
    none[3] = 0
    assert call(ca=none) == INVALID and "fad_sliced_bootstrap: replicate 3 takes no row of x" in _capi.last_error()
    none = cy.copy()
    none[1] = 0
    assert call(cb=none) == INVALID and "replicate 1 takes no row of y" in _capi.last_error()
    # totals are checked on the counts alone: rows that do not exist are never read before a refusal
    many = np.full((1, 2 ** 24), 255, np.uint8)                                        # 255 x 2^24 > 2^31 - 129
    assert call(n=2 ** 24, ca=many, B=1) == INVALID and "at most" in _capi.last_error()
    wide_x, wide_y = np.full((1, 2 ** 20), 128, np.uint8), np.full((1, 2 ** 20), 64, np.uint8)     # n_b m_b = 2^27 x 2^26 = 2^53
    assert call(n=2 ** 20, m=2 ** 20, ca=wide_x, cb=wide_y, B=1) == INVALID and "2^53" in _capi.last_error()
    assert res.observed.sw2_squared == -7.0 and res.replicates == 99
    for a in (boot, boot_max, vals, sx, sy):
        assert np.all(a == -7.0)
    assert np.all(ix == -7) and np.all(iy == -7) and np.all(tot == -7)
    plan = (C.c_int64 * 6)(9, 9, 9, 9, 9, 9)
    assert lib.fad_sliced_bootstrap_last_plan(plan) == 0 and list(plan) == [0] * 6
    assert lib.fad_sliced_bootstrap_last_plan(None) == INVALID
    if not torch.cuda.is_available():
        assert call() == _capi.FAD_ERR_NO_DEVICE
