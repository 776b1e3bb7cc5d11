"""The sliced Wasserstein distance without a GPU: the float64 reference of tests/sliced_reference.py checked against what the definition
implies -- the overlap weights against replication to lcm(n, m), their sum, symmetry, exact integers -- and the Python
layer of fadtk_amd/sliced.py: the pinned directions, its refusals before the native library is touched, the CSV, the prototype.  The
library's argument checks (the rounding of the directions among them) run here too: they come before any device call."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

import sliced_reference as SR

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((1, 7), (7, 1), (6, 4), (33, 32), (64, 128), (257, 130), (130, 257))


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n,m", SHAPES)
def test_overlap_form_equals_replication(n, m):
    rng = np.random.default_rng([n, m])
    a, b = np.sort(rng.integers(-50, 51, n)).astype(np.float64), np.sort(rng.integers(-50, 51, m)).astype(np.float64)
    want = SR.replicated_sum(a, b)                                                     # integers: every sum is exact
    assert SR.match_sum(a, b) == want and SR.match_sum_ordered(a, b) == want


@pytest.mark.parametrize("n,m", SHAPES + ((5, 5), (255, 257), (300, 1), (70001, 33333)))
def test_weights(n, m):
    i, j, w = SR.overlap(n, m)
    assert w.min() > 0 and int(w.sum()) == n * m
    assert np.array_equal(np.bincount(i, weights=w), np.full(n, float(m))) and np.array_equal(np.bincount(j, weights=w), np.full(m, float(n)))
    per_i = np.bincount(i)
    assert per_i.max() <= -(-m // n) + 1                                               # at most ceil(ratio) + 1 partners
    if n == m:
        assert np.array_equal(i, j) and np.all(w == n)


def test_two_partners_at_257_against_130():
    i, j, w = SR.overlap(257, 130)
    assert np.bincount(i).max() == 2


@pytest.mark.parametrize("n,m", SHAPES)
def test_symmetry(n, m):
    rng = np.random.default_rng([3, n, m])
    a, b = np.sort(rng.standard_normal(n)), np.sort(rng.standard_normal(m))
    assert SR.match_sum_ordered(a, b) == SR.match_sum_ordered(b, a)                    # the larger set leads either way: the same bits
    assert abs(SR.match_sum(a, b) - SR.match_sum(b, a)) <= (n + m) * 2.0 ** -52 * SR.match_sum(a, b)
    assert abs(SR.match_sum(a, b) - SR.match_sum_ordered(a, b)) <= (n + m) * 2.0 ** -52 * SR.match_sum(a, b)


def test_exact_integers_on_integer_inputs():
    x, y = SR.exact_rows(257, 130, 64)
    t = SR.exact_directions(5, 64)
    for dt in SR.DTYPES:
        assert np.array_equal(SR.round_to_dtype(x, dt), x) and np.array_equal(SR.round_to_dtype(t, dt), t)
    r = SR.sliced(x, y, t, "fp16")
    assert np.array_equal(r["sorted_x"], r["sorted_x"].astype(np.float32))             # every projection is a float32 value
    scaled = r["sorted_x"] * 256.0
    assert np.array_equal(scaled, np.rint(scaled))                                     # a multiple of 2^-8
    assert np.array_equal(r["q"], np.rint(r["q"]))
    xi, yi = np.rint(np.clip(x, -8, 8)), np.rint(np.clip(y, -8, 8))                    # integer inputs proper: S is an exact integer
    ri = SR.sliced(xi, yi, t, "fp32")
    for l in range(5):
        s = SR.match_sum(ri["sorted_x"][l], ri["sorted_y"][l])
        assert s == round(s) and s == SR.match_sum_ordered(ri["sorted_x"][l], ri["sorted_y"][l])


def test_translation_and_identity():
    x, _ = SR.rows(300, 1, 37, "fp32")
    x = np.rint(x * 16) / 16                                                           # so that x + 4 is exact
    t = SR.directions(3, 37)
    t[0] = 0
    t[0, 0] = 1.0
    r = SR.sliced(x, x.copy(), t, "fp32")
    assert np.all(r["values"] == 0) and r["sw2_squared"] == 0.0
    y = x.copy()
    y[:, 0] += 4.0
    assert SR.sliced(x, y, t, "fp32")["values"][0] == 16.0


def test_statistics_in_index_order():
    v = np.array([3.0, 1.0, 7.0, 7.0, 2.0])
    mean, se, mx, k = SR.statistics(v)
    assert mean == 4.0 and mx == 7.0 and k == 2 and abs(se - np.std(v, ddof=1) / math.sqrt(5)) <= 1e-15
    assert math.isnan(SR.statistics(v[:1])[1])


def test_round_to_dtype():
    a = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 70000.0, 2.0 ** -25, 3 * 2.0 ** -25], np.float32)
    assert np.array_equal(SR.round_to_dtype(a, "fp16")[:2], np.array([1.0, 1.0 + 2.0 ** -9], np.float32))          # ties to even
    assert np.isinf(SR.round_to_dtype(a, "fp16")[4]) and SR.round_to_dtype(a, "fp16")[5] == 0 and SR.round_to_dtype(a, "fp16")[6] == 2.0 ** -23
    assert np.array_equal(SR.round_to_dtype(a, "bf16")[2:4], np.array([1.0, 1.0 + 2.0 ** -6], np.float32))
    assert np.array_equal(SR.round_to_dtype(a, "fp32"), a)


# ------------------------------------------------------------------------------------------------------------ surface
def test_directions_pinned():
    from fadtk_amd import sliced
    t = sliced.sliced_directions(5, 3, seed=0)
    assert t.dtype == np.float32 and t.shape == (3, 5)
    assert np.array_equal(t, np.random.default_rng(0).standard_normal((3, 5)).astype(np.float32))
    assert np.array_equal(t[0, :3], np.array([0.12573022, -0.13210486, 0.64042264], np.float32))
    assert not np.array_equal(t, sliced.sliced_directions(5, 3, seed=1))


def test_prototype_and_structures():
    from fadtk_amd import _capi
    res, args = _capi.SIGNATURES["fad_sliced_wasserstein"]
    assert res is C.c_int and len(args) == 15 and args[9:11] == [C.c_void_p, C.c_int]
    assert [f for f, _ in _capi.FadSlicedResult._fields_] == ["sw2_squared", "std_error", "max_sliced", "max_index", "n", "m", "projections"]
    assert [f for f, _ in _capi.FadSlicedDetail._fields_] == ["values", "sorted_x", "sorted_y"]
    assert "fad_sliced_last_plan" in _capi.SIGNATURES
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert "int fad_sliced_wasserstein(" in header and "fad_sliced_detail_t" in header and "FAD_SLICED_WORKSPACE" in header
    assert "int fad_sliced_last_plan(int64_t out[4]);" in header


def test_library_exports_the_entry():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, "fad_sliced_wasserstein") and hasattr(lib, "fad_sliced_last_plan") and lib.fad_version() == 2


def test_exports_and_alias():
    import fadtk_amd
    import fadtk.sliced as alias
    from fadtk_amd import sliced
    assert fadtk_amd.calc_sliced_wasserstein is sliced.calc_sliced_wasserstein
    assert fadtk_amd.SlicedWasserstein is sliced.SlicedWasserstein and fadtk_amd.sliced_directions is sliced.sliced_directions
    assert alias.calc_sliced_wasserstein is sliced.calc_sliced_wasserstein and alias.main is sliced.main
    assert alias.SlicedWasserstein is sliced.SlicedWasserstein and alias.CSV_HEADER == sliced.CSV_HEADER


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, sliced

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    x, y = np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32)
    for bad in (0, -3, 65537, 2.5, True):
        with pytest.raises(ValueError, match="projections"):
            sliced.calc_sliced_wasserstein(x, y, projections=bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            sliced.calc_sliced_wasserstein(x, y, seed=bad)
    with pytest.raises(ValueError, match="different dimensions"):
        sliced.calc_sliced_wasserstein(x, np.zeros((30, 5), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        sliced.calc_sliced_wasserstein(x[0], y)
    with pytest.raises(ValueError, match="at least 1 row"):
        sliced.calc_sliced_wasserstein(x[:0], y)
    with pytest.raises(ValueError, match="outside 1 .. 2048"):
        sliced.calc_sliced_wasserstein(np.zeros((3, 2049), np.float32), np.zeros((3, 2049), np.float32))
    with pytest.raises(ValueError, match=r"directions must be \[L x 4\]"):
        sliced.calc_sliced_wasserstein(x, y, directions=np.ones((3, 5), np.float32))
    with pytest.raises(ValueError, match="not finite"):
        sliced.calc_sliced_wasserstein(x, y, directions=np.array([[1.0, np.nan, 0.0, 0.0]]))
    with pytest.raises(ValueError, match="outside 1 .. 65536"):
        sliced.calc_sliced_wasserstein(x, y, directions=np.ones((0, 4), np.float32))
    with pytest.raises(ValueError, match="projections"):
        sliced.SlicedWasserstein(None, projections=0)


def test_csv(tmp_path):
    from fadtk_amd import sliced
    res = {"sw2_squared": 0.25, "sliced_w2": 0.5, "std_error": 0.125, "max_sliced": 1.5, "max_index": 3, "fad_scale": 32.0, "n": 10, "m": 20,
           "projections": 8, "seed": 0}
    target = tmp_path / "sub" / "sliced.csv"
    sliced.append_csv(target, sliced.csv_row("vggish", "a", "b", res))
    sliced.append_csv(target, sliced.csv_row("vggish", "a", "c", dict(res, seed=None)))
    lines = target.read_text().splitlines()
    assert lines[0] + "\n" == sliced.CSV_HEADER and lines[1] == "vggish,a,b,10,20,0.25,0.5,0.125,1.5,3,32.0,8,0" and lines[2].endswith(",8,")
    assert len(lines[1].split(",")) == len(sliced.CSV_HEADER.split(","))
    other = tmp_path / "kad.csv"
    other.write_text("model,baseline,eval,kad\n")
    with pytest.raises(ValueError, match="another file"):
        sliced.append_csv(other, "x")
    assert other.read_text() == "model,baseline,eval,kad\n"


def test_argument_errors_before_any_device_call():
    """the library's own refusals need no GPU: they come before the device is opened (FAD_ERR_NO_DEVICE where there is none)"""
    import torch
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(30, 20, 37, "fp32")
    t = SR.directions(4, 37)
    res = _capi.FadSlicedResult()
    res.sw2_squared = -7.0
    vals = np.full(4, -7.0)
    det = _capi.FadSlicedDetail(vals.ctypes.data, None, None)

    def call(n=30, m=20, d=37, dt=_capi.FAD_F32, th=t, L=4, out=C.byref(res), ld=37):
        return lib.fad_sliced_wasserstein(x.ctypes.data, n, ld, y.ctypes.data, m, ld, d, dt, 0, th.ctypes.data if th is not None else None, L,
                                          out, C.byref(det), 0, None)
    INVALID, TOO_FEW = _capi.FAD_ERR_INVALID, _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(dt=_capi.FAD_F64) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID
    assert call(d=37, ld=36) == INVALID                                                # row pitch < D
    assert call(L=0) == INVALID and call(L=65537) == INVALID
    assert call(out=None) == INVALID and call(th=None) == INVALID
    assert call(n=0) == TOO_FEW and call(m=0) == TOO_FEW
    assert call(n=2 ** 27, m=2 ** 26) == INVALID                                       # n m = 2^53
    for bad in (np.nan, np.inf):
        tb = t.copy()
        tb[2, 5] = bad
        assert call(th=tb) == INVALID
    tz = t.copy()
    tz[1] = 0
    assert call(th=tz) == INVALID                                                      # q = 0
    tz[1, 0] = 1e-9
    assert call(th=tz, dt=_capi.FAD_F16) == INVALID                                    # rounds to a zero direction in float16
    tz[1, 0] = 70000.0
    assert call(th=tz, dt=_capi.FAD_F16) == INVALID                                    # rounds to infinity in float16
    assert res.sw2_squared == -7.0 and np.all(vals == -7.0)                            # every refusal leaves the outputs as they were
    plan = (C.c_int64 * 4)(9, 9, 9, 9)
    assert lib.fad_sliced_last_plan(plan) == 0 and list(plan) == [0, 0, 0, 0]
    if not torch.cuda.is_available():
        assert call() == _capi.FAD_ERR_NO_DEVICE
