"""The per-song sliced Wasserstein distance (fad_sliced_individual) without a GPU: the prototype, the header and the
built library's symbols; the Python layer's refusals before the native library is touched; the per-song CSV; the alias package; and the
library's own argument refusals, which come before any device call and leave sentinel-filled outputs and an all-zero plan."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import sliced_reference as SR

ROOT = Path(__file__).resolve().parent.parent


def test_prototype_header_and_symbols():
    from fadtk_amd import _capi
    res, args = _capi.SIGNATURES["fad_sliced_individual"]
    assert res is C.c_int and len(args) == 21 and args[6] == C.POINTER(C.c_int64) and args[11:13] == [C.c_void_p, C.c_int]
    assert args[18] == C.POINTER(_capi.FadSlicedIndividualDetail) and args[19:] == [C.c_int, C.c_void_p]
    assert _capi.SIGNATURES["fad_sliced_individual_last_plan"] == (C.c_int, [C.POINTER(C.c_int64)])
    assert [f for f, _ in _capi.FadSlicedIndividualDetail._fields_] == ["values", "sorted_x", "sorted_rows"]
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert "int fad_sliced_individual(" in header and "fad_sliced_individual_detail_t" in header
    assert "int fad_sliced_individual_last_plan(int64_t out[6]);" in header
    assert "int fad_sliced_last_plan(int64_t out[4]);" in header                       # the whole-set entry is as it was
    lib = _capi.load_library()
    assert hasattr(lib, "fad_sliced_individual") and hasattr(lib, "fad_sliced_individual_last_plan") and lib.fad_version() == 2


def test_exports_and_alias():
    import fadtk_amd
    import fadtk.sliced as alias
    from fadtk_amd import sliced
    assert fadtk_amd.calc_sliced_wasserstein_individual is sliced.calc_sliced_wasserstein_individual
    assert alias.calc_sliced_wasserstein_individual is sliced.calc_sliced_wasserstein_individual
    assert alias.INDIV_CSV_HEADER == sliced.INDIV_CSV_HEADER == "file,rows,sw2_squared,sliced_w2,std_error,fad_scale\n"
    assert alias.write_indiv_csv is sliced.write_indiv_csv and sliced.INDIV_CSV_NAME == "sliced-individual-results.csv"
    assert hasattr(sliced.SlicedWasserstein, "score_individual")


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, sliced

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    f = sliced.calc_sliced_wasserstein_individual
    x, songs = np.zeros((20, 4), np.float32), [np.zeros((3, 4), np.float32), np.zeros((0, 4), np.float32)]
    for bad in (0, -3, 65537, 2.5, True):
        with pytest.raises(ValueError, match="projections"):
            f(x, songs, projections=bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            f(x, songs, seed=bad)
    with pytest.raises(ValueError, match="2-D baseline"):
        f(x[0], songs)
    with pytest.raises(ValueError, match="at least 1 baseline row"):
        f(x[:0], songs)
    with pytest.raises(ValueError, match="at least 1 song"):
        f(x, [])
    with pytest.raises(ValueError, match="a song of shape"):
        f(x, [np.zeros((3, 5), np.float32)])
    with pytest.raises(ValueError, match="a song of shape"):
        f(x, [np.zeros(4, np.float32)])
    with pytest.raises(ValueError, match="outside 1 .. 2048"):
        f(np.zeros((3, 2049), np.float32), [np.zeros((3, 2049), np.float32)])
    with pytest.raises(ValueError, match=r"directions must be \[L x 4\]"):
        f(x, songs, directions=np.ones((3, 5), np.float32))
    with pytest.raises(ValueError, match="not finite"):
        f(x, songs, directions=np.array([[1.0, np.nan, 0.0, 0.0]]))


def test_per_song_csv(tmp_path):
    from fadtk_amd import sliced
    res = {"rows": np.array([3.0, 7.0, 2.0, 5.0]), "sw2_squared": np.array([0.25, 4.0, np.nan, 1.0]),
           "sliced_w2": np.array([0.5, 2.0, np.nan, 1.0]), "std_error": np.array([0.125, 0.5, np.nan, np.nan]),
           "fad_scale": np.array([32.0, 512.0, np.nan, 128.0]), "status": np.array([0.0, 0.0, -7.0, 0.0])}
    assert sliced.indiv_csv_row("a,b.wav", res, 0) == "a_b.wav,3,0.25,0.5,0.125,32.0"
    target = tmp_path / "sub" / "indiv.csv"
    assert sliced.write_indiv_csv(target, ["a.wav", "b.wav", "c.wav", "d.wav"], res) == 3
    lines = target.read_text().splitlines()
    assert lines[0] + "\n" == sliced.INDIV_CSV_HEADER
    assert lines[1:] == ["b.wav,7,4.0,2.0,0.5,512.0", "d.wav,5,1.0,1.0,nan,128.0", "a.wav,3,0.25,0.5,0.125,32.0"]   # descending; c dropped
    assert all(len(ln.split(",")) == len(sliced.INDIV_CSV_HEADER.split(",")) for ln in lines)
    assert sliced.write_indiv_csv(target, ["a.wav"], {k: v[:1] for k, v in res.items()}) == 1                     # replaced, not appended
    assert len(target.read_text().splitlines()) == 2
    for header in ("model,baseline,eval,kad\n", sliced.CSV_HEADER):                    # a foreign CSV, the whole-set CSV: refused, untouched
        other = tmp_path / "other.csv"
        other.write_text(header)
        with pytest.raises(ValueError, match="another file"):
            sliced.write_indiv_csv(other, ["a.wav"], res)
        assert other.read_text() == header
    with pytest.raises(ValueError, match="another file"):
        sliced.append_csv(target, "x")                                                 # and the other way round


def test_command_line_refuses_a_foreign_csv_before_any_work(tmp_path):
    from fadtk_amd import sliced
    other = tmp_path / "kad.csv"
    other.write_text("model,baseline,eval,kad\n")
    with pytest.raises(ValueError, match="another file"):
        sliced.main(["vggish", str(tmp_path / "none"), str(tmp_path / "none2"), str(other), "--indiv"])
    assert other.read_text() == "model,baseline,eval,kad\n"


def test_argument_errors_before_any_device_call():
    """the library's own refusals need no GPU: they come before the device is opened (FAD_ERR_NO_DEVICE where there is none)"""
    import torch
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(30, 20, 37, "fp32")
    t = SR.directions(4, 37)
    good = np.array([0, 5, 5, 20], np.int64)
    outs = [np.full(3, -7.0) for _ in range(3)]
    idx, status = np.full(3, 99, np.int64), np.full(3, 55, np.int32)
    vals = np.full((3, 4), -7.0)
    det = _capi.FadSlicedIndividualDetail(vals.ctypes.data, None, None)
    I64P = C.POINTER(C.c_int64)

    def call(xa=x.ctypes.data, n=30, rows=y.ctypes.data, n_rows=20, off=good, S=3, d=37, dt=_capi.FAD_F32, th=t, L=4, ldx=37, ldy=37,
             sw2=outs[0].ctypes.data, st=status.ctypes.data):
        return lib.fad_sliced_individual(xa, n, ldx, rows, n_rows, ldy, off.ctypes.data_as(I64P) if off is not None else None, S, d, dt, 0,
                                         th.ctypes.data if th is not None else None, L, sw2, outs[1].ctypes.data, outs[2].ctypes.data,
                                         idx.ctypes.data, st, C.byref(det), 0, None)
    INVALID, TOO_FEW = _capi.FAD_ERR_INVALID, _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(dt=_capi.FAD_F64) == INVALID and call(dt=17) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ldx=2049, ldy=2049) == INVALID
    assert call(ldx=36) == INVALID and call(ldy=36) == INVALID                          # a row pitch < D
    assert call(L=0) == INVALID and call(L=65537) == INVALID
    assert call(xa=None) == INVALID and call(rows=None) == INVALID and call(off=None) == INVALID and call(th=None) == INVALID
    assert call(sw2=None) == INVALID and call(st=None) == INVALID
    assert call(n=0) == TOO_FEW and call(S=0) == INVALID and call(n_rows=-1) == INVALID and call(n_rows=2 ** 31 - 128) == INVALID
    assert call(off=np.array([1, 5, 5, 20], np.int64)) == INVALID                       # does not start at 0
    assert call(off=np.array([0, 5, 5, 19], np.int64)) == INVALID                       # does not end at n_rows
    assert call(off=np.array([0, 9, 5, 20], np.int64)) == INVALID                       # decreases
    big = np.array([0, 2 ** 26, 2 ** 26 + 3], np.int64)
    assert call(n=2 ** 27, n_rows=2 ** 26 + 3, off=big, S=2) == INVALID                 # n m_0 = 2^53
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
    assert all(np.all(o == -7.0) for o in outs) and np.all(idx == 99) and np.all(status == 55) and np.all(vals == -7.0)
    plan = (C.c_int64 * 6)(9, 9, 9, 9, 9, 9)
    assert lib.fad_sliced_individual_last_plan(plan) == 0 and list(plan) == [0] * 6
    assert lib.fad_sliced_individual_last_plan(None) == INVALID
    if not torch.cuda.is_available():
        assert call() == _capi.FAD_ERR_NO_DEVICE
        assert all(np.all(o == -7.0) for o in outs) and np.all(status == 55)
