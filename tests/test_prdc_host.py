"""Precision, recall, density and coverage, host side (no GPU): the float64 reference against brute-force loops, the unit map of the
passes (checked with g++), the C ABI surface, the errors raised before any library call, and the command line."""
import ctypes as C
import importlib.util
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("prdc_reference", Path(__file__).resolve().parent / "prdc_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def _brute(x, y, k):
    n, m = len(x), len(y)

    def d2(a, b):
        return float(sum((float(p) - float(q)) ** 2 for p, q in zip(a, b)))

    def radius(a, i):
        return sorted(d2(a[i], a[j]) for j in range(len(a)) if j != i)[k - 1]
    rx = [radius(x, i) for i in range(n)]
    ry = [radius(y, j) for j in range(m)]
    balls = [sum(d2(x[i], y[j]) < rx[i] for i in range(n)) for j in range(m)]
    rec = [any(d2(x[i], y[j]) < ry[j] for j in range(m)) for i in range(n)]
    cov = [any(d2(x[i], y[j]) < rx[i] for j in range(m)) for i in range(n)]
    return {"radius2_x": rx, "radius2_y": ry, "balls_y": balls, "flags_x": [int(a) | 2 * int(b) for a, b in zip(rec, cov)],
            "precision": sum(b > 0 for b in balls) / m, "recall": sum(rec) / n, "density": sum(balls) / (k * m),
            "coverage": sum(cov) / n}


@pytest.mark.parametrize("k", [1, 2, 5])
def test_reference_matches_brute_force_loops(k):
    rng = np.random.default_rng(11 + k)
    x = rng.integers(-2, 3, size=(13, 3)).astype(np.float64)
    y = rng.integers(-2, 3, size=(11, 3)).astype(np.float64) + (rng.random((11, 3)) < 0.3)
    x[5] = x[2]                                      # duplicate rows: neighbours at distance 0, self excluded by index only
    x[9] = x[2]
    y[4] = y[1]
    y[7] = x[3]                                      # a y row on top of an x row
    want = _brute(x, y, k)
    got = R.prdc(x, y, k)
    for key in ("radius2_x", "radius2_y", "balls_y", "flags_x"):
        assert list(got[key]) == list(want[key]), key
    for key in ("precision", "recall", "density", "coverage"):
        assert got[key] == want[key], key
    br = R.bracket(x, y, k, 0.0)                     # no margin: the bracket closes on the exact value
    for key in ("precision", "recall", "density", "coverage"):
        assert br[f"{key}_lo"] == br[f"{key}_hi"] == want[key], key


def test_bracket_widens_with_the_margin():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((60, 8))
    y = rng.standard_normal((50, 8)) * 1.1 + 0.2
    exact = R.prdc(x, y, 3)
    br = R.bracket(x, y, 3, 1e-3)
    assert (br["balls_lo"] <= exact["balls_y"]).all() and (exact["balls_y"] <= br["balls_hi"]).all()
    for key in ("precision", "recall", "density", "coverage"):
        assert br[f"{key}_lo"] <= exact[key] <= br[f"{key}_hi"], key
    assert (br["balls_hi"] - br["balls_lo"]).sum() > 0


def test_prdc_unit_map_covers_every_tile_once(tmp_path):
    exe = tmp_path / "prdc_tiles_cover"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "native_cpu" / "prdc_tiles_cover.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("OK"), r.stdout


def test_header_declares_and_capi_binds_prdc():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_prdc\s*\(", text)
    assert "fad_prdc_result_t" in text and "fad_prdc_detail_t" in text
    _capi, lib = _lib()
    assert "fad_prdc" in _capi.SIGNATURES and hasattr(lib, "fad_prdc")
    assert [f for f, _ in _capi.FadPrdcResult._fields_] == ["precision", "recall", "density", "coverage", "n", "m", "k"]
    assert C.sizeof(_capi.FadPrdcResult) == 4 * 8 + 3 * 8
    assert [f for f, _ in _capi.FadPrdcDetail._fields_] == ["radius2_x", "radius2_y", "balls_y", "flags_x"]


def test_prdc_argument_errors_come_before_the_device():
    _capi, lib = _lib()
    x = np.random.default_rng(0).standard_normal((16, 8)).astype(np.float16)
    res = _capi.FadPrdcResult()

    def call(n=16, m=16, k=5, dtype=_capi.FAD_F16, d=8, ld=8):
        return lib.fad_prdc(x.ctypes.data, n, ld, x.ctypes.data, m, ld, d, dtype, 0, k, C.byref(res), None, 0, None)
    assert call(k=0) == _capi.FAD_ERR_INVALID
    assert call(k=17) == _capi.FAD_ERR_INVALID
    assert call(dtype=_capi.FAD_F64) == _capi.FAD_ERR_INVALID
    assert call(dtype=9) == _capi.FAD_ERR_INVALID
    assert call(d=0) == _capi.FAD_ERR_INVALID
    assert call(ld=4) == _capi.FAD_ERR_INVALID
    assert call(n=5) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(m=5) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(n=2, m=16, k=1) != _capi.FAD_ERR_TOO_FEW_ROWS


def test_prdc_python_errors_raise_before_the_library():
    from fadtk_amd import calc_precision_recall_density_coverage as prdc
    from fadtk_amd import hip
    x = np.zeros((8, 4), np.float32)
    for a, b, k in ((x, x, 0), (x, x, 17), (x, x, 8), (x[:5], x, 5), (x, x[:5], 5), (x, x[:, :3], 2), (x[0], x, 2), (x[None], x, 2)):
        with pytest.raises(ValueError):
            prdc(a, b, k=k)
    with pytest.raises(ValueError):
        hip.prdc(x, x, k=0)
    with pytest.raises(ValueError):
        hip.prdc(x, x[:, :3], k=2)
    with pytest.raises(ValueError, match="cast"):
        hip.prdc(x.astype(np.float64), x, k=2)


def test_prdc_refuses_statistics_baseline(tmp_path):
    from fadtk_amd import PrecisionRecall

    class Toy:
        name = "toy"
        sr = 16000
    npz = tmp_path / "base.npz"
    np.savez(npz, **{"toy.mu": np.zeros(4), "toy.cov": np.eye(4)})
    with pytest.raises(ValueError, match="statistics"):
        PrecisionRecall(Toy()).score(npz, tmp_path)


def test_prdc_cli_help_parses():
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.prdc", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    for flag in ("-k", "-w", "baseline", "eval", "csv"):
        assert flag in r.stdout
