"""KAD standard errors (fad_kad_uncertainty), host side (no GPU): the work units of the pass (kad_unc_tiles.h, checked with g++), the
C ABI surface, the errors raised before any device call, the float64 reference against kad_reference and against the spread of the
estimate over independent draws, the paired comparison arithmetic and the command line's help."""
import ctypes as C
import importlib.util
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


U = _load("kad_uncertainty_reference")
R = _load("kad_reference")


def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def test_kad_unc_units_cover_every_tile_once(tmp_path):
    exe = tmp_path / "kad_unc_tiles_cover"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "native_cpu" / "kad_unc_tiles_cover.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("OK"), r.stdout


def test_header_declares_and_library_exports_kad_uncertainty():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_kad_uncertainty\s*\(", text)
    _capi, lib = _lib()
    assert "fad_kad_uncertainty" in _capi.SIGNATURES and hasattr(lib, "fad_kad_uncertainty")
    assert len(_capi.SIGNATURES["fad_kad_uncertainty"][1]) == 17
    assert lib.fad_version() == 2
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_capi.LIB_PATH)], capture_output=True, text=True)
    assert nm.returncode == 0 and re.search(r"\bT fad_kad_uncertainty$", nm.stdout, flags=re.M)


def _call(lib, _capi, x, ys, dtype=None, d=None, ldx=None, ldys=None, bandwidth=0.0, n_sets=None):
    S = len(ys)
    ptrs = (C.c_void_p * max(S, 1))(*[y.ctypes.data for y in ys])
    ms = np.array([y.shape[0] for y in ys] or [0], dtype=np.int64)
    lds = np.array(ldys or [y.shape[1] for y in ys] or [0], dtype=np.int64)
    res = (_capi.FadKadResult * max(S, 1))()
    cov = np.zeros(max(S, 1) ** 2)
    d = x.shape[1] if d is None else d
    return lib.fad_kad_uncertainty(x.ctypes.data, x.shape[0], ldx or x.shape[1], ptrs, ms.ctypes.data_as(C.POINTER(C.c_int64)),
                                   lds.ctypes.data_as(C.POINTER(C.c_int64)), S if n_sets is None else n_sets, d,
                                   _capi.FAD_F16 if dtype is None else dtype, 0, bandwidth, res, cov.ctypes.data, None, None, 0, None)


def test_kad_uncertainty_without_gpu_is_no_device_after_argument_errors():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _capi, lib = _lib()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((16, 8)).astype(np.float16)
    y = rng.standard_normal((10, 8)).astype(np.float16)
    assert _call(lib, _capi, x, [y, y[:2]]) == _capi.FAD_ERR_NO_DEVICE
    # argument errors come first, device or not
    assert _call(lib, _capi, x, [y, y[:1]]) == _capi.FAD_ERR_TOO_FEW_ROWS             # a one-row set
    assert _call(lib, _capi, x[:1], [y]) == _capi.FAD_ERR_TOO_FEW_ROWS                # a one-row baseline
    assert _call(lib, _capi, x, []) == _capi.FAD_ERR_INVALID                          # S = 0
    assert _call(lib, _capi, x, [y] * 65) == _capi.FAD_ERR_INVALID                    # S = 65
    assert _call(lib, _capi, x, [y], dtype=_capi.FAD_F64) == _capi.FAD_ERR_INVALID
    assert b"cast" in lib.fad_last_error()
    assert _call(lib, _capi, x, [y], dtype=17) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, [y], d=0) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, [y], d=4096, ldx=4096, ldys=[4096]) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, [y], ldx=4) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, [y], ldys=[4]) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, [y], bandwidth=float("inf")) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, [y], bandwidth=float("nan")) == _capi.FAD_ERR_INVALID
    from fadtk_amd import calc_kernel_audio_distance_uncertainty
    with pytest.raises(_capi.FadHipUnavailable):
        calc_kernel_audio_distance_uncertainty(x, [y])


def test_kad_uncertainty_shape_errors_raise_before_the_library():
    from fadtk_amd import calc_kernel_audio_distance_uncertainty, hip
    x = np.zeros((8, 4), np.float32)
    for a, ys in ((x[0], [x]), (x[:1], [x]), (x, [x[:, :3]]), (x, [x[0]]), (x, [x[:1]]), (x[None], [x])):
        with pytest.raises(ValueError):
            calc_kernel_audio_distance_uncertainty(a, ys)
    with pytest.raises(ValueError, match="cast"):
        hip.kad_uncertainty(x.astype(np.float64), [x])
    with pytest.raises(ValueError):
        hip.kad_uncertainty(x, [])
    with pytest.raises(ValueError):
        hip.kad_uncertainty(x, [x] * 65)
    with pytest.raises(ValueError):
        hip.kad_uncertainty(x, [x], bandwidth=0.0)


def test_reference_mmd2_matches_kad_reference():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((60, 5))
    ys = [rng.standard_normal((40, 5)) * 1.2 + 0.3, rng.standard_normal((2, 5)), rng.standard_normal((75, 5)) + 0.1]
    u = U.uncertainty(x, ys)
    for y, got in zip(ys, u["sets"]):
        want = R.kad(x, y)
        for k in ("mmd2", "kxx_mean", "kyy_mean", "kxy_mean"):
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
    assert u["cov"] == pytest.approx(u["cov"].T, rel=1e-12)
    assert np.all(np.linalg.eigvalsh(u["cov"]) > -1e-15)


def test_reference_variance_matches_spread_over_draws():
    """The first-order variance against the empirical variance of MMD^2_U over independent draws (sets that differ from X)."""
    rng = np.random.default_rng(1)
    sigma, n, d, draws = 4.0, 200, 8, 300
    est, pred = [], []
    for _ in range(draws):
        x = rng.standard_normal((n, d))
        y = rng.standard_normal((n, d)) + 0.5
        u = U.uncertainty(x, [y], sigma=sigma)
        est.append(u["sets"][0]["mmd2"])
        pred.append(u["cov"][0, 0])
    ratio = np.var(est, ddof=1) / np.mean(pred)
    print(f"[kad-unc] empirical / predicted variance over {draws} draws: {ratio:.3f}")
    assert 0.8 <= ratio <= 1.25, ratio


def test_compare_z_and_p():
    from fadtk_amd.kad import KadUncertainty
    cov = np.array([[4.0, 1.0, 0.0], [1.0, 9.0, 0.0], [0.0, 0.0, 0.0]])
    r = KadUncertainty(values=np.array([1.0, 4.0, 1.0]), stderr=np.sqrt(np.diag(cov)), cov=cov, bandwidth=1.0, scale=1.0)
    z, p = r.compare()
    assert z[0, 1] == pytest.approx(-3.0 / math.sqrt(4 + 9 - 2)) and z[1, 0] == pytest.approx(-z[0, 1])
    assert p[0, 1] == pytest.approx(math.erfc(abs(z[0, 1]) / math.sqrt(2)))
    assert np.all(np.diag(z) == 0) and np.all(np.diag(p) == 1)
    assert z[0, 2] == pytest.approx(0.0) and p[0, 2] == pytest.approx(1.0)
    assert p[0, 1] == pytest.approx(0.36571, abs=1e-4)


def test_kad_compare_cli_help():
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad_compare", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.replace("\n", " ")
    assert "--csv" in out and "--bandwidth" in out and "--scale" in out
