"""Kernel Audio Distance, host side (no GPU): the tile map of the kernels (kad_tiles.h, checked with g++), the C ABI surface, the
errors raised before any library call, the command line, and the float64 reference the GPU tests compare against."""
import ctypes as C
import importlib.util
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("kad_reference", Path(__file__).resolve().parent / "kad_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def test_kad_tile_map_covers_every_pair_once(tmp_path):
    exe = tmp_path / "kad_tiles_cover"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "native_cpu" / "kad_tiles_cover.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("OK"), r.stdout


def test_header_declares_and_capi_binds_kad():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_kad\s*\(", text) and re.search(r"\bint\s+fad_kad_median_distance\s*\(", text)
    assert "fad_kad_result_t" in text
    _capi, lib = _lib()
    for name in ("fad_kad", "fad_kad_median_distance"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert [f for f, _ in _capi.FadKadResult._fields_] == ["mmd2", "kxx_mean", "kyy_mean", "kxy_mean", "bandwidth", "n", "m"]
    assert C.sizeof(_capi.FadKadResult) == 5 * 8 + 2 * 8
    assert lib.fad_version() == 2


def test_kad_without_gpu_is_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _capi, lib = _lib()
    x = np.random.default_rng(0).standard_normal((16, 8)).astype(np.float16)
    res = _capi.FadKadResult()
    sig = C.c_double()
    assert lib.fad_kad(x.ctypes.data, 16, 8, x.ctypes.data, 16, 8, 8, _capi.FAD_F16, 0, 0.0, C.byref(res), 0, None) == _capi.FAD_ERR_NO_DEVICE
    assert lib.fad_kad_median_distance(x.ctypes.data, 16, 8, 8, _capi.FAD_F16, 0, C.byref(sig), 0, None) == _capi.FAD_ERR_NO_DEVICE
    # argument errors come first, device or not
    assert lib.fad_kad(x.ctypes.data, 1, 8, x.ctypes.data, 16, 8, 8, _capi.FAD_F16, 0, 0.0, C.byref(res), 0, None) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert lib.fad_kad(x.ctypes.data, 16, 8, x.ctypes.data, 16, 8, 8, _capi.FAD_F64, 0, 0.0, C.byref(res), 0, None) == _capi.FAD_ERR_INVALID
    assert b"cast" in lib.fad_last_error()
    assert lib.fad_kad(x.ctypes.data, 16, 8, x.ctypes.data, 16, 8, 8, _capi.FAD_F16, 0, float("nan"), C.byref(res), 0, None) == _capi.FAD_ERR_INVALID
    from fadtk_amd import calc_kernel_audio_distance
    with pytest.raises(_capi.FadHipUnavailable):
        calc_kernel_audio_distance(x, x)


def test_kad_shape_errors_raise_before_the_library():
    from fadtk_amd import calc_kernel_audio_distance, hip
    x = np.zeros((8, 4), np.float32)
    for a, b in ((x[0], x), (x, x[:, :3]), (x[:1], x), (x, x[:1]), (x[None], x)):
        with pytest.raises(ValueError):
            calc_kernel_audio_distance(a, b)
    with pytest.raises(ValueError, match="cast"):
        hip.kad(x.astype(np.float64), x)
    with pytest.raises(ValueError, match="cast"):
        hip.kad_median_distance(x.astype(np.float64))


def test_kad_refuses_statistics_baseline(tmp_path):
    from fadtk_amd import KernelAudioDistance

    class Toy:
        name = "toy"
        sr = 16000
    npz = tmp_path / "base.npz"
    np.savez(npz, **{"toy.mu": np.zeros(4), "toy.cov": np.eye(4)})
    kad = KernelAudioDistance(Toy())
    with pytest.raises(ValueError, match="statistics"):
        kad.score(npz, tmp_path)
    with pytest.raises(ValueError, match="statistics"):
        kad.load_rows(npz)


def test_kad_cli_help_parses():
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    for flag in ("--bandwidth", "--scale", "-w", "baseline", "eval", "csv"):
        assert flag in r.stdout


def test_reference_matches_brute_force_loops():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((7, 3))
    y = rng.standard_normal((5, 3)) + 0.5
    dists = [np.sqrt(((x[i] - x[j]) ** 2).sum()) for i in range(7) for j in range(i + 1, 7)]     # 21 pairs: odd count
    s = sorted(dists)[10]
    assert R.median_distance(x) == pytest.approx(s, rel=1e-15)
    even = sorted(np.sqrt(((x[i] - x[j]) ** 2).sum()) for i in range(5) for j in range(i + 1, 5))  # 10 pairs: mean of two
    assert R.median_distance(x[:5]) == pytest.approx((even[4] + even[5]) / 2, rel=1e-15)

    def k(a, b):
        return np.exp(-((a - b) ** 2).sum() / (2 * s * s))
    kxx = sum(k(x[i], x[j]) for i in range(7) for j in range(7) if i != j) / (7 * 6)
    kyy = sum(k(y[i], y[j]) for i in range(5) for j in range(5) if i != j) / (5 * 4)
    kxy = sum(k(x[i], y[j]) for i in range(7) for j in range(5)) / (7 * 5)
    ref = R.kad(x, y)
    assert ref["bandwidth"] == pytest.approx(s, rel=1e-15)
    for key, want in (("kxx_mean", kxx), ("kyy_mean", kyy), ("kxy_mean", kxy), ("mmd2", kxx + kyy - 2 * kxy)):
        assert ref[key] == pytest.approx(want, rel=1e-12, abs=1e-15), key
