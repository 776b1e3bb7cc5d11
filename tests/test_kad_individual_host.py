"""Per-song Kernel Audio Distance (fad_kad_individual), host side (no GPU): the work units of the cross and band passes
(kad_song_tiles.h, checked with g++), the C ABI surface, the errors raised before any device call, and the command line."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def test_kad_song_units_cover_every_pair_once(tmp_path):
    exe = tmp_path / "kad_song_tiles_cover"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "native_cpu" / "kad_song_tiles_cover.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("OK"), r.stdout


def test_header_declares_and_capi_binds_kad_individual():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_kad_individual\s*\(", text)
    _capi, lib = _lib()
    assert "fad_kad_individual" in _capi.SIGNATURES and hasattr(lib, "fad_kad_individual")
    assert len(_capi.SIGNATURES["fad_kad_individual"][1]) == 19
    assert lib.fad_version() == 2


def _call(lib, _capi, x, rows, offsets, dtype=None, d=None, ldx=None, ldy=None, bandwidth=0.0):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    S = max(off.shape[0] - 1, 0)
    outs = [np.zeros(max(S, 1)) for _ in range(3)]
    status = np.zeros(max(S, 1), dtype=np.int32)
    res = _capi.FadKadResult()
    d = x.shape[1] if d is None else d
    return lib.fad_kad_individual(x.ctypes.data, x.shape[0], ldx or x.shape[1], rows.ctypes.data, rows.shape[0], ldy or rows.shape[1],
                                  off.ctypes.data_as(C.POINTER(C.c_int64)), S, d, _capi.FAD_F16 if dtype is None else dtype, 0,
                                  bandwidth, C.byref(res), outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data,
                                  status.ctypes.data, 0, None)


def test_kad_individual_without_gpu_is_no_device_after_argument_errors():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _capi, lib = _lib()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((16, 8)).astype(np.float16)
    y = rng.standard_normal((10, 8)).astype(np.float16)
    assert _call(lib, _capi, x, y, [0, 3, 10]) == _capi.FAD_ERR_NO_DEVICE
    assert _call(lib, _capi, x, y, [0, 0, 1, 10]) == _capi.FAD_ERR_NO_DEVICE          # empty and one-frame songs are not argument errors
    # argument errors come first, device or not
    assert _call(lib, _capi, x, y, [1, 3, 10]) == _capi.FAD_ERR_INVALID                # offsets[0] != 0
    assert _call(lib, _capi, x, y, [0, 5, 3, 10]) == _capi.FAD_ERR_INVALID             # decreasing
    assert _call(lib, _capi, x, y, [0, 3, 9]) == _capi.FAD_ERR_INVALID                 # last offset != n_rows
    assert _call(lib, _capi, x, y, [0, 3, 11]) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x[:1], y, [0, 3, 10]) == _capi.FAD_ERR_TOO_FEW_ROWS       # a baseline of one row
    assert _call(lib, _capi, x, y, [0, 3, 10], dtype=_capi.FAD_F64) == _capi.FAD_ERR_INVALID
    assert b"cast" in lib.fad_last_error()
    assert _call(lib, _capi, x, y, [0, 3, 10], dtype=17) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, [0, 3, 10], d=0) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, [0, 3, 10], d=4096, ldx=4096, ldy=4096) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, [0, 3, 10], ldx=4) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, [0, 3, 10], ldy=4) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, [0, 3, 10], bandwidth=float("inf")) == _capi.FAD_ERR_INVALID
    from fadtk_amd import calc_kernel_audio_distance_individual
    with pytest.raises(_capi.FadHipUnavailable):
        calc_kernel_audio_distance_individual(x, [y[:3], y[3:]])


def test_kad_individual_shape_errors_raise_before_the_library():
    from fadtk_amd import calc_kernel_audio_distance_individual, hip
    x = np.zeros((8, 4), np.float32)
    for a, songs in ((x[0], [x]), (x[:1], [x]), (x, [x[:, :3]]), (x, [x[0]]), (x[None], [x])):
        with pytest.raises(ValueError):
            calc_kernel_audio_distance_individual(a, songs)
    with pytest.raises(ValueError, match="cast"):
        hip.kad_individual(x.astype(np.float64), x, [0, 8])
    with pytest.raises(ValueError):
        hip.kad_individual(x, x, [0, 8], bandwidth=0.0)


def test_kad_individual_refuses_statistics_baseline(tmp_path):
    from fadtk_amd import KernelAudioDistance

    class Toy:
        name = "toy"
        sr = 16000
    npz = tmp_path / "base.npz"
    np.savez(npz, **{"toy.mu": np.zeros(4), "toy.cov": np.eye(4)})
    (tmp_path / "evl").mkdir()
    kad = KernelAudioDistance(Toy())
    with pytest.raises(ValueError, match="statistics"):
        kad.score_individual(npz, tmp_path / "evl", tmp_path / "out.csv")
    existing = tmp_path / "done.csv"
    existing.write_text("a,1\n")
    assert kad.score_individual(npz, tmp_path / "evl", existing) == existing          # an existing CSV is returned untouched
    assert existing.read_text() == "a,1\n"


def test_kad_cli_help_shows_indiv():
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "--indiv" in r.stdout and "kad-individual-results.csv" in r.stdout.replace("-\n", "-").replace("\n", " ").replace(" ", "")
