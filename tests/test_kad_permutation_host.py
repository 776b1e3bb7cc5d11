"""KAD permutation test (fad_kad_permutation_test), host side (no GPU): the launches of the pass (kad_perm_tiles.h, checked with g++),
the C ABI surface, the errors raised before any device call, the q / R / T algebra of the float64 reference against kad_reference on
explicitly relabelled sets, the p-value with ties, label packing and the command line's help."""
import ctypes as C
import importlib.util
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


PR = _load("kad_permutation_reference")
R = _load("kad_reference")


def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def test_kad_perm_launches_cover_every_tile_once_per_group(tmp_path):
    exe = tmp_path / "kad_perm_tiles_cover"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "native_cpu" / "kad_perm_tiles_cover.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("OK"), r.stdout


def test_header_declares_and_library_exports_kad_permutation_test():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_kad_permutation_test\s*\(", text)
    _capi, lib = _lib()
    assert "fad_kad_permutation_test" in _capi.SIGNATURES and hasattr(lib, "fad_kad_permutation_test")
    assert len(_capi.SIGNATURES["fad_kad_permutation_test"][1]) == 18
    assert lib.fad_version() == 2
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_capi.LIB_PATH)], capture_output=True, text=True)
    assert nm.returncode == 0 and re.search(r"\bT fad_kad_permutation_test$", nm.stdout, flags=re.M)


def _labels(n, m, P, seed=0):
    from fadtk_amd.hip import pack_labels
    return pack_labels(PR.random_labellings(n, m, P, np.random.default_rng(seed)))


def _call(lib, _capi, x, y, labels, dtype=None, d=None, ldx=None, ldy=None, bandwidth=0.0, n_perm=None, on_device=0):
    res = _capi.FadKadResult()
    P = labels.shape[0] if n_perm is None else n_perm
    null = np.zeros(max(P, 1))
    pv = C.c_double()
    d = x.shape[1] if d is None else d
    return lib.fad_kad_permutation_test(x.ctypes.data, x.shape[0], ldx or x.shape[1], y.ctypes.data, y.shape[0], ldy or y.shape[1], d,
                                        _capi.FAD_F16 if dtype is None else dtype, 0, bandwidth, labels.ctypes.data, P, on_device,
                                        C.byref(res), null.ctypes.data, C.byref(pv), 0, None)


def test_kad_permutation_without_gpu_is_no_device_after_argument_errors():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _capi, lib = _lib()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((16, 8)).astype(np.float16)
    y = rng.standard_normal((10, 8)).astype(np.float16)
    lab = _labels(16, 10, 5)
    assert _call(lib, _capi, x, y, lab) == _capi.FAD_ERR_NO_DEVICE
    assert _call(lib, _capi, x, y, lab, on_device=1) == _capi.FAD_ERR_NO_DEVICE          # device labels: counted on the device
    # argument errors come first, device or not
    assert _call(lib, _capi, x[:1], y, _labels(1, 10, 5)) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert _call(lib, _capi, x, y[:1], _labels(16, 1, 5)) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert _call(lib, _capi, x, y, lab, dtype=_capi.FAD_F64) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, dtype=17) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, d=0) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, d=4096, ldx=4096, ldy=4096) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, ldx=4) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, ldy=4) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, n_perm=0) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, n_perm=65537) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, bandwidth=float("nan")) == _capi.FAD_ERR_INVALID
    # host labels with a wrong count, or a bit past N, are caught before the device
    bad = lab.copy()
    bad[2, 0] ^= 1
    assert _call(lib, _capi, x, y, bad) == _capi.FAD_ERR_INVALID
    assert b"labelling 2" in lib.fad_last_error()
    hi = lab.copy()
    ones = PR.unpack(hi, 26)[3]
    hi[3] = 0
    hi[3, 0] = np.uint32((1 << 15) - 1)          # 15 ones below N ...
    hi[3, 0] |= np.uint32(1 << 30)               # ... and one at row 30 >= N = 26
    assert ones.sum() == 16
    assert _call(lib, _capi, x, y, hi) == _capi.FAD_ERR_INVALID
    assert b"past N" in lib.fad_last_error()
    from fadtk_amd import calc_kernel_audio_distance_permutation_test
    with pytest.raises(_capi.FadHipUnavailable):
        calc_kernel_audio_distance_permutation_test(x, y, labels=lab)


def test_kad_permutation_shape_errors_raise_before_the_library():
    from fadtk_amd import calc_kernel_audio_distance_permutation_test, hip
    x = np.zeros((8, 4), np.float32)
    lab = _labels(8, 8, 3)
    for a, b in ((x[0], x), (x[:1], x), (x, x[:, :3]), (x, x[:1])):
        with pytest.raises(ValueError):
            calc_kernel_audio_distance_permutation_test(a, b, labels=lab)
    with pytest.raises(ValueError):
        calc_kernel_audio_distance_permutation_test(x, x, permutations=0)
    with pytest.raises(ValueError):
        calc_kernel_audio_distance_permutation_test(x, x, permutations=65537)
    with pytest.raises(ValueError, match="cast"):
        hip.kad_permutation_test(x.astype(np.float64), x, lab)
    with pytest.raises(ValueError):
        hip.kad_permutation_test(x, x, lab[:, :0])                         # no words
    with pytest.raises(ValueError):
        hip.kad_permutation_test(x, x, np.zeros((3, 15), bool))            # 0/1 labels of the wrong width
    with pytest.raises(ValueError):
        hip.kad_permutation_test(x, x, lab.astype(np.int64))
    with pytest.raises(ValueError):
        hip.kad_permutation_test(x, x, lab, bandwidth=0.0)


@pytest.mark.parametrize("n,m,d", [(2, 2, 3), (7, 19, 5), (40, 25, 1), (33, 64, 8)])
def test_reference_algebra_matches_kad_reference_on_relabelled_sets(n, m, d):
    """t(u) from q, R and T on the pooled kernel is fad_kad's MMD^2 of the relabelled sets, for the observed and random labellings."""
    rng = np.random.default_rng(n * 100 + m)
    x = rng.standard_normal((n, d))
    y = rng.standard_normal((m, d)) * 1.3 + 0.4
    sigma = PR.median_distance_pooled(x, y)
    z = PR.pooled(x, y)
    u = np.concatenate([PR.observed_labelling(n, m), PR.random_labellings(n, m, 6, rng)])
    t = PR.statistics(x, y, u, sigma)
    for ul, tl in zip(u, t):
        want = R.kad(z[ul], z[~ul], sigma=sigma)["mmd2"]
        assert tl == pytest.approx(want, rel=1e-10, abs=1e-13)
    assert t[0] == pytest.approx(R.kad(x, y, sigma=sigma)["mmd2"], rel=1e-10, abs=1e-13)


def test_reference_bandwidth_is_the_pooled_median():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((30, 4)), rng.standard_normal((21, 4)) + 1.0
    assert PR.median_distance_pooled(x, y) == R.median_distance(np.concatenate([x, y]))
    t_default = PR.statistics(x, y, PR.observed_labelling(30, 21))
    t_given = PR.statistics(x, y, PR.observed_labelling(30, 21), PR.median_distance_pooled(x, y))
    assert t_default[0] == t_given[0]


def test_p_value_formula_with_ties():
    assert PR.p_value(0.5, [0.1, 0.2, 0.3]) == 0.25
    assert PR.p_value(0.2, [0.1, 0.2, 0.3]) == 0.75                    # a tie counts as at least as extreme
    assert PR.p_value(0.0, [0.0] * 9) == 1.0
    assert PR.p_value(1.0, [0.0] * 199) == 1.0 / 200
    assert PR.p_value(-1.0, [-2.0, -1.0, -1.0, 0.0]) == 4.0 / 5


def test_label_packing_round_trip():
    from fadtk_amd.hip import kad_label_words, pack_labels
    rng = np.random.default_rng(2)
    for N in (4, 31, 32, 33, 64, 65, 1000):
        u = rng.random((5, N)) < 0.5
        w = pack_labels(u)
        assert w.dtype == np.uint32 and w.shape == (5, kad_label_words(N))
        assert np.array_equal(PR.unpack(w, N), u)
        for i in (0, N - 1, N // 2):                                        # bit i & 31 of word i >> 5 is row i
            assert bool((w[0, i >> 5] >> np.uint32(i & 31)) & 1) == u[0, i]


def test_kad_permutation_cli_help():
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad_permutation", "--help"], capture_output=True, text=True, cwd=ROOT,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.replace("\n", " ")
    for flag in ("--permutations", "--seed", "--bandwidth", "--scale", "--workers", "csv"):
        assert flag in out, flag
    from fadtk_amd import kad_permutation
    assert kad_permutation.CSV_HEADER == "model,baseline,eval,kad,p_value,permutations,seed,bandwidth,scale,time\n"
