"""KAD permutation test over several bandwidths, aggregated (fad_kad_permutation_sweep, fad_kad_aggregate), host side (no GPU): the C
ABI surface, fad_kad_aggregate against the float64 reference of tests/kad_aggregate_reference.py (ties, one bandwidth, a duplicated
bandwidth, P = 1), the counting itself as a stand-alone program under AddressSanitizer and UBSan, the sweep's argument errors before any
device call, Python's shape errors before the library, the plan of the walks (kad_perm_sweep_tiles.h, checked with g++), the command
line, and the blobs pair and the calibration draws through the float64 reference alone."""
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


AR = _load("kad_aggregate_reference")
PR = AR.PR


def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def _run_cpp(tmp_path, name, flags=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-o", str(exe), str(ROOT / "tests" / "native_cpu" / f"{name}.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout


def test_header_declares_and_library_exports_sweep_and_aggregate():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_kad_permutation_sweep\s*\(", text) and re.search(r"\bint\s+fad_kad_aggregate\s*\(", text)
    assert re.search(r"#define\s+FAD_KAD_PERM_MAX_BANDWIDTHS\s+16\b", text)
    _capi, lib = _lib()
    assert len(_capi.SIGNATURES["fad_kad_permutation_sweep"][1]) == 22 and len(_capi.SIGNATURES["fad_kad_aggregate"][1]) == 5
    assert hasattr(lib, "fad_kad_permutation_sweep") and hasattr(lib, "fad_kad_aggregate")
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_capi.LIB_PATH)], capture_output=True, text=True)
    assert nm.returncode == 0
    for sym in ("fad_kad_permutation_sweep", "fad_kad_aggregate"):
        assert re.search(rf"\bT {sym}$", nm.stdout, flags=re.M), sym
    from fadtk_amd import hip
    assert hip.KAD_PERM_MAX_BANDWIDTHS == 16


def _agree(t):
    from fadtk_amd import hip
    got = hip.kad_aggregate(t)
    pv, pa = AR.aggregate(t)
    assert got["p_values"].tolist() == pv.tolist(), (got["p_values"], pv)
    assert got["p_aggregated"] == pa, (got["p_aggregated"], pa)
    return got


@pytest.mark.parametrize("B,L", [(1, 2), (1, 200), (2, 2), (3, 33), (5, 200), (7, 1000), (16, 300), (40, 64)])
def test_kad_aggregate_equals_reference_on_random_matrices(B, L):
    rng = np.random.default_rng(B * 1000 + L)
    got = _agree(rng.standard_normal((B, L)))
    if B == 1:
        assert got["p_aggregated"] == got["p_values"][0]
    ties = _agree(rng.integers(0, 3, size=(B, L)).astype(np.float64))          # exact ties: >= counts them
    assert np.all(ties["p_values"] >= 1.0 / L)
    _agree(np.zeros((B, L)))                                                    # all tied: every p is 1
    assert _agree(np.zeros((B, L)))["p_aggregated"] == 1.0


def test_kad_aggregate_one_bandwidth_is_the_single_p_value_and_a_copied_row_changes_nothing():
    rng = np.random.default_rng(7)
    t = rng.standard_normal((4, 200))
    t[:, 0] += 1.5
    for b in range(4):
        one = _agree(t[b:b + 1])
        assert one["p_aggregated"] == one["p_values"][0] == PR.p_value(t[b, 0], t[b, 1:])
    base = _agree(t)
    twice = _agree(np.concatenate([t, t[1:2], t[1:2]]))
    assert twice["p_aggregated"] == base["p_aggregated"] and twice["p_values"][:4].tolist() == base["p_values"].tolist()
    assert twice["p_values"][4] == twice["p_values"][5] == base["p_values"][1]
    # P = 1: the aggregate is 1/2 only where the observed labelling is strictly the extreme one at its best bandwidth
    assert _agree(np.array([[1.0, 0.0], [3.0, 2.0]]))["p_aggregated"] == 0.5
    assert _agree(np.array([[1.0, 0.0], [0.5, 2.0]]))["p_aggregated"] == 1.0
    assert _agree(np.array([[0.0, 0.0]]))["p_aggregated"] == 1.0


def test_kad_aggregate_argument_errors():
    from fadtk_amd import hip
    _capi, lib = _lib()
    t = np.zeros((2, 5))
    pv = np.zeros(2)
    pa = C.c_double()
    assert lib.fad_kad_aggregate(None, 2, 5, pv.ctypes.data, C.byref(pa)) == _capi.FAD_ERR_INVALID
    assert lib.fad_kad_aggregate(t.ctypes.data, 0, 5, pv.ctypes.data, C.byref(pa)) == _capi.FAD_ERR_INVALID
    assert lib.fad_kad_aggregate(t.ctypes.data, 2, 1, pv.ctypes.data, C.byref(pa)) == _capi.FAD_ERR_INVALID
    assert lib.fad_kad_aggregate(t.ctypes.data, 2, 5, None, C.byref(pa)) == _capi.FAD_ERR_INVALID
    for bad in (np.zeros(5), np.zeros((2, 1)), np.zeros((0, 5)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError):
            hip.kad_aggregate(bad)


def test_kad_aggregate_counting_under_sanitizers(tmp_path):
    """The counting of fad_kad_aggregate as a program of its own (not loaded into Python), under ASan and UBSan, against brute force."""
    _run_cpp(tmp_path, "kad_aggregate_check", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def test_kad_perm_sweep_plan_covers_every_bandwidth_word_and_tile_once(tmp_path):
    _run_cpp(tmp_path, "kad_perm_sweep_cover", ("-O2",))


def _labels(n, m, P, seed=0):
    from fadtk_amd.hip import pack_labels
    return pack_labels(PR.random_labellings(n, m, P, np.random.default_rng(seed)))


def _call(lib, _capi, x, y, labels, bw=(1.0, 2.0), n_bw=None, relative=0, kernel=0, dtype=None, d=None, ldx=None, n_perm=None,
          on_device=0):
    bw = np.asarray(bw, dtype=np.float64)
    B = len(bw) if n_bw is None else n_bw
    res = (_capi.FadKadResult * max(B, 1))()
    P = labels.shape[0] if n_perm is None else n_perm
    null = np.full((max(B, 1), max(P, 1)), -7.0)
    pv = np.full(max(B, 1), -7.0)
    pa = C.c_double(-7.0)
    st = lib.fad_kad_permutation_sweep(x.ctypes.data, x.shape[0], ldx or x.shape[1], y.ctypes.data, y.shape[0], y.shape[1],
                                       x.shape[1] if d is None else d, _capi.FAD_F16 if dtype is None else dtype, 0,
                                       bw.ctypes.data_as(C.POINTER(C.c_double)), B, relative, kernel, labels.ctypes.data, P, on_device, res,
                                       null.ctypes.data, pv.ctypes.data, C.byref(pa), 0, None)
    assert np.all(null == -7.0) and np.all(pv == -7.0) and pa.value == -7.0 or st == 0           # a refusal writes nothing
    return st


def test_kad_permutation_sweep_argument_errors_come_before_the_device():
    import torch
    _capi, lib = _lib()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((16, 8)).astype(np.float16)
    y = rng.standard_normal((10, 8)).astype(np.float16)
    lab = _labels(16, 10, 5)
    if not torch.cuda.is_available():            # valid arguments reach the device check
        assert _call(lib, _capi, x, y, lab) == _capi.FAD_ERR_NO_DEVICE
        assert _call(lib, _capi, x, y, lab, relative=1, on_device=1) == _capi.FAD_ERR_NO_DEVICE
    wide = np.ones(17)
    assert _call(lib, _capi, x, y, lab, bw=wide, n_bw=0) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, bw=wide) == _capi.FAD_ERR_INVALID and b"1 .. 16" in lib.fad_last_error()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        for relative in (0, 1):
            assert _call(lib, _capi, x, y, lab, bw=(1.0, v, 2.0), relative=relative) == _capi.FAD_ERR_INVALID
            assert (b"factor 1 is" if relative else b"bandwidth 1 is") in lib.fad_last_error()
    assert _call(lib, _capi, x, y, lab, kernel=3) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x[:1], y, _labels(1, 10, 5)) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert _call(lib, _capi, x, y, lab, dtype=_capi.FAD_F64) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, d=0) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, ldx=4) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, n_perm=0) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, n_perm=65537) == _capi.FAD_ERR_INVALID
    bad = lab.copy()
    bad[2, 0] ^= 1                               # a labelling with n + 1 or n - 1 ones
    assert _call(lib, _capi, x, y, bad) == _capi.FAD_ERR_INVALID and b"labelling 2" in lib.fad_last_error()
    hi = lab.copy()
    hi[3] = 0
    hi[3, 0] = np.uint32((1 << 15) - 1) | np.uint32(1 << 30)          # 15 ones below N = 26 and one at row 30
    assert _call(lib, _capi, x, y, hi) == _capi.FAD_ERR_INVALID and b"past N" in lib.fad_last_error()


def test_kad_permutation_sweep_shape_errors_raise_before_the_library():
    from fadtk_amd import calc_kernel_audio_distance_aggregated_test as agg, hip
    x = np.zeros((8, 4), np.float32)
    lab = _labels(8, 8, 3)
    for a, b in ((x[0], x), (x[:1], x), (x, x[:, :3]), (x, x[:1])):
        with pytest.raises(ValueError):
            agg(a, b, labels=lab)
    for kw in ({"permutations": 0}, {"permutations": 65537}, {"factors": ()}, {"factors": [1.0] * 17}, {"factors": (1.0, 0.0)},
               {"factors": (1.0, float("nan"))}, {"bandwidths": (1.0, -2.0)}, {"bandwidths": [1.0], "factors": [1.0]}, {"kernel": "rbf"},
               {"bandwidths": "wide"}):
        with pytest.raises(ValueError):
            agg(x, x, **kw)
    with pytest.raises(ValueError):
        hip.kad_permutation_sweep(x, x, lab)                                 # neither bandwidths nor factors
    with pytest.raises(ValueError):
        hip.kad_permutation_sweep(x, x, lab, bandwidths=[1.0], factors=[1.0])
    with pytest.raises(ValueError, match="1 .. 16"):
        hip.kad_permutation_sweep(x, x, lab, bandwidths=[1.0] * 17)
    with pytest.raises(ValueError, match="cast"):
        hip.kad_permutation_sweep(x.astype(np.float64), x, lab, factors=[1.0])
    with pytest.raises(ValueError):
        hip.kad_permutation_sweep(x, x, np.zeros((3, 15), bool), factors=[1.0])
    with pytest.raises(ValueError):
        hip.kad_permutation_sweep(x, x, lab.astype(np.int64), factors=[1.0])
    import fadtk_amd
    assert fadtk_amd.calc_kernel_audio_distance_aggregated_test is agg
    assert hasattr(fadtk_amd.KernelAudioDistance, "aggregated_test")


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "fadtk_amd.kad_permutation", *args], capture_output=True, text=True, cwd=ROOT, timeout=300)


def test_kad_permutation_cli_flags_of_the_aggregated_test(tmp_path):
    r = _cli("--help")
    assert r.returncode == 0, r.stderr
    out = r.stdout.replace("\n", " ")
    for flag in ("--bandwidth-factors", "--bandwidths", "--bandwidth", "p_aggregated"):
        assert flag in out, flag
    from fadtk_amd import kad_permutation as KP
    assert KP.AGG_CSV_HEADER == "model,baseline,eval,kad,p_value,permutations,seed,bandwidth,scale,time,p_aggregated\n"
    assert KP.CSV_HEADER == "model,baseline,eval,kad,p_value,permutations,seed,bandwidth,scale,time\n"
    model = next(iter(__import__("fadtk_amd.cli", fromlist=["_registry"])._registry()))
    for pair in (("--bandwidth", "1.0", "--bandwidths", "1,2"), ("--bandwidth", "1.0", "--bandwidth-factors", "1,2"),
                 ("--bandwidths", "1,2", "--bandwidth-factors", "1,2")):
        r = _cli(model, "a", "b", *pair)
        assert r.returncode == 2 and "not allowed with" in r.stderr, r.stderr
    for bad in (("--bandwidth-factors", "1,0"), ("--bandwidths", ",".join(["1"] * 17)), ("--bandwidth-factors", "1,x")):
        r = _cli(model, "a", "b", *bad)
        assert r.returncode == 2, r.stderr
    # a CSV of the other form is refused, in both directions and in both kernel forms
    single, agg = tmp_path / "single.csv", tmp_path / "agg.csv"
    single.write_text(KP.CSV_HEADER)
    agg.write_text(KP.AGG_CSV_HEADER.rstrip("\n") + ",kernel\n")
    with pytest.raises(ValueError):
        KP.check_csv_form(single, KP.AGG_CSV_HEADER, "gaussian")
    with pytest.raises(ValueError):
        KP.check_csv_form(agg, KP.CSV_HEADER, "iq")
    with pytest.raises(ValueError):
        KP.check_csv_form(agg, KP.AGG_CSV_HEADER, "gaussian")              # the kernel column, as check_csv refuses it today
    KP.check_csv_form(single, KP.CSV_HEADER, "gaussian")
    KP.check_csv_form(agg, KP.AGG_CSV_HEADER, "imq")
    KP.check_csv_form(tmp_path / "new.csv", KP.AGG_CSV_HEADER, "gaussian")


def test_blobs_pair_median_sigma_is_blind_and_the_aggregate_is_not():
    """float64 reference alone: 3 x 3 unit Gaussians at spacing 10 against the same grid with within-blob correlation 0.8,
    n = m = 400, P = 199, the ladder 2^-5 .. 2 of the pooled median."""
    x, y, u = AR.blobs_case()
    x, y = x.astype(np.float64), y.astype(np.float64)
    med = PR.median_distance_pooled(x, y)
    t = AR.statistics(x, y, AR.with_observed(400, 400, u), [f * med for f in AR.BLOBS_LADDER])
    pv, pa = AR.aggregate(t)
    print(f"[kad-agg] blobs float64: p_values = {np.round(pv, 3).tolist()}, p_aggregated = {pa}")
    assert pv[AR.BLOBS_LADDER.index(1.0)] > 0.2
    assert pa <= 0.05
    assert pv[AR.BLOBS_LADDER.index(1.0)] == PR.p_value(t[5, 0], t[5, 1:])


def test_calibration_seeds_hold_in_float64():
    """The 100 null draws of the GPU calibration check, through the float64 reference alone: the cap holds for the seeds themselves."""
    hits = 0
    for s in range(100):
        x, y, u = AR.null_draw(s)
        x, y = x.astype(np.float64), y.astype(np.float64)
        med = PR.median_distance_pooled(x, y)
        _, pa = AR.aggregate(AR.statistics(x, y, AR.with_observed(150, 150, u), [f * med for f in AR.CALIBRATION_FACTORS]))
        hits += pa <= 0.05
    print(f"[kad-agg] calibration float64: {hits} of 100 aggregates <= 0.05")
    assert hits <= AR.CALIBRATION_CAP
