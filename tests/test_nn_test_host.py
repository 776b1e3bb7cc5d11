"""Leave-one-out k-NN two-sample test (fad_nn_test), host side (no GPU): the vote rule on a hand-written line, the blobs pair, the
calibration draws and the near-copies pair through the float64 reference of tests/nn_test_reference.py alone, Python's argument errors
before the library is loaded, the command line's refusal of a CSV with another header, the C ABI surface with its argument errors
before any device call, and the bit-sliced votes of csrc/nn_vote.h as a stand-alone program (once more under ASan and UBSan)."""
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


NT = _load("nn_test_reference")
AR = _load("kad_aggregate_reference")
PR = NT.PR


# ------------------------------------------------------------------------------------------------------- the reference alone
@pytest.mark.parametrize("k", [1, 3])
def test_vote_rule_on_a_hand_written_line(k):
    idx, d2 = NT.graph(NT.LINE_X, NT.LINE_Y, k)
    assert idx.tolist() == NT.LINE_GRAPH[k]                                    # exact ties in distance go to the smaller index
    assert d2.tolist() == NT.LINE_DIST2[k]
    u = np.concatenate([PR.observed_labelling(4, 3), NT.LINE_U])
    cx, cy = NT.counts(idx, u)
    assert (int(cx[0]), int(cy[0])) == NT.LINE_COUNTS[k][0]
    assert (int(cx[1]), int(cy[1])) == NT.LINE_COUNTS[k][1]
    res = NT.results(idx, 4, 3, NT.LINE_U)
    c0, c1 = sum(NT.LINE_COUNTS[k][0]), sum(NT.LINE_COUNTS[k][1])
    assert res["accuracy"] == c0 / 7.0 and res["accuracy_x"] == NT.LINE_COUNTS[k][0][0] / 4.0
    assert res["accuracy_y"] == NT.LINE_COUNTS[k][0][1] / 3.0
    assert res["p_value"] == (1.0 + (c1 >= c0)) / 2.0 and res["p_value_low"] == (1.0 + (c1 <= c0)) / 2.0


def test_p_values_count_ties_in_both_tails():
    assert NT.p_values([5, 5, 4, 6, 5]) == (4.0 / 5.0, 4.0 / 5.0)
    assert NT.p_values([9, 1, 2, 3]) == (0.25, 1.0)
    assert NT.p_values([0, 1, 2, 3]) == (1.0, 0.25)


def test_blobs_pair_is_told_apart_with_no_bandwidth():
    """float64 reference alone: the pair on which the median-sigma KAD test is blind (test_kad_aggregate_host.py)."""
    x, y, u = AR.blobs_case()
    idx, _ = NT.graph(x, y, 5)
    for k in (1, 5):
        res = NT.results(idx[:, :k], 400, 400, u)
        print(f"[nn-test] blobs float64 k = {k}: accuracy {res['accuracy']:.4f}, p_value {res['p_value']}")
        assert res["p_value"] <= 0.05 and res["accuracy"] > 0.5


def test_calibration_seeds_hold_in_float64():
    """100 null draws (kad_aggregate_reference.null_draw: rows, then labellings, from default_rng(1000 + s)), k = 1 and k = 5."""
    hits = {1: 0, 5: 0}
    for s in range(100):
        x, y, u = AR.null_draw(s)
        idx, _ = NT.graph(x, y, 5)
        for k in hits:
            hits[k] += NT.results(idx[:, :k], 150, 150, u)["p_value"] <= 0.05
    print(f"[nn-test] calibration float64: {hits[1]} (k = 1) and {hits[5]} (k = 5) of 100 p-values <= 0.05")
    assert hits[1] <= AR.CALIBRATION_CAP and hits[5] <= AR.CALIBRATION_CAP


def test_near_copies_sit_in_the_lower_tail():
    x, y, u = NT.near_copies_case()
    res = NT.reference(x, y, u, 1)
    print(f"[nn-test] near copies float64: accuracy {res['accuracy']:.4f}, eval rows {res['accuracy_y']}, p_value_low {res['p_value_low']}")
    assert res["accuracy_y"] == 0.0 and res["accuracy"] < 0.25 and res["p_value_low"] <= 0.05


# ------------------------------------------------------------------------------------------------------------ Python entries
def test_argument_errors_raise_before_the_library_loads(monkeypatch):
    import fadtk_amd
    from fadtk_amd import _capi, hip, nn_test

    def no_library(*a, **k):
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(_capi, "load_library", no_library)
    calc = fadtk_amd.calc_nearest_neighbour_test
    assert calc is nn_test.calc_nearest_neighbour_test and fadtk_amd.NearestNeighbourTest is nn_test.NearestNeighbourTest
    x = np.zeros((8, 4), np.float32)
    lab = hip.pack_labels(PR.random_labellings(8, 8, 3, np.random.default_rng(0)))
    for a, b in ((x[0], x), (x[:1], x), (x, x[:, :3]), (x, x[:1])):           # shapes, dimensions, fewer than 2 rows
        with pytest.raises(ValueError):
            calc(a, b, labels=lab)
    for k in (0, 2, 4, 16, 17, -1, 1.5, True):
        with pytest.raises(ValueError, match="k"):
            calc(x, x, k=k, labels=lab)
        with pytest.raises(ValueError, match="k"):
            hip.nn_test(x, x, lab, k=k)
    with pytest.raises(ValueError, match="pooled rows"):
        calc(x[:2], x[:2], k=5, labels=lab)                                    # k > n + m - 1
    for p in (0, hip.KAD_MAX_PERMUTATIONS + 1):
        with pytest.raises(ValueError, match="permutations"):
            calc(x, x, permutations=p)
    obj = nn_test.NearestNeighbourTest.__new__(nn_test.NearestNeighbourTest)   # no model, no files: the checks come first
    for kw in ({"k": 2}, {"k": 17}, {"permutations": 0}):
        with pytest.raises(ValueError):
            obj.test("a", "b", **kw)
    assert hip.NN_TEST_MAX_K == 15 and [hip.nn_test_k(k, 16) for k in (1, 3, 15)] == [1, 3, 15]
    import fadtk.nn_test as alias
    assert alias.calc_nearest_neighbour_test is calc and alias.main is nn_test.main


def test_command_line_refuses_a_csv_with_another_header_before_reading_rows(tmp_path, monkeypatch):
    from fadtk_amd import nn_test
    from fadtk_amd.kad import CSV_HEADER as KAD_HEADER
    assert nn_test.CSV_HEADER == ("model,baseline,eval,k,n,m,accuracy,accuracy_baseline,accuracy_eval,p_value,p_value_low,permutations,"
                                  "seed\n")

    def no_rows(self, *a, **k):
        raise AssertionError("rows were asked for")
    monkeypatch.setattr(nn_test.NearestNeighbourTest, "__init__", no_rows)
    model = next(iter(__import__("fadtk_amd.cli", fromlist=["_registry"])._registry()))
    csv = tmp_path / "other.csv"
    csv.write_text(KAD_HEADER + "vggish,a,b,0.1,1.0,1.0,0.0\n")
    before = csv.read_bytes()
    with pytest.raises(ValueError, match="header"):
        nn_test.main([model, str(tmp_path / "none"), str(tmp_path / "none"), str(csv)])
    assert csv.read_bytes() == before
    for bad in (("-k", "2"), ("-k", "17"), ("-p", "0")):                       # refused by the parser, exit status 2
        with pytest.raises(SystemExit) as e:
            nn_test.main([model, "a", "b", str(tmp_path / "new.csv"), *bad])
        assert e.value.code == 2
    own = tmp_path / "own.csv"
    nn_test.append_csv(own, "vggish,a,b,1,2,2,0.5,0.5,0.5,1.0,1.0,1,0")
    nn_test.check_csv(own)
    assert own.read_text().splitlines()[0] + "\n" == nn_test.CSV_HEADER and len(own.read_text().splitlines()) == 2
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.nn_test", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "--permutations" in r.stdout and "--seed" in r.stdout, r.stderr


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def test_header_declares_and_library_exports_fad_nn_test():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_nn_test\s*\(", text) and "fad_nn_test_result_t" in text
    _capi, lib = _lib()
    assert len(_capi.SIGNATURES["fad_nn_test"][1]) == 20 and hasattr(lib, "fad_nn_test")
    assert C.sizeof(_capi.FadNnTestResult) == 5 * 8 + 4 * 8 + 8               # the int k, padded to the struct's alignment
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_capi.LIB_PATH)], capture_output=True, text=True)
    assert nm.returncode == 0 and re.search(r"\bT fad_nn_test$", nm.stdout, flags=re.M)
    assert lib.fad_version() == 2


def _call(lib, _capi, x, y, labels, k=1, dtype=None, d=None, ldx=None, n_perm=None, on_device=0, out=True, nulls=True):
    P = labels.shape[0] if n_perm is None else n_perm
    N = x.shape[0] + y.shape[0]
    res = _capi.FadNnTestResult()
    res.accuracy = -7.0
    nx, ny = np.full(max(P, 1), -7, np.int64), np.full(max(P, 1), -7, np.int64)
    idx, d2 = np.full(N * 16, -7, np.int32), np.full(N * 16, -7.0, np.float32)
    st = lib.fad_nn_test(x.ctypes.data, x.shape[0], ldx or x.shape[1], y.ctypes.data, y.shape[0], y.shape[1],
                         x.shape[1] if d is None else d, _capi.FAD_F16 if dtype is None else dtype, 0, k, labels.ctypes.data, P, on_device,
                         C.byref(res) if out else None, nx.ctypes.data if nulls else None, ny.ctypes.data, idx.ctypes.data, d2.ctypes.data,
                         0, None)
    untouched = res.accuracy == -7.0 and (nx == -7).all() and (ny == -7).all() and (idx == -7).all() and (d2 == -7.0).all()
    assert untouched or st == 0                                                # a refusal writes nothing
    return st


def test_fad_nn_test_argument_errors_come_before_the_device():
    import torch
    from fadtk_amd.hip import pack_labels
    _capi, lib = _lib()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((16, 8)).astype(np.float16)
    y = rng.standard_normal((10, 8)).astype(np.float16)
    lab = pack_labels(PR.random_labellings(16, 10, 5, rng))
    if not torch.cuda.is_available():            # valid arguments reach the device check
        assert _call(lib, _capi, x, y, lab) == _capi.FAD_ERR_NO_DEVICE
        assert _call(lib, _capi, x, y, lab, k=15) == _capi.FAD_ERR_NO_DEVICE
    for k in (0, 2, 16, 17, -1):
        assert _call(lib, _capi, x, y, lab, k=k) == _capi.FAD_ERR_INVALID and b"odd" in lib.fad_last_error()
    small = pack_labels(PR.random_labellings(2, 2, 5, rng))
    assert _call(lib, _capi, x[:2], y[:2], small, k=5) == _capi.FAD_ERR_INVALID and b"pooled rows" in lib.fad_last_error()   # k = N + 1
    assert _call(lib, _capi, x, y, lab, out=False) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x, y, lab, nulls=False) == _capi.FAD_ERR_INVALID
    assert _call(lib, _capi, x[:1], y, pack_labels(PR.random_labellings(1, 10, 5, rng))) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert _call(lib, _capi, x, y[:1], pack_labels(PR.random_labellings(16, 1, 5, rng))) == _capi.FAD_ERR_TOO_FEW_ROWS
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


# ------------------------------------------------------------------------------------------------- the votes of csrc/nn_vote.h
def _run_cpp(tmp_path, name, flags=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-o", str(exe), str(ROOT / "tests" / "native_cpu" / f"{name}.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout


def test_bit_sliced_votes_equal_popcount_majority(tmp_path):
    _run_cpp(tmp_path, "nn_vote_check")


def test_bit_sliced_votes_under_sanitizers(tmp_path):
    """The same program (not loaded into Python) under ASan and UBSan."""
    _run_cpp(tmp_path, "nn_vote_check", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
