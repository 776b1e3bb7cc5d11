"""Kernel-by-kernel checks of the nine-launch Frechet chain (fadtk_amd/csrc/ns_fast.h) against host float64 arithmetic: a
gfx950 executable built from tests/native/nsfast_check.hip by `python -m fadtk_amd.build` (see the header of that file for
what is compared).  The chain as a whole is checked against the oracle in test_gpu_parity.py.

tests/native/gemm_check.hip does the same one level down: every instantiation of the float64 and float32 MFMA GEMM kernels
(fadtk_amd/csrc/gemm_f64.hip, gemm_f32.hip) element by element against long double host products, at bounds derived from the
precision of the formats (the header of that file).

tests/native/nsbig_check.hip checks the BATCHED forms of the chain (fadtk_amd/csrc/ns_fast_big.h: nsf_big<SP_FIRST | SP_T | SP_U> on
both tile widths, nsf_i8_big<I8_A | I8_G | I8_G with R planes>) one launch at a time: every problem of a batch has operands, header
scales and step scales of its own, a shared baseline and pairs, skipped, refused and declined problems, guards between all fields, and
batch sizes that exercise every remainder class of the cut over the XCDs -- at the tolerances nsfast_check has for the same arithmetic.
Its res128 section runs nsf_res128<false> and <true> (ns_fast_res.h, D = 128) on batches of 1, 5 and 64 problems, plain and with scaled
steps, and holds the trace estimate of <true>'s record against the tiled route of ns_fast.h and a host float64 correction.

tests/native/nsf64_check.hip checks the all-float64 iteration that every route ends on (fadtk_amd/csrc/frechet_f64.hip, ns_check.h)
below the public entry: ns_tilestats + ns_prepare (statistics, scale rule, the state they arm, the low-precision switch), the mu[k]
schedule of the scaled steps, ns_first, ns_check_block on a table of synthetic residual / trace sequences with the expected state after
every check written out, and run_ns whole on problems this module writes to a file from tests/frechet_f64_reference.py (inputs, the
emulation's stop code and count, the eigenvalue value and its bound).  tests/test_gpu_frechet_f64.py has the public entries."""
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EXE = Path(__file__).resolve().parent / "native" / "nsfast_check"


@pytest.mark.parametrize("dims", [["512"], ["256", "768"], ["1024", "384"]])
def test_ns_fast_kernels_against_host_arithmetic(dims):
    if not EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(EXE), *dims], capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout


GEMM_EXE = EXE.with_name("gemm_check")


@pytest.mark.parametrize("section", ["f64", "f64big", "stats", "f32"])
def test_gemm_kernels_element_by_element(section):
    if not GEMM_EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(GEMM_EXE), section], capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout


BIG_EXE = EXE.with_name("nsbig_check")
BIG_SHAPES = [["256:1", "256:7", "256:8", "256:9", "256:20"], ["384:3", "384:9"], ["768:3", "768:9"], ["512:3", "1024:3"]]


@pytest.mark.parametrize("shapes", BIG_SHAPES, ids=lambda s: s[0].split(":")[0] + "+")
@pytest.mark.parametrize("section", ["big_iter", "big_i8"])
def test_batched_chain_kernels_against_host_arithmetic(section, shapes):
    if not BIG_EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(BIG_EXE), section, *shapes], capture_output=True, text=True, timeout=900)
    fails = "".join(ln + "\n" for ln in r.stdout.splitlines() if "FAIL" in ln or "bytes changed" in ln)
    print(r.stdout[-6000:])
    assert r.returncode == 0, fails[:6000] + r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout


@pytest.mark.parametrize("batches", [["1", "5"], ["64"]], ids=lambda b: "x".join(b))
def test_resident_chain_kernel_against_host_arithmetic(batches):
    if not BIG_EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(BIG_EXE), "res128", *batches], capture_output=True, text=True, timeout=900)
    fails = "".join(ln + "\n" for ln in r.stdout.splitlines() if "FAIL" in ln or "bytes changed" in ln)
    print(r.stdout[-6000:])
    assert r.returncode == 0, fails[:6000] + r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout


F64_EXE = EXE.with_name("nsf64_check")


def _f64_problem_file(path, shared):
    """Five problems of d = 33 in one batch -- full rank, rank-deficient, zero, NaN, an eigenvalue of -1e-9 -- as nsf64_check reads them:
    float64 little-endian [20250, d, B, B x (nonfinite, conv, iters, count may differ by one, exact tr sqrt, bound), B x cov1, B x cov2].
    shared: every problem has the first covariance of the full-rank pair (run_ns with stride 0), the second ones carry the cases."""
    spec = importlib.util.spec_from_file_location("frechet_f64_reference", Path(__file__).resolve().parent / "frechet_f64_reference.py")
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    d = 33
    _, F1, _, F2 = R.value_case(d, False, 1.0)
    _, D1, _, D2 = R.value_case(d, True, 1.0)
    _, N1, _, N2 = R.negative_case(-1e-9)
    bad = np.array(F2)
    bad[3, 4] = np.nan
    zero = np.zeros((d, d))
    if shared:
        pairs = [(F1, F2), (F1, D2), (F1, zero), (F1, bad), (F1, N1)]
    else:
        pairs = [(F1, F2), (D1, D2), (zero, F2), (bad, F1), (N1, N2)]
    head, c1, c2 = [20250.0, d, len(pairs)], [], []
    for C1, C2 in pairs:
        e = R.emulate(C1, C2)
        if e["nonfinite"]:
            head += [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        else:
            x = R.tr_sqrt_exact(C1, C2)
            head += [0.0, e["conv"], e["iters"], 0.0 if e["firm"] else 1.0, x, R.tr_sqrt_bound(e["tr_sqrt"], x, d) if e["rule"] != "zero" else 0.0]
        c1.append(np.ravel(C1))
        c2.append(np.ravel(C2))
    np.concatenate([np.array(head, dtype=np.float64), *c1, *c2]).astype("<f8").tofile(path)


@pytest.mark.parametrize("section", ["stats", "schedule", "first", "check", "run", "run_shared"])
def test_f64_iteration_kernels_against_host_arithmetic(section, tmp_path):
    if not F64_EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    args = [section]
    if section.startswith("run"):
        _f64_problem_file(tmp_path / "problems.f64", shared=section == "run_shared")
        args = ["run", str(tmp_path / "problems.f64")]
    r = subprocess.run([str(F64_EXE), *args], capture_output=True, text=True, timeout=900)
    fails = "".join(ln + "\n" for ln in r.stdout.splitlines() if "FAIL" in ln or "DRIFTED" in ln)
    print(r.stdout[-8000:])
    assert r.returncode == 0, fails[:6000] + r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
