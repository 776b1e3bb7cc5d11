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
steps, and holds the trace estimate of <true>'s record against the tiled route of ns_fast.h and a host float64 correction."""
import subprocess
from pathlib import Path

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
