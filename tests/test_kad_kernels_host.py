"""The inverse-quadratic and inverse-multiquadric KAD kernels on the host: the float64 reference of tests/kad_kernels_reference.py
against the Gaussian references and against brute-force double loops; the float32-chain emulation of the new epilogue inside the
conditioning bound the GPU tests hold; the Python entries refuse an unknown kernel before the library loads; the header, the ctypes
table and the command lines carry the kernel; the CSV rule of the command lines.  No GPU needed."""
import inspect
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kad_conditioning_reference as CR
import kad_kernels_reference as KR
import kad_permutation_reference as PMR
import kad_reference as R
import kad_uncertainty_reference as U
from test_gpu_kad import MEAN_RTOL, MMD_TOL          # importing that module needs no GPU

ROOT = Path(__file__).resolve().parent.parent
NEW = ("iq", "imq")
DTYPES = ("fp16", "bf16", "fp32")


def _sets(n, m, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)), rng.standard_normal((m, d)) * 1.1 + 0.3


# ------------------------------------------------------------------------------------------------------------ the reference
def test_gaussian_reference_equals_the_existing_references():
    x, y = _sets(40, 33, 9, seed=1)
    y2 = _sets(2, 21, 9, seed=2)[1]
    for sigma in (None, 3.7):
        got, want = KR.kad(x, y, sigma, "gaussian"), R.kad(x, y, sigma)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-13), k
        gu, wu = KR.uncertainty(x, [y, y2], sigma, "gaussian"), U.uncertainty(x, [y, y2], sigma)
        for s in range(2):
            for k in wu["sets"][s]:
                assert gu["sets"][s][k] == pytest.approx(wu["sets"][s][k], rel=1e-13), (s, k)
            np.testing.assert_allclose(gu["proj_y"][s], wu["proj_y"][s], rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(gu["cov"], wu["cov"], rtol=1e-13, atol=1e-18)
        np.testing.assert_allclose(gu["proj_x"], wu["proj_x"], rtol=1e-13, atol=1e-15)
        u = np.concatenate([PMR.observed_labelling(40, 33), PMR.random_labellings(40, 33, 17, np.random.default_rng(3))])
        np.testing.assert_allclose(KR.statistics(x, y, u, sigma, "gaussian"), PMR.statistics(x, y, u, sigma), rtol=1e-13, atol=1e-15)
    kxx, sigma, songs = KR.kad_individual(x, [y, y[:1], y2], None, "gaussian")
    assert songs[1] is None and sigma == R.median_distance(x)
    for got, ys in ((songs[0], y), (songs[2], y2)):
        want = R.kad(x, ys, sigma)
        for k in ("mmd2", "kxx_mean", "kyy_mean", "kxy_mean"):
            assert got[k] == pytest.approx(want[k], rel=1e-13), k


def _k_scalar(a, b, sigma, kernel):
    t = sum((p - q) ** 2 for p, q in zip(a, b)) / (2.0 * sigma * sigma)
    return {"iq": 1.0 / (1.0 + t), "imq": 1.0 / math.sqrt(1.0 + t)}[kernel]


@pytest.mark.parametrize("kernel", NEW)
def test_reference_equals_brute_force_double_loops(kernel):
    n, m, d, sigma = 5, 7, 3, 1.3
    x, y = _sets(n, m, d, seed=4)
    k = lambda a, b: _k_scalar(a, b, sigma, kernel)          # noqa: E731
    kxx = sum(k(x[i], x[j]) for i in range(n) for j in range(n) if i != j) / (n * (n - 1))
    kyy = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j) / (m * (m - 1))
    kxy = sum(k(x[i], y[j]) for i in range(n) for j in range(m)) / (n * m)
    got = KR.kad(x, y, sigma, kernel)
    for key, want in (("kxx_mean", kxx), ("kyy_mean", kyy), ("kxy_mean", kxy), ("mmd2", kxx + kyy - 2 * kxy)):
        assert got[key] == pytest.approx(want, rel=1e-13, abs=1e-15), key

    _, _, songs = KR.kad_individual(x, [y[:3], y[3:4], y[4:]], sigma, kernel)          # songs of 3, 1 and 3 rows
    assert songs[1] is None
    for got_s, ys in ((songs[0], y[:3]), (songs[2], y[4:])):
        ms = len(ys)
        syy = sum(k(ys[i], ys[j]) for i in range(ms) for j in range(ms) if i != j) / (ms * (ms - 1))
        sxy = sum(k(x[i], ys[j]) for i in range(n) for j in range(ms)) / (n * ms)
        assert got_s["kyy_mean"] == pytest.approx(syy, rel=1e-13) and got_s["kxy_mean"] == pytest.approx(sxy, rel=1e-13)
        assert got_s["mmd2"] == pytest.approx(kxx + syy - 2 * sxy, rel=1e-12, abs=1e-15)

    # uncertainty: the definitions of include/fad_hip.h, pair by pair
    a = [sum(k(x[i], x[j]) for j in range(n) if j != i) / (n - 1) - sum(k(x[i], y[l]) for l in range(m)) / m for i in range(n)]
    b = [sum(k(y[l], y[q]) for q in range(m) if q != l) / (m - 1) - sum(k(x[i], y[l]) for i in range(n)) / n for l in range(m)]
    ma, mb = sum(a) / n, sum(b) / m
    cov = 4.0 / (n * (n - 1)) * sum((v - ma) ** 2 for v in a) + 4.0 / (m * (m - 1)) * sum((v - mb) ** 2 for v in b)
    gu = KR.uncertainty(x, [y], sigma, kernel)
    np.testing.assert_allclose(gu["proj_x"][0], a, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(gu["proj_y"][0], b, rtol=1e-13, atol=1e-15)
    assert gu["cov"][0, 0] == pytest.approx(cov, rel=1e-12) and gu["sets"][0]["mmd2"] == pytest.approx(ma + mb, rel=1e-12, abs=1e-15)

    # permutation statistics: MMD^2 of the relabelled groups, by loops
    z = np.concatenate([x, y])
    u = np.concatenate([PMR.observed_labelling(n, m), PMR.random_labellings(n, m, 6, np.random.default_rng(5))])
    got_t = KR.statistics(x, y, u, sigma, kernel)
    for row, t in zip(u, got_t):
        g1, g0 = np.flatnonzero(row), np.flatnonzero(~row)
        s11 = sum(k(z[i], z[j]) for i in g1 for j in g1 if i != j) / (n * (n - 1))
        s00 = sum(k(z[i], z[j]) for i in g0 for j in g0 if i != j) / (m * (m - 1))
        s10 = sum(k(z[i], z[j]) for i in g1 for j in g0) / (n * m)
        assert t == pytest.approx(s11 + s00 - 2 * s10, rel=1e-11, abs=1e-14)
    assert got_t[0] == pytest.approx(got["mmd2"], rel=1e-11, abs=1e-14)


def test_kernels_are_ordered_and_meet_at_zero():
    t = np.linspace(0.0, 50.0, 501)
    g, q, s = (KR.kernel_of_t(t, k) for k in KR.KERNELS)
    assert np.all(g <= q) and np.all(q <= s) and g[0] == q[0] == s[0] == 1.0
    assert KR.kernel_of_t(0.5, "iq") == pytest.approx(2.0 / 3.0, rel=1e-15)           # the permutation test's literal shifts
    assert KR.kernel_of_t(0.5, "imq") == pytest.approx(0.81649658092772603, rel=1e-15)
    assert float(np.float32(0.81649658092772603)) == pytest.approx(1.0 / math.sqrt(1.5), rel=6e-8)
    with pytest.raises(ValueError):
        KR.kernel_of_t(t, "laplace")


# ------------------------------------------------------------------------------------------------- the float32 emulation
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d,off", CR.GAUSS_CASES)
@pytest.mark.parametrize("kernel", NEW)
def test_float32_chain_of_the_new_epilogue_meets_the_conditioning_bound(kernel, d, off, dt):
    """The bound the GPU conditioning test holds, MEAN_RTOL + 4 A kappa with the Gaussian's own A, asked of the float32 emulation of
    the chain and the fma / max / reciprocal epilogue: the condition that the reference alone passes.  (k's sensitivity to an error in
    t is 1 / (1 + t) for iq and 1 / (2 (1 + t)) for imq, against 1 for the Gaussian.)"""
    c = CR.gauss_case(d, off, dt)
    tol = MEAN_RTOL + 4 * CR.conditioning_constant(dt) * c["kappa"]
    want = KR.kad(c["x"], c["y"], c["sigma"], kernel)
    err = CR.mean_errors(KR.chain32_means(c["x"], c["y"], c["sigma"], CR.STEP[dt], kernel), want)
    print(f"[kad-kern-host] {kernel} {dt} d={d} off={off}: kappa {c['kappa']:.1f}; chain32 " + " ".join(f"{k}={v:.2e}" for k, v in err.items())
          + f"; bound {tol:.2e}; gaussian " + " ".join(f"{k}={v:.2e}" for k, v in c["chain_err"].items()))
    for k in CR.MEANS:
        assert err[k] <= tol, (k, err[k], tol)
    assert err["mmd2"] <= tol


@pytest.mark.parametrize("kernel", NEW)
def test_float32_chain_at_the_origin_meets_the_plain_tolerances(kernel):
    """Offset 0, and the tiny n = 2 / m = 3 case: MEAN_RTOL per mean and MMD_TOL of the scale, from the emulation alone."""
    for dt in DTYPES:
        for d in (17, 128, 512):
            x, y = CR.gauss_sets(d, 0, dt)
            sigma = KR.median_distance(x)
            err = CR.mean_errors(KR.chain32_means(x, y, sigma, CR.STEP[dt], kernel), KR.kad(x, y, sigma, kernel))
            assert max(err[k] for k in CR.MEANS) <= MEAN_RTOL and err["mmd2"] <= MMD_TOL, (dt, d, err)
    x, y = CR.gauss_sets(128, 0, "fp16")
    x, y = x[:2], y[:3]
    sigma = KR.median_distance(x)
    err = CR.mean_errors(KR.chain32_means(x, y, sigma, 16, kernel), KR.kad(x, y, sigma, kernel))
    assert max(err[k] for k in CR.MEANS) <= MEAN_RTOL and err["mmd2"] <= MMD_TOL, err


def test_epilogue_emulation_edges():
    acc = np.array([-np.inf, np.float32(1e-3), 0.0, -0.5, -1.5], dtype=np.float32)          # padding row, rounding residue, t = 0, 1/2, 3/2
    for kernel, at_half in (("iq", 2.0 / 3.0), ("imq", 1.0 / math.sqrt(1.5))):
        k = KR.epilogue32(acc, 1.0, kernel)
        assert k[0] == 0.0 and k[1] == 1.0 and k[2] == 1.0
        assert k[3] == pytest.approx(at_half, rel=1.2e-7) and k[4] == pytest.approx(KR.kernel_of_t(1.5, kernel), rel=1.2e-7)


# --------------------------------------------------------------------------------------------------------- Python entries
def test_unknown_kernel_is_a_value_error_before_the_library_loads(monkeypatch):
    import fadtk_amd
    from fadtk_amd import _capi, hip, kad

    def no_library(*a, **k):
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(_capi, "load_library", no_library)
    x = np.zeros((4, 3), dtype=np.float32)
    u = np.zeros((1, 8), dtype=bool)
    u[0, :4] = True
    calls = [
        lambda k: hip.kad(x, x, kernel=k),
        lambda k: hip.kad_individual(x, x, [0, 4], kernel=k),
        lambda k: hip.kad_uncertainty(x, [x], kernel=k),
        lambda k: hip.kad_permutation_test(x, x, u, kernel=k),
        lambda k: fadtk_amd.calc_kernel_audio_distance(x, x, kernel=k),
        lambda k: fadtk_amd.calc_kernel_audio_distance_individual(x, [x], kernel=k),
        lambda k: fadtk_amd.calc_kernel_audio_distance_uncertainty(x, [x], kernel=k),
        lambda k: fadtk_amd.calc_kernel_audio_distance_permutation_test(x, x, labels=u, kernel=k),
    ]
    obj = kad.KernelAudioDistance.__new__(kad.KernelAudioDistance)              # no model, no files: the check comes first
    calls += [
        lambda k: obj.score("a", "b", kernel=k),
        lambda k: obj.score_many("a", ["b"], kernel=k),
        lambda k: obj.permutation_test("a", "b", kernel=k),
        lambda k: obj.score_individual("a", "b", "c.csv", kernel=k),
    ]
    for call in calls:
        for bad in ("laplace", "IQ", "", None, 1):
            with pytest.raises(ValueError, match="kernel"):
                call(bad)
    assert [hip.kad_kernel_code(k) for k in ("gaussian", "iq", "imq")] == [0, 1, 2] and fadtk_amd.KAD_KERNELS == ("gaussian", "iq", "imq")
    for fn in (hip.kad, hip.kad_individual, hip.kad_uncertainty, hip.kad_permutation_test, kad.calc_kernel_audio_distance,
               kad.calc_kernel_audio_distance_individual, kad.calc_kernel_audio_distance_uncertainty,
               kad.calc_kernel_audio_distance_permutation_test, kad.KernelAudioDistance.score, kad.KernelAudioDistance.score_many,
               kad.KernelAudioDistance.permutation_test, kad.KernelAudioDistance.score_individual):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "kernel" and params[-1].default == "gaussian", fn          # trailing, Gaussian by default


def test_individual_batches_pass_the_kernel_on_with_the_first_sigma(monkeypatch):
    from fadtk_amd import hip, kad
    seen = []

    def fake(x, rows, off, bandwidth=None, device=0, kernel="gaussian"):
        seen.append((len(rows), bandwidth, kernel))
        S = len(off) - 1
        return {"mmd2": np.zeros(S), "kyy_mean": np.zeros(S), "kxy_mean": np.zeros(S), "status": np.zeros(S, dtype=np.int32),
                "kxx_mean": 0.5, "bandwidth": 2.25, "n": len(x)}
    monkeypatch.setattr(hip, "kad_individual", fake)
    x = np.zeros((4, 8), dtype=np.float32)
    songs = [np.zeros((3, 8), dtype=np.float32)] * 3
    kad.calc_kernel_audio_distance_individual(x, songs, kernel="imq", max_bytes=3 * 8 * 4)          # one song per call
    assert seen == [(3, None, "imq"), (3, 2.25, "imq"), (3, 2.25, "imq")]


# ------------------------------------------------------------------------------------------------------ header and ctypes
def test_header_declares_and_capi_binds_the_kernel_entries():
    from fadtk_amd import _capi
    text = (ROOT / "include" / "fad_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for parent in ("fad_kad", "fad_kad_individual", "fad_kad_uncertainty", "fad_kad_permutation_test"):
        name = parent + "_k"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        assert re.search(r"double\s+bandwidth\s*,\s*int\s+kernel\s*,", m.group(1)), name          # directly after the bandwidth
        mp = re.search(r"\bint\s+" + parent + r"\s*\(([^;]*)\)\s*;", code)
        strip = lambda s: re.sub(r"\s+", " ", s).strip()          # noqa: E731
        assert strip(m.group(1)).replace("double bandwidth, int kernel,", "double bandwidth,") == strip(mp.group(1)), name
        res, args = _capi.SIGNATURES[name]
        pres, pargs = _capi.SIGNATURES[parent]
        at = pargs.index(_capi.C.c_double) + 1
        assert res is pres and args == pargs[:at] + [_capi.C.c_int] + pargs[at:], name
    assert re.search(r"FAD_KAD_GAUSSIAN\s*=\s*0\s*,\s*FAD_KAD_IQ\s*=\s*1\s*,\s*FAD_KAD_IMQ\s*=\s*2", code)
    assert (_capi.FAD_KAD_GAUSSIAN, _capi.FAD_KAD_IQ, _capi.FAD_KAD_IMQ) == (0, 1, 2)
    assert "1e-8" in text and "gamma = 1 / (2 sigma^2)" in text                              # the convention and the toolkit's eps
    if _capi.LIB_PATH.exists():
        lib = _capi.load_library()
        assert all(hasattr(lib, p + "_k") for p in ("fad_kad", "fad_kad_individual", "fad_kad_uncertainty", "fad_kad_permutation_test"))


# ---------------------------------------------------------------------------------------------------------- command lines
@pytest.mark.parametrize("module", ["fadtk_amd.kad", "fadtk_amd.kad_compare", "fadtk_amd.kad_permutation"])
def test_command_line_help_lists_the_kernel(module):
    import os
    r = subprocess.run([sys.executable, "-m", module, "--help"], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=str(ROOT)), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--kernel" in r.stdout and "{gaussian,iq,imq}" in r.stdout


@pytest.mark.parametrize("module", ["kad", "kad_compare", "kad_permutation"])
def test_csv_rule(module, tmp_path):
    import importlib
    from fadtk_amd.kad import append_csv
    header = importlib.import_module(f"fadtk_amd.{module}").CSV_HEADER
    plain, ext = tmp_path / "plain.csv", tmp_path / "ext.csv"
    append_csv(plain, header, ["a,1"])                                          # no kernel given, and the Gaussian by name: today's bytes
    append_csv(plain, header, ["b,2"], "gaussian")
    assert plain.read_bytes() == (header + "a,1\nb,2\n").encode()
    append_csv(ext, header, ["a,1"], "iq")
    append_csv(ext, header, ["b,2", "c,3"], "imq")
    assert ext.read_text() == header.rstrip("\n") + ",kernel\na,1,iq\nb,2,imq\nc,3,imq\n"
    for target, kernel in ((plain, "iq"), (plain, "imq"), (ext, "gaussian")):
        before = target.read_bytes()
        with pytest.raises(ValueError) as e:
            append_csv(target, header, ["z,9"], kernel)
        assert header.strip() + "'" in str(e.value) and header.strip() + ",kernel'" in str(e.value)          # both headers named
        assert target.read_bytes() == before                                      # no mixed file
    sub = tmp_path / "new" / "dir" / "k.csv"                                     # parents are made, as before
    append_csv(sub, header, ["a,1"], "imq")
    assert sub.read_text().splitlines()[0].endswith(",kernel")


def test_command_line_refuses_a_csv_of_the_other_form_before_any_work(tmp_path):
    import os
    from fadtk_amd.kad import CSV_HEADER
    csv = tmp_path / "kad.csv"
    csv.write_text(CSV_HEADER + "vggish,a,b,0.1,1.0,1.0,0.0\n")
    before = csv.read_bytes()
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "vggish", str(tmp_path / "none"), str(tmp_path / "none"), str(csv), "--kernel", "iq"],
                       capture_output=True, text=True, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=str(ROOT)), timeout=600)
    assert r.returncode != 0 and CSV_HEADER.strip() + "'" in r.stderr and CSV_HEADER.strip() + ",kernel'" in r.stderr, r.stderr[-2000:]
    assert csv.read_bytes() == before
