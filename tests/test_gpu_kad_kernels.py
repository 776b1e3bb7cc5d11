"""The inverse-quadratic (iq) and inverse-multiquadric (imq) kernels of the KAD family on the GPU (fad_kad_k, fad_kad_individual_k,
fad_kad_uncertainty_k, fad_kad_permutation_test_k; csrc/kad.hip) against the float64 reference of tests/kad_kernels_reference.py on the
same values, upcast, at the tolerances of the Gaussian tests: the Gaussian _k entries return the old entries' bits; a closed form;
set-level accuracy over D, ragged sizes, dtypes and row pitches; the order of the three kernels; determinism and symmetry; per song;
standard errors; the permutation test with the literal shift and with the one from the sum pass; rows far from the origin; errors; the
command lines.  The shapes are the smallest that reach a diagonal tile, an off-diagonal tile, a padding row and a ragged k step."""
import ctypes as C
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kad_conditioning_reference as CR
import kad_kernels_reference as KR
import kad_permutation_reference as PMR
import test_gpu_kad as TK
import test_gpu_kad_uncertainty as TU
from test_gpu_kad import MEAN_RTOL, MMD_TOL
from test_gpu_kad_permutation import TAU
from test_gpu_kad_uncertainty import COV_RTOL

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NEW = ("iq", "imq")
TOO_FEW, NOT_FINITE, INVALID = -6, -7, -1
PARENTS = ("fad_kad", "fad_kad_individual", "fad_kad_uncertainty", "fad_kad_permutation_test")
assert COV_RTOL == 1e-4 and TAU == 1e-2 and MEAN_RTOL == 4e-7 and MMD_TOL == 1.5e-7


def _offsets(songs):
    return np.concatenate([[0], np.cumsum([len(y) for y in songs])]).astype(np.int64)


# ------------------------------------------------------------------------------------------- 1. old and new entries agree
class _OldEntries:
    """The library with every fad_kad*_k call sent to its parent entry, the kernel argument (FAD_KAD_GAUSSIAN) dropped."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        from fadtk_amd import _capi
        if name[:-2] in PARENTS and name.endswith("_k"):
            old = getattr(self._lib, name[:-2])
            at = _capi.SIGNATURES[name[:-2]][1].index(C.c_double) + 1

            def call(*a):
                assert a[at] == _capi.FAD_KAD_GAUSSIAN
                return old(*a[:at], *a[at + 1:])
            return call
        return getattr(self._lib, name)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        elif isinstance(a[k], list):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(a[k], b[k])), k
        else:
            assert a[k] == b[k], k


def test_gaussian_k_entries_return_what_the_old_entries_return(monkeypatch):
    from fadtk_amd import _capi, hip
    x, y = TK._sets(255, 257, 130, 1, seed=1)
    x, y = x.astype(np.float16), y.astype(np.float16)
    off = np.array([0, 1, 3, 130, 257], dtype=np.int64)
    u = hip.pack_labels(PMR.random_labellings(255, 257, 33, np.random.default_rng(2)))
    calls = (lambda: hip.kad(x, y, kernel="gaussian"), lambda: hip.kad(x, y, bandwidth=15.0, kernel="gaussian"),
             lambda: hip.kad_individual(x, y, off, kernel="gaussian"),
             lambda: hip.kad_uncertainty(x, [y, y[:2], y[:130]], rows=True, kernel="gaussian"),
             lambda: hip.kad_permutation_test(x, y, u, kernel="gaussian"),
             lambda: hip.kad_permutation_test(x, y, u, bandwidth=15.0, kernel="gaussian"))
    new = [call() for call in calls]
    old_lib = _OldEntries(_capi.load_library())
    monkeypatch.setattr(_capi, "load_library", lambda: old_lib)
    old = [call() for call in calls]
    for a, b in zip(new, old):
        _same(a, b)
    assert np.isfinite(new[0]["mmd2"]) and np.isnan(new[2]["mmd2"][0]) and np.all(np.isfinite(new[2]["mmd2"][1:]))


# ----------------------------------------------------------------------------------------------------------- 2. closed form
@pytest.mark.parametrize("kernel", KR.KERNELS)
def test_closed_form(kernel):
    """D = 8, x = {0, 2 e1}, y = {0, 2 e2, 2 e1 + 2 e2}, sigma = sqrt 2: t = d^2 / 4 is 1 for the x pair; 1, 2, 1 for the y pairs; 0, 1,
    2, 1, 2, 1 for the cross pairs.  Rows and every d^2 are small integers, so they are exact; two float32 ulps for each mean."""
    from fadtk_amd import hip
    x = np.zeros((2, 8), dtype=np.float16)
    y = np.zeros((3, 8), dtype=np.float16)
    x[1, 0] = 2
    y[1, 1] = 2
    y[2, 0] = y[2, 1] = 2
    k = {"gaussian": lambda t: math.exp(-t), "iq": lambda t: 1.0 / (1.0 + t), "imq": lambda t: 1.0 / math.sqrt(1.0 + t)}[kernel]
    want = {"kxx_mean": k(1), "kyy_mean": (2 * k(1) + k(2)) / 3, "kxy_mean": (k(0) + 3 * k(1) + 2 * k(2)) / 6}
    assert want["kxx_mean"] == pytest.approx({"gaussian": math.exp(-1), "iq": 0.5, "imq": 1 / math.sqrt(2)}[kernel], rel=1e-15)
    got = hip.kad(x, y, bandwidth=math.sqrt(2.0), kernel=kernel)
    print(f"[kad-kern-err] closed form {kernel}: " + " ".join(f"{q}={abs(got[q] - w) / w:.2e}" for q, w in want.items()))
    for q, w in want.items():
        assert abs(got[q] - w) <= 2.4e-7 * w, (kernel, q, got[q], w)
    assert got["bandwidth"] == math.sqrt(2.0) and got["n"] == 2 and got["m"] == 3


# ---------------------------------------------------------------------------------------------------- 3. set-level accuracy
@pytest.mark.parametrize("kernel", NEW)
@pytest.mark.parametrize("d,n,m", [(1, 255, 257), (17, 255, 257), (128, 2, 3), (512, 255, 257), (1280, 130, 129)])
def test_set_level_float16_matches_float64(d, n, m, kernel):
    from fadtk_amd import hip
    x, y = TK._sets(n, m, d, 1, seed=d + n)
    x16, y16 = x.astype(np.float16), y.astype(np.float16)
    got = hip.kad(x16, y16, kernel=kernel)
    assert got["bandwidth"] == hip.kad_median_distance(x16)                     # the default bandwidth is the median for every kernel
    assert got["bandwidth"] == pytest.approx(KR.median_distance(x16), rel=1e-5)
    TK._check(got, KR.kad(x16, y16, got["bandwidth"], kernel), f"{kernel} f16 d={d} n={n} m={m}")


@pytest.mark.parametrize("kernel", NEW)
@pytest.mark.parametrize("dtype", ["bfloat16", "float32", "float16"])
@pytest.mark.parametrize("d,ld", [(17, 24), (512, 520)])
def test_set_level_dtypes_and_row_pitch_on_device(dtype, d, ld, kernel):
    import torch
    from fadtk_amd import hip
    x, y = TK._sets(700, 333, d, 1, seed=ld)
    tdt = getattr(torch, dtype)
    xw = torch.zeros((700, ld), dtype=tdt, device="cuda")
    yw = torch.zeros((333, ld), dtype=tdt, device="cuda")
    xw[:, :d] = torch.from_numpy(x).to(tdt)
    yw[:, :d] = torch.from_numpy(y).to(tdt)
    xv, yv = xw[:, :d], yw[:, :d]                         # ld > D, used in place
    got = hip.kad(xv, yv, kernel=kernel)
    xr, yr = xv.float().cpu().numpy(), yv.float().cpu().numpy()
    TK._check(got, KR.kad(xr, yr, got["bandwidth"], kernel), f"{kernel} {dtype} d={d} ld={ld}")
    if dtype == "float32":                                # the host route of the same rows
        assert hip.kad(np.ascontiguousarray(xr), np.ascontiguousarray(yr), kernel=kernel) == got


# ------------------------------------------------------------------------------------------ 4., 5. order, determinism, symmetry
def test_the_three_kernels_are_in_order():
    """e^-t <= 1 / (1 + t) <= 1 / sqrt(1 + t) pair by pair, strictly for t > 0: two kernels swapped in a dispatch table show here."""
    from fadtk_amd import hip
    x, y = TK._sets(255, 257, 17, 1, seed=3)
    x, y = x.astype(np.float16), y.astype(np.float16)
    g, q, s = (hip.kad(x, y, bandwidth=6.0, kernel=k) for k in KR.KERNELS)
    for key in ("kxx_mean", "kyy_mean", "kxy_mean"):
        assert g[key] < q[key] < s[key], (key, g[key], q[key], s[key])
    ind = [hip.kad_individual(x, y, [0, 130, 257], bandwidth=6.0, kernel=k) for k in KR.KERNELS]
    unc = [hip.kad_uncertainty(x, [y], bandwidth=6.0, kernel=k) for k in KR.KERNELS]
    u = hip.pack_labels(PMR.random_labellings(255, 257, 3, np.random.default_rng(0)))
    perm = [hip.kad_permutation_test(x, y, u, bandwidth=6.0, kernel=k) for k in KR.KERNELS]
    for res in (ind, unc, perm):
        assert res[0]["kxx_mean"] < res[1]["kxx_mean"] < res[2]["kxx_mean"]
        assert np.all(res[0]["kyy_mean"] < res[1]["kyy_mean"]) and np.all(res[1]["kyy_mean"] < res[2]["kyy_mean"])


def test_iq_is_deterministic_and_symmetric():
    import torch
    from fadtk_amd import hip
    x, y = TK._sets(300, 257, 130, 1, seed=11)
    xd, yd = torch.from_numpy(x).half().cuda(), torch.from_numpy(y).half().cuda()
    a, b = hip.kad(xd, yd, kernel="iq"), hip.kad(xd, yd, kernel="iq")
    assert a == b                                         # bitwise: no float atomics anywhere
    s1 = hip.kad(xd, yd, bandwidth=a["bandwidth"], kernel="iq")
    s2 = hip.kad(yd, xd, bandwidth=a["bandwidth"], kernel="iq")
    assert s1 == a
    assert s1["kxx_mean"] == s2["kyy_mean"] and s1["kyy_mean"] == s2["kxx_mean"]
    assert s1["kxy_mean"] == pytest.approx(s2["kxy_mean"], rel=1e-12)
    assert s1["mmd2"] == pytest.approx(s2["mmd2"], rel=1e-12, abs=1e-15)


# ----------------------------------------------------------------------------------------------------------------- 6. per song
@pytest.mark.parametrize("kernel", NEW)
@pytest.mark.parametrize("d", [17, 768])
def test_per_song_matches_float64_and_the_set_level_entry(d, kernel):
    from fadtk_amd import hip
    lengths = [0, 1, 2, 3, 127, 128, 129, 300]
    rng = np.random.default_rng(d)
    x = rng.standard_normal((257, d)).astype(np.float16)
    songs = [(rng.standard_normal((m, d)) * (1.0 + 0.05 * (s % 3)) + 0.3 * (s % 2)).astype(np.float16) for s, m in enumerate(lengths)]
    rows, off = np.concatenate(songs), _offsets(songs)
    got = hip.kad_individual(x, rows, off, kernel=kernel)
    sigma = got["bandwidth"]
    assert sigma == hip.kad_median_distance(x)
    kxx, _, want = KR.kad_individual(x, songs, sigma, kernel)
    assert got["kxx_mean"] == pytest.approx(kxx, rel=MEAN_RTOL) and got["n"] == 257
    worst = 0.0
    for s, y in enumerate(songs):
        if len(y) < 2:
            assert want[s] is None and got["status"][s] == TOO_FEW and np.isnan(got["mmd2"][s]) and np.isnan(got["kyy_mean"][s])
            continue
        assert got["status"][s] == 0
        one = hip.kad(x, y, bandwidth=sigma, kernel=kernel)
        assert one["kxx_mean"] == got["kxx_mean"]                                  # the baseline term: the same launches and sum
        for ref, name in ((want[s], "float64"), (one, "fad_kad_k")):
            scale = ref["kxx_mean"] + ref["kyy_mean"] + 2 * ref["kxy_mean"]
            for k in ("kyy_mean", "kxy_mean"):
                worst = max(worst, abs(got[k][s] - ref[k]) / ref[k])
                assert got[k][s] == pytest.approx(ref[k], rel=MEAN_RTOL), (name, s, k, got[k][s], ref[k])
            assert abs(got["mmd2"][s] - ref["mmd2"]) <= MMD_TOL * scale, (name, s, got["mmd2"][s], ref["mmd2"])
    print(f"[kad-kern-err] per song {kernel} d={d}: worst mean rel {worst:.2e}")

    bad = rows.copy()
    bad[off[6] + 5, 0] = np.nan                                                    # one row of the song of 129 rows
    a, g = hip.kad_individual(x, bad, off, kernel=kernel), hip.kad_individual(x, bad, off)
    assert np.array_equal(a["status"], g["status"]) and a["status"][6] == NOT_FINITE and np.isnan(a["mmd2"][6])
    assert list(a["status"][:2]) == [TOO_FEW, TOO_FEW]
    keep = np.arange(len(songs)) != 6
    for k in ("mmd2", "kyy_mean", "kxy_mean"):
        assert a[k][keep].tobytes() == got[k][keep].tobytes(), k                  # the other songs do not depend on it


# -------------------------------------------------------------------------------------------------------------- 7. uncertainty
@pytest.mark.parametrize("kernel", NEW)
@pytest.mark.parametrize("d", [17, 512])
def test_uncertainty_matches_float64(d, kernel):
    from fadtk_amd import hip
    x, ys = TU._sets(255, [257, 2, 130], d, [1, 2, 3], seed=d)
    x16, ys16 = x.astype(np.float16), [y.astype(np.float16) for y in ys]
    got = hip.kad_uncertainty(x16, ys16, rows=True, kernel=kernel)
    assert got["bandwidth"] == hip.kad_median_distance(x16)
    TU._check(got, KR.uncertainty(x16, ys16, got["bandwidth"], kernel), f"{kernel} f16 d={d}")
    single = hip.kad(x16, ys16[0], bandwidth=got["bandwidth"], kernel=kernel)
    scale = single["kxx_mean"] + single["kyy_mean"] + 2 * single["kxy_mean"]
    assert abs(got["mmd2"][0] - single["mmd2"]) <= MEAN_RTOL * scale
    for k, v in (("kxx_mean", got["kxx_mean"]), ("kyy_mean", got["kyy_mean"][0]), ("kxy_mean", got["kxy_mean"][0])):
        assert v == pytest.approx(single[k], rel=MEAN_RTOL), k


# ----------------------------------------------------------------------------------------------------------- 8. permutation test
def _perm_sets(n, m, d, dtype, seed):
    import torch
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * 1.05 + 0.1).astype(np.float32)
    if dtype == "bf16":
        xt, yt = torch.from_numpy(x).cuda().bfloat16(), torch.from_numpy(y).cuda().bfloat16()
        return xt, yt, xt.double().cpu().numpy(), yt.double().cpu().numpy()
    x, y = x.astype(np.float16 if dtype == "f16" else np.float32), y.astype(np.float16 if dtype == "f16" else np.float32)
    return x, y, x.astype(np.float64), y.astype(np.float64)


@pytest.mark.parametrize("given", [False, True], ids=["pooled-median", "given-bandwidth"])
@pytest.mark.parametrize("kernel", NEW)
@pytest.mark.parametrize("dtype,d,n,m,P", [("f16", 128, 2, 2, 1), ("f16", 3, 127, 129, 128), ("f16", 512, 128, 160, 129),
                                           ("bf16", 128, 127, 129, 129), ("f32", 17, 31, 97, 1000)])
def test_permutation_matches_float64_reference(dtype, d, n, m, P, kernel, given):
    """Every statistic within TAU of the reference null's standard deviation.  The pooled-median bandwidth takes the literal shift
    (k at t = 1/2); a given one -- 1.3 times the float64 pooled median -- takes the mean kernel value from the sum pass."""
    from fadtk_amd import hip
    x, y, xr, yr = _perm_sets(n, m, d, dtype, seed=d + n + m + P)
    label = f"{kernel} {dtype} D={d} n={n} m={m} P={P} {'given' if given else 'median'}"
    rng = np.random.default_rng(P)
    u = PMR.random_labellings(n, m, P, rng)
    bandwidth = 1.3 * PMR.median_distance_pooled(xr, yr) if given else None
    got = hip.kad_permutation_test(x, y, hip.pack_labels(u), bandwidth=bandwidth, kernel=kernel)
    sigma = got["bandwidth"]
    if given:
        assert sigma == bandwidth
    elif isinstance(x, np.ndarray):                                            # the pooled median, bit for bit
        assert sigma == hip.kad_median_distance(np.concatenate([x, y]))
    else:
        import torch
        assert sigma == hip.kad_median_distance(torch.cat([x, y]))
    t = KR.statistics(xr, yr, np.concatenate([PMR.observed_labelling(n, m), u]), sigma, kernel)
    t0, null = t[0], t[1:]
    spread = null if P >= 50 else KR.statistics(xr, yr, PMR.random_labellings(n, m, 200, rng), sigma, kernel)
    sd = float(np.std(spread))
    tau = TAU * sd
    err = max(abs(got["mmd2"] - t0), float(np.max(np.abs(got["null"] - null))))
    print(f"[kad-kern-perm-err] {label}: max |dt| / sd = {err / sd:.2e}")
    assert abs(got["mmd2"] - t0) <= tau, (label, got["mmd2"], t0, tau)
    assert np.max(np.abs(got["null"] - null)) <= tau, (label, np.max(np.abs(got["null"] - null)), tau)
    kad = hip.kad(x, y, bandwidth=sigma, kernel=kernel)
    assert abs(got["mmd2"] - kad["mmd2"]) <= tau, (label, got["mmd2"], kad["mmd2"])
    if not np.any(np.abs(null - t0) <= 4 * tau):
        assert got["p_value"] == PMR.p_value(t0, null), (label, got["p_value"], PMR.p_value(t0, null))


# -------------------------------------------------------------------------------------------------------------- 9. conditioning
def _rows(a, dt):
    """float32 values that are exact in dt -> fp16 and fp32 numpy on the host, bf16 a torch tensor on the device"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert np.array_equal(CR.round_to(a, dt), a), dt
    if dt == "bf16":
        return torch.from_numpy(a).cuda().bfloat16()
    return a.astype(np.float16) if dt == "fp16" else a


@pytest.mark.parametrize("kernel", NEW)
@pytest.mark.parametrize("dt", ("fp16", "bf16", "fp32"))
@pytest.mark.parametrize("d,off", [(d, off) for off in (4, 16) for d in (17, 512)])
def test_rows_far_from_the_origin_within_what_float32_allows(d, off, dt, kernel):
    """kappa = 9 and 130: every mean within MEAN_RTOL + 4 A kappa of float64, A the Gaussian's own constant (the sensitivity of k to t
    is at most 1 for iq and 1/2 for imq; tests/test_kad_kernels_host.py holds the float32 emulation to the same bound)."""
    from fadtk_amd import hip
    c = CR.gauss_case(d, off, dt)
    tol = MEAN_RTOL + 4 * CR.conditioning_constant(dt) * c["kappa"]
    got = hip.kad(_rows(c["x"], dt), _rows(c["y"], dt), bandwidth=c["sigma"], kernel=kernel)
    want = KR.kad(c["x"], c["y"], c["sigma"], kernel)
    err = CR.mean_errors(got, want)
    print(f"[kad-kern-cond] {kernel} {dt} d={d} off={off}: kappa {c['kappa']:.1f} tol {tol:.2e}; " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    for k in CR.MEANS + ("mmd2",):
        assert err[k] <= tol, (k, err[k], tol)


# ------------------------------------------------------------------------------------------------------------------- 10. errors
@pytest.mark.parametrize("kernel", NEW)
def test_errors_on_device(kernel):
    from fadtk_amd import hip
    x = np.random.default_rng(0).standard_normal((50, 16)).astype(np.float16)
    bad = x.copy()
    bad[7, 3] = np.inf
    with pytest.raises(ValueError):
        hip.kad(bad, x, kernel=kernel)
    same = np.repeat(np.round(x[:1] * 4), 10, axis=0).astype(np.float16)          # every baseline distance is exactly 0
    with pytest.raises(RuntimeError, match="must be > 0"):
        hip.kad(same, x, kernel=kernel)
    with pytest.raises(ValueError):
        hip.kad(x, x, bandwidth=-1.0, kernel=kernel)
    with pytest.raises(RuntimeError, match="float32 range"):                       # c = 1 / sigma^2 past float32
        hip.kad(x, x, bandwidth=1e-30, kernel=kernel)
    assert np.isfinite(hip.kad(x, x[:20], kernel=kernel)["mmd2"])                  # the call after errors


def test_unknown_kernel_code_is_invalid():
    from fadtk_amd import _capi, hip
    lib = _capi.load_library()
    x = np.random.default_rng(1).standard_normal((8, 4)).astype(np.float32)
    off = np.array([0, 8], dtype=np.int64)
    lab = hip.pack_labels(PMR.random_labellings(8, 8, 2, np.random.default_rng(0)))
    res, out, st, pv = _capi.FadKadResult(), np.zeros(4), np.zeros(1, dtype=np.int32), C.c_double()
    ptrs, ms, lds = (C.c_void_p * 1)(x.ctypes.data), np.array([8], dtype=np.int64), np.array([4], dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    p = x.ctypes.data
    calls = {
        "fad_kad": lambda k: lib.fad_kad_k(p, 8, 4, p, 8, 4, 4, _capi.FAD_F32, 0, 0.0, k, C.byref(res), 0, None),
        "fad_kad_individual": lambda k: lib.fad_kad_individual_k(p, 8, 4, p, 8, 4, off.ctypes.data_as(i64p), 1, 4, _capi.FAD_F32, 0, 0.0, k,
                                                                 C.byref(res), out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                                                 st.ctypes.data, 0, None),
        "fad_kad_uncertainty": lambda k: lib.fad_kad_uncertainty_k(p, 8, 4, ptrs, ms.ctypes.data_as(i64p), lds.ctypes.data_as(i64p), 1, 4,
                                                                   _capi.FAD_F32, 0, 0.0, k, C.byref(res), out.ctypes.data, None, None, 0, None),
        "fad_kad_permutation_test": lambda k: lib.fad_kad_permutation_test_k(p, 8, 4, p, 8, 4, 4, _capi.FAD_F32, 0, 0.0, k, lab.ctypes.data, 2,
                                                                             0, C.byref(res), out.ctypes.data, C.byref(pv), 0, None),
    }
    for name, call in calls.items():
        for k in (7, -1, 3):
            assert call(k) == INVALID, (name, k)
            msg = _capi.last_error()
            assert name in msg and f"kernel {k}" in msg, msg
        assert call(_capi.FAD_KAD_IMQ) == 0, (name, _capi.last_error())


# ------------------------------------------------------------------------------------------------------------ 11. command lines
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """Six tiny cached files per directory (the fixture of test_kad_cli_end_to_end) -> (run, base dir, eval dir, x rows, y rows)"""
    from fadtk_amd import FrechetAudioDistance
    from fadtk_amd.model_loader import get_all_models
    tmp = tmp_path_factory.mktemp("kad_kernels_cli")
    rng = np.random.default_rng(5)
    for name, shift in (("base", 0.0), ("evl", 0.4)):
        d = tmp / name
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i in range(6):
            (d / f"s{i}.wav").write_bytes(b"")             # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"s{i}.npy", (rng.standard_normal((40 + 7 * i, 128)) + shift).astype(np.float32))
    env = dict(os.environ, PYTHONPATH=str(ROOT))

    def run(module, *args):
        r = subprocess.run([sys.executable, "-m", module, "vggish", *args, "-w", "2"], capture_output=True, text=True, cwd=tmp, env=env,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return r
    ml = {m.name: m for m in get_all_models()}["vggish"]
    fad = FrechetAudioDistance(ml, load_model=False)
    return run, tmp, str(tmp / "base"), str(tmp / "evl"), fad.load_embeddings(tmp / "base"), fad.load_embeddings(tmp / "evl")


def test_kad_command_line_with_a_kernel_writes_the_extended_csv(cli):
    from fadtk_amd import calc_kernel_audio_distance
    run, tmp, base, evl, x, y = cli
    csv = tmp / "iq.csv"
    run("fadtk_amd.kad", base, evl, str(csv), "--scale", "10", "--kernel", "iq")
    lines = csv.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,kad,bandwidth,scale,time,kernel" and len(lines) == 2
    row = lines[1].split(",")
    value, res = calc_kernel_audio_distance(x, y, scale=10.0, details=True, kernel="iq")
    assert float(row[3]) == value and float(row[4]) == res["bandwidth"] and float(row[5]) == 10.0 and row[7] == "iq" and len(row) == 8
    assert value == pytest.approx(10 * KR.kad(x, y, None, "iq")["mmd2"], rel=1e-4)


def test_kad_command_line_without_the_flag_writes_the_plain_csv(cli):
    from fadtk_amd import calc_kernel_audio_distance
    run, tmp, base, evl, x, y = cli
    plain = tmp / "plain.csv"
    run("fadtk_amd.kad", base, evl, str(plain), "--scale", "10")
    lines = plain.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,kad,bandwidth,scale,time" and len(lines) == 2 and len(lines[1].split(",")) == 7
    assert float(lines[1].split(",")[3]) == calc_kernel_audio_distance(x, y, scale=10.0)


def test_kad_compare_command_line_with_a_kernel(cli):
    run, tmp, base, evl, x, y = cli
    csv = tmp / "cmp.csv"
    run("fadtk_amd.kad_compare", base, evl, base, "--csv", str(csv), "--kernel", "imq")
    lines = csv.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,kad,stderr,bandwidth,scale,kernel" and len(lines) == 3
    assert all(line.split(",")[-1] == "imq" and len(line.split(",")) == 8 for line in lines[1:])
    assert float(lines[1].split(",")[3]) == pytest.approx(KR.kad(x, y, None, "imq")["mmd2"], rel=1e-4)


def test_kad_permutation_command_line_with_a_kernel(cli):
    run, tmp, base, evl, x, y = cli
    csv = tmp / "perm.csv"
    run("fadtk_amd.kad_permutation", base, evl, str(csv), "-p", "99", "--kernel", "imq")
    lines = csv.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,kad,p_value,permutations,seed,bandwidth,scale,time,kernel" and len(lines) == 2
    row = lines[1].split(",")
    assert row[-1] == "imq" and float(row[4]) == 0.01 and int(row[5]) == 99        # a shift of 0.4 per coordinate: no labelling reaches t_0
    assert float(row[3]) == pytest.approx(KR.kad(x, y, float(row[7]), "imq")["mmd2"], rel=1e-3)
