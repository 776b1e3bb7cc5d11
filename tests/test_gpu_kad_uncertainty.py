"""KAD standard errors on the GPU (fad_kad_uncertainty, csrc/kad.hip) against the float64 reference of
tests/kad_uncertainty_reference.py on the same 16-bit values, upcast: every mean, projection and covariance over D, dtypes, ragged
sizes and row pitches; agreement with fad_kad; bitwise determinism; errors; the estimate against the spread over independent draws;
the config-3 size against torch float64 row sums on the GPU; the kad_compare command line end to end."""
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


U = _load("kad_uncertainty_reference")
R = _load("kad_reference")

MEAN_RTOL = 4e-7            # test_gpu_kad.py's bound: means, MMD^2 and every projection against the kernel-mean scale
COV_RTOL = 1e-4


def _sets(n, ms, d, shifts, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    ys = [(rng.standard_normal((m, d)) * (1.0 + 0.1 * s) + 0.3 * s).astype(np.float32) for m, s in zip(ms, shifts)]
    return x, ys


def _check(got, want, label, cov=True):
    S = len(want["sets"])
    for s in range(S):
        w = want["sets"][s]
        scale = w["kxx_mean"] + w["kyy_mean"] + 2 * w["kxy_mean"]
        for k in ("kxx_mean", "kyy_mean", "kxy_mean"):
            g = got[k] if k == "kxx_mean" else got[k][s]
            assert g == pytest.approx(w[k], rel=MEAN_RTOL), (label, s, k)
        assert abs(got["mmd2"][s] - w["mmd2"]) <= MEAN_RTOL * scale, (label, s, got["mmd2"][s], w["mmd2"])
        if "proj_x" in got:
            assert np.max(np.abs(got["proj_x"][s] - want["proj_x"][s])) <= MEAN_RTOL * scale, (label, s, "proj_x")
            assert np.max(np.abs(got["proj_y"][s] - want["proj_y"][s])) <= MEAN_RTOL * scale, (label, s, "proj_y")
    if cov:
        err = np.max(np.abs(got["cov"] - want["cov"])) / np.max(np.abs(want["cov"]))
        print(f"[kad-unc-err] {label}: cov {err:.2e}")
        assert err <= COV_RTOL, (label, err)


CASES = [  # (d, n, ms, shifts)
    (1, 255, [257], [1]), (17, 300, [129, 2, 200], [1, 2, 3]), (128, 255, [257], [1]), (512, 400, [130, 333, 64], [2, 1, 3]),
    (1024, 255, [257], [2]),
]


@pytest.mark.parametrize("d,n,ms,shifts", CASES)
def test_kad_uncertainty_float16_matches_float64(d, n, ms, shifts):
    from fadtk_amd import hip
    x, ys = _sets(n, ms, d, shifts, seed=d + n)
    x16, ys16 = x.astype(np.float16), [y.astype(np.float16) for y in ys]
    got = hip.kad_uncertainty(x16, ys16, rows=True)
    assert got["bandwidth"] == pytest.approx(R.median_distance(x16), rel=1e-5)
    want = U.uncertainty(x16, ys16, sigma=got["bandwidth"])
    _check(got, want, f"f16 d={d} n={n} ms={ms}")
    assert np.array_equal(got["m"], ms) and got["n"] == n
    single = hip.kad(x16, ys16[0], bandwidth=got["bandwidth"])
    scale = single["kxx_mean"] + single["kyy_mean"] + 2 * single["kxy_mean"]
    assert abs(got["mmd2"][0] - single["mmd2"]) <= MEAN_RTOL * scale
    assert got["kxx_mean"] == pytest.approx(single["kxx_mean"], rel=MEAN_RTOL)


@pytest.mark.parametrize("dtype", ["bfloat16", "float32", "float16"])
@pytest.mark.parametrize("d,ld", [(17, 24), (128, 136), (512, 520)])
def test_kad_uncertainty_dtypes_and_row_pitch_on_device(dtype, d, ld):
    import torch
    from fadtk_amd import hip
    x, ys = _sets(700, [333, 129, 5], d, [1, 2, 1], seed=ld)
    tdt = getattr(torch, dtype)

    def wide(a):
        w = torch.zeros((a.shape[0], ld), dtype=tdt, device="cuda")
        w[:, :d] = torch.from_numpy(a).to(tdt)
        return w[:, :d]                                   # ld > D, used in place
    xv, yv = wide(x), [wide(y) for y in ys]
    got = hip.kad_uncertainty(xv, yv, rows=True)
    xr, yr = xv.float().cpu().numpy(), [y.float().cpu().numpy() for y in yv]
    _check(got, U.uncertainty(xr, yr, sigma=got["bandwidth"]), f"{dtype} d={d} ld={ld}")
    if dtype == "float32":                                # the host route of the same rows: the same bits
        host = hip.kad_uncertainty(np.ascontiguousarray(xr), [np.ascontiguousarray(y) for y in yr], rows=True)
        for k in ("mmd2", "kyy_mean", "kxy_mean", "cov", "proj_x"):
            assert np.array_equal(host[k], got[k]), k


def test_kad_uncertainty_is_deterministic_and_agrees_with_kad():
    import torch
    from fadtk_amd import hip
    x, ys = _sets(3000, [2500, 1700, 900], 256, [1, 2, 0], seed=11)
    xd, yd = torch.from_numpy(x).half().cuda(), [torch.from_numpy(y).half().cuda() for y in ys]
    a = hip.kad_uncertainty(xd, yd, rows=True)
    b = hip.kad_uncertainty(xd, yd, rows=True)
    for k in ("mmd2", "kyy_mean", "kxy_mean", "stderr", "cov", "proj_x"):
        assert np.array_equal(a[k], b[k]), k              # bitwise: no float atomics anywhere
    assert all(np.array_equal(p, q) for p, q in zip(a["proj_y"], b["proj_y"]))
    assert a["kxx_mean"] == b["kxx_mean"] and a["bandwidth"] == b["bandwidth"]
    assert np.array_equal(a["cov"], a["cov"].T)
    # the raw per-set results: kxx_mean has the same bits in every set
    from fadtk_amd import _capi as K
    import ctypes as C
    lib = K.load_library()
    S = len(yd)
    ptrs = (C.c_void_p * S)(*[y.data_ptr() for y in yd])
    ms = np.array([y.shape[0] for y in yd], dtype=np.int64)
    lds = np.full(S, 256, dtype=np.int64)
    res = (K.FadKadResult * S)()
    cov = np.zeros((S, S))
    K.check(lib.fad_kad_uncertainty(xd.data_ptr(), xd.shape[0], 256, ptrs, ms.ctypes.data_as(C.POINTER(C.c_int64)),
                                    lds.ctypes.data_as(C.POINTER(C.c_int64)), S, 256, K.FAD_F16, 1, 0.0, res, cov.ctypes.data, None, None,
                                    0, K.current_stream_ptr(0)), "fad_kad_uncertainty")
    assert len({r.kxx_mean.hex() for r in res}) == 1 and res[0].kxx_mean == a["kxx_mean"]
    assert np.array_equal(cov, a["cov"])
    for s in range(S):
        one = hip.kad(xd, yd[s], bandwidth=a["bandwidth"])
        scale = one["kxx_mean"] + one["kyy_mean"] + 2 * one["kxy_mean"]
        assert abs(a["mmd2"][s] - one["mmd2"]) <= MEAN_RTOL * scale, s
    assert hip.kad(xd, yd[0])["bandwidth"] == a["bandwidth"]


def test_kad_uncertainty_errors_on_device():
    from fadtk_amd import _capi, hip
    x = np.random.default_rng(0).standard_normal((50, 16)).astype(np.float16)
    bad = x.copy()
    bad[7, 3] = np.nan
    for args in ((bad, [x]), (x, [x, bad])):
        with pytest.raises(ValueError, match=r"status -7"):                # FAD_ERR_NOT_FINITE
            hip.kad_uncertainty(*args)
    with pytest.raises(AssertionError, match=r"status -6"):                # a one-row set: FAD_ERR_TOO_FEW_ROWS
        hip.kad_uncertainty(x, [x, x[:1]])
    lib = _capi.load_library()
    import ctypes as C
    ptrs = (C.c_void_p * 1)(x[:1].ctypes.data)
    ms = np.array([1], dtype=np.int64)
    lds = np.array([16], dtype=np.int64)
    res = (_capi.FadKadResult * 1)()
    cov = np.zeros(1)
    rc = lib.fad_kad_uncertainty(x.ctypes.data, 50, 16, ptrs, ms.ctypes.data_as(C.POINTER(C.c_int64)), lds.ctypes.data_as(C.POINTER(C.c_int64)),
                                 1, 16, _capi.FAD_F16, 0, 0.0, res, cov.ctypes.data, None, None, 0, None)
    assert rc == _capi.FAD_ERR_TOO_FEW_ROWS
    xn = np.ascontiguousarray(bad)
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    ms = np.array([50], dtype=np.int64)
    rc = lib.fad_kad_uncertainty(xn.ctypes.data, 50, 16, ptrs, ms.ctypes.data_as(C.POINTER(C.c_int64)), lds.ctypes.data_as(C.POINTER(C.c_int64)),
                                 1, 16, _capi.FAD_F16, 0, 0.0, res, cov.ctypes.data, None, None, 0, None)
    assert rc == _capi.FAD_ERR_NOT_FINITE


def test_kad_uncertainty_monte_carlo():
    """100 independent draws at n = m = 1000, D = 64, fixed sigma: Y and Z from one shifted distribution, W shifted a little more."""
    import torch
    from fadtk_amd import calc_kernel_audio_distance_uncertainty
    gen = torch.Generator(device="cuda").manual_seed(7)
    est, se, z_same, z_diff = [], [], [], []
    for _ in range(100):
        x, y, z, w = (torch.randn((1000, 64), generator=gen, device="cuda") for _ in range(4))
        r = calc_kernel_audio_distance_uncertainty(x, [y + 0.25, z + 0.25, w + 0.28], bandwidth=8.0)
        zz, _ = r.compare()
        est.append(r.values[0])
        se.append(r.stderr[0])
        z_same.append(zz[0, 1])
        z_diff.append(zz[0, 2])
    ratio = np.std(est, ddof=1) / np.mean(se)
    same = np.mean(np.abs(z_same) > 1.96)
    diff = np.mean(np.array(z_diff) < -3)
    print(f"[kad-unc] std / mean stderr {ratio:.3f}; |z| > 1.96 for equal shifts {same:.2f}; z < -3 for 0.25 vs 0.28 {diff:.2f}")
    assert 0.8 <= ratio <= 1.2, ratio
    assert same <= 0.12, same
    assert diff >= 0.95, diff


def _row_sums_f64(a, b, sigma, same, chunk=4096):
    """row sums of k(a_i, b_j) over j (j != i when same) and column sums over i, float64 on the GPU chunk by chunk (test plumbing)"""
    import torch
    g = 1.0 / (2.0 * sigma * sigma)
    nb = (b * b).sum(1)
    rows = torch.zeros(a.shape[0], dtype=torch.float64, device=a.device)
    cols = torch.zeros(b.shape[0], dtype=torch.float64, device=a.device)
    for i0 in range(0, a.shape[0], chunk):
        ac = a[i0:i0 + chunk]
        d2 = ((ac * ac).sum(1)[:, None] + nb[None, :] - 2.0 * ac @ b.T).clamp_min_(0)
        k = torch.exp(-g * d2)
        if same:
            idx = torch.arange(ac.shape[0], device=a.device)
            k[idx, idx + i0] = 0.0
        rows[i0:i0 + chunk] = k.sum(1)
        cols += k.sum(0)
        del d2, k
    return rows, cols


def test_kad_uncertainty_config3_size_against_torch_float64():
    import torch
    from fadtk_amd import hip
    gen = torch.Generator(device="cuda").manual_seed(2025)
    n = 100_000
    x = torch.randn((n, 512), generator=gen, device="cuda").half()
    y = (torch.randn((n, 512), generator=gen, device="cuda") * 1.05 + 0.02).half()
    z = (torch.randn((n, 512), generator=gen, device="cuda") * 1.1 + 0.03).half()
    got = hip.kad_uncertainty(x, [y, z], rows=True)
    sigma = got["bandwidth"]
    xd, yd, zd = x.double(), y.double(), z.double()
    rxx, _ = _row_sums_f64(xd, xd, sigma, True)
    a, b, sets = [], [], []
    for e in (yd, zd):
        ree, _ = _row_sums_f64(e, e, sigma, True)
        rxe, rex = _row_sums_f64(xd, e, sigma, False)
        a.append((rxx / (n - 1) - rxe / n).cpu().numpy())
        b.append((ree / (n - 1) - rex / n).cpu().numpy())
        sets.append({"mmd2": float(a[-1].mean() + b[-1].mean()), "kxx_mean": float(rxx.sum()) / (n * (n - 1)),
                     "kyy_mean": float(ree.sum()) / (n * (n - 1)), "kxy_mean": float(rxe.sum()) / (n * n)})
    a = np.stack(a)
    ac = a - a.mean(1, keepdims=True)
    cov = 4.0 / (n * (n - 1)) * (ac @ ac.T)
    for s in range(2):
        cov[s, s] += 4.0 / (n * (n - 1)) * float(((b[s] - b[s].mean()) ** 2).sum())
    _check(got, {"sets": sets, "cov": cov, "proj_x": a, "proj_y": b}, "config-3 100000 x 512 f16, S = 2")


def test_kad_compare_cli_end_to_end(tmp_path):
    from fadtk_amd import FrechetAudioDistance, calc_kernel_audio_distance_uncertainty
    rng = np.random.default_rng(5)
    for name, shift in (("base", 0.0), ("evl", 0.4), ("evl2", 0.6)):
        d = tmp_path / name
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i in range(6):
            (d / f"s{i}.wav").write_bytes(b"")             # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"s{i}.npy", (rng.standard_normal((40 + 7 * i, 128)) + shift).astype(np.float32))
    csv = tmp_path / "out" / "cmp.csv"
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad_compare", "vggish", str(tmp_path / "base"), str(tmp_path / "evl"),
                        str(tmp_path / "evl2"), "--csv", str(csv), "--scale", "10", "-w", "2"], capture_output=True, text=True, cwd=tmp_path,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert " z = " in r.stderr and " p = " in r.stderr
    lines = csv.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,kad,stderr,bandwidth,scale" and len(lines) == 3
    from fadtk_amd.model_loader import get_all_models
    ml = {m.name: m for m in get_all_models()}["vggish"]
    fad = FrechetAudioDistance(ml, load_model=False)
    x = fad.load_embeddings(tmp_path / "base")
    ys = [fad.load_embeddings(tmp_path / e) for e in ("evl", "evl2")]
    res = calc_kernel_audio_distance_uncertainty(x, ys, scale=10.0)
    for line, e, v, se in zip(lines[1:], ("evl", "evl2"), res.values, res.stderr):
        row = line.split(",")
        assert row[2] == str(tmp_path / e) and float(row[3]) == v and float(row[4]) == se
        assert float(row[5]) == res.bandwidth and float(row[6]) == 10.0
    want = U.uncertainty(x, ys)
    assert res.values == pytest.approx(10 * np.array([s["mmd2"] for s in want["sets"]]), rel=1e-4)
    assert res.stderr == pytest.approx(10 * want["stderr"], rel=1e-3)
