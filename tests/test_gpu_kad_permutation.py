"""KAD permutation test on the GPU (fad_kad_permutation_test, csrc/kad.hip) against the float64 reference of
tests/kad_permutation_reference.py on the same 16-bit values, upcast: every null statistic and t_0 within tau = 1e-2 of the reference
null's spread, over dtypes, D, ragged sizes around tile and word edges, labelling counts and row pitches; the pooled-median bandwidth;
bitwise determinism and seeded labellings; calibration and power; errors; the config-3 size against torch float64 on the GPU."""
import importlib.util
import time
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PR = _load("kad_permutation_reference")
TAU = 1e-2           # of the reference null's standard deviation


def _sets(n, m, d, dtype, seed, shift=0.1):
    import torch
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * 1.05 + shift).astype(np.float32)
    if dtype == "bf16":
        xt, yt = torch.from_numpy(x).cuda().bfloat16(), torch.from_numpy(y).cuda().bfloat16()
        return xt, yt, xt.double().cpu().numpy(), yt.double().cpu().numpy()
    x, y = x.astype(np.float16 if dtype == "f16" else np.float32), y.astype(np.float16 if dtype == "f16" else np.float32)
    return x, y, x.astype(np.float64), y.astype(np.float64)


def _check(x, y, xr, yr, P, seed, label, bandwidth=None):
    from fadtk_amd import hip
    n, m = xr.shape[0], yr.shape[0]
    rng = np.random.default_rng(seed)
    u = PR.random_labellings(n, m, P, rng)
    got = hip.kad_permutation_test(x, y, hip.pack_labels(u), bandwidth=bandwidth)
    sigma = got["bandwidth"]
    if bandwidth is None:                                                       # the pooled median, bit for bit
        if isinstance(x, np.ndarray):
            assert sigma == hip.kad_median_distance(np.concatenate([x, y]))
        else:
            import torch
            assert sigma == hip.kad_median_distance(torch.cat([x, y]))
    t = PR.statistics(xr, yr, np.concatenate([PR.observed_labelling(n, m), u]), sigma)
    t0, null = t[0], t[1:]
    spread = null if P >= 50 else PR.statistics(xr, yr, PR.random_labellings(n, m, 200, rng), sigma)
    tau = TAU * float(np.std(spread))
    err = max(abs(got["mmd2"] - t0), float(np.max(np.abs(got["null"] - null))))
    print(f"[kad-perm-err] {label}: max |dt| / sd = {err / (tau / TAU):.2e}")
    assert abs(got["mmd2"] - t0) <= tau, (label, got["mmd2"], t0, tau)
    assert np.max(np.abs(got["null"] - null)) <= tau, (label, np.max(np.abs(got["null"] - null)), tau)
    kad = hip.kad(x, y, bandwidth=sigma)
    assert abs(got["mmd2"] - kad["mmd2"]) <= tau, (label, got["mmd2"], kad["mmd2"])
    if not np.any(np.abs(null - t0) <= 4 * tau):
        assert got["p_value"] == PR.p_value(t0, null), (label, got["p_value"], PR.p_value(t0, null))
    return got


CASES = [  # (dtype, d, n, m, P)
    ("f16", 128, 2, 2, 1), ("f16", 17, 2, 700, 33), ("f16", 3, 127, 129, 128), ("f16", 512, 128, 160, 129),
    ("f16", 1024, 96, 97, 1000), ("f16", 2048, 64, 33, 31), ("f16", 130, 255, 257, 127), ("f16", 1, 300, 200, 32),
    ("bf16", 128, 127, 129, 129), ("bf16", 512, 33, 64, 1000), ("f32", 128, 127, 129, 129), ("f32", 17, 31, 97, 1000),
    ("f32", 1024, 64, 64, 33),
]


@pytest.mark.parametrize("dtype,d,n,m,P", CASES)
def test_kad_permutation_matches_float64_reference(dtype, d, n, m, P):
    x, y, xr, yr = _sets(n, m, d, dtype, seed=d + n + m + P)
    _check(x, y, xr, yr, P, seed=P, label=f"{dtype} D={d} n={n} m={m} P={P}")


def test_kad_permutation_row_pitch_on_device_and_given_bandwidth():
    import torch
    rng = np.random.default_rng(4)
    xw = rng.standard_normal((150, 200)).astype(np.float16)
    yw = (rng.standard_normal((90, 200)) + 0.2).astype(np.float16)
    x, y = torch.from_numpy(xw).cuda()[:, :130], torch.from_numpy(yw).cuda()[:, :130]          # ld = 200 > D = 130
    _check(x, y, xw[:, :130].astype(np.float64), yw[:, :130].astype(np.float64), 129, seed=1, label="ld > D, device rows")
    _check(x, y, xw[:, :130].astype(np.float64), yw[:, :130].astype(np.float64), 64, seed=2, label="given sigma", bandwidth=11.0)


def test_kad_permutation_is_deterministic_and_seeded():
    import torch
    from fadtk_amd import calc_kernel_audio_distance_permutation_test as perm
    x, y, _, _ = _sets(300, 211, 64, "f16", seed=9)
    a = perm(x, y, permutations=1000, seed=7, return_labels=True)
    b = perm(x, y, permutations=1000, seed=7, return_labels=True)
    assert torch.equal(a["labels"], b["labels"])
    assert a["null"].tobytes() == b["null"].tobytes() and a["mmd2"] == b["mmd2"] and a["p_value"] == b["p_value"]
    u = PR.unpack(a["labels"].cpu().numpy(), 511)
    assert u.shape == (1000, 511) and np.all(u.sum(1) == 300)
    c = perm(x, y, permutations=1000, seed=8, return_labels=True)
    assert not torch.equal(a["labels"], c["labels"]) and c["mmd2"] == a["mmd2"]
    d = perm(x, y, labels=a["labels"].cpu().numpy().view(np.uint32))                          # host words give the same bits
    assert d["null"].tobytes() == a["null"].tobytes() and d["seed"] is None
    e = perm(x, y, labels=torch.from_numpy(u).cuda())                                         # 0/1 on the device
    assert e["null"].tobytes() == a["null"].tobytes()


def test_kad_permutation_calibration_and_power():
    from fadtk_amd import calc_kernel_audio_distance_permutation_test as perm
    rng = np.random.default_rng(11)
    ps = []
    for s in range(100):
        x = rng.standard_normal((150, 16)).astype(np.float32)
        y = rng.standard_normal((150, 16)).astype(np.float32)
        ps.append(perm(x, y, permutations=199, seed=s)["p_value"])
    frac = float(np.mean(np.array(ps) <= 0.05))
    print(f"[kad-perm] fraction of p <= 0.05 over 100 null draws: {frac:.2f}")
    assert 0.01 <= frac <= 0.11, frac
    for s in range(10):
        x = rng.standard_normal((150, 16)).astype(np.float32)
        y = (rng.standard_normal((150, 16)) + 0.5).astype(np.float32)
        assert perm(x, y, permutations=199, seed=s)["p_value"] == 1.0 / 200


def test_kad_permutation_errors_on_device():
    import torch
    from fadtk_amd import calc_kernel_audio_distance_permutation_test as perm, hip
    x, y, _, _ = _sets(40, 30, 8, "f32", seed=3)
    bad = x.copy()
    bad[5, 2] = np.nan
    with pytest.raises(ValueError, match=r"status -7"):                         # FAD_ERR_NOT_FINITE
        perm(bad, y, permutations=10)
    u = PR.random_labellings(40, 30, 6, np.random.default_rng(0))
    for delta in (+1, -1):
        v = u.copy()
        row = v[3]
        idx = np.flatnonzero(~row if delta > 0 else row)[0]
        row[idx] = delta > 0
        words = torch.from_numpy(hip.pack_labels(v).view(np.int32)).cuda()
        with pytest.raises(RuntimeError, match=r"status -1"):                   # FAD_ERR_INVALID, from the device check
            hip.kad_permutation_test(x, y, words)
    with pytest.raises(ValueError):
        perm(x, y, permutations=0)
    ok = hip.kad_permutation_test(x, y, torch.from_numpy(hip.pack_labels(u).view(np.int32)).cuda())          # the call after errors
    assert np.all(np.isfinite(ok["null"]))


def test_kad_permutation_config3_size_against_torch_float64():
    import torch
    from fadtk_amd import calc_kernel_audio_distance_permutation_test as perm, hip
    gen = torch.Generator(device="cuda").manual_seed(2026)
    n = 100_000
    x = torch.randn((n, 512), generator=gen, device="cuda").half()
    y = (torch.randn((n, 512), generator=gen, device="cuda") * 1.05 + 0.02).half()
    t = time.perf_counter()
    got = perm(x, y, permutations=200, seed=1, return_labels=True)
    print(f"[kad-perm] config-3 P = 200: {time.perf_counter() - t:.3f} s (first call)")
    sigma = got["bandwidth"]
    z = torch.cat([x, y]).double()
    N = 2 * n
    g = 1.0 / (2.0 * sigma * sigma)
    nz = (z * z).sum(1)
    lab = got["labels"][:5].cpu().numpy().view(np.uint32)
    U = torch.from_numpy(PR.unpack(lab, N).astype(np.float64)).cuda()            # observed is not among them: add it
    U = torch.cat([torch.zeros((1, N), dtype=torch.float64, device="cuda").index_fill_(1, torch.arange(n, device="cuda"), 1.0), U])
    r = torch.zeros(N, dtype=torch.float64, device="cuda")
    KU = torch.zeros((N, U.shape[0]), dtype=torch.float64, device="cuda")
    for i0 in range(0, N, 8192):
        zc = z[i0:i0 + 8192]
        k = torch.exp(-g * ((zc * zc).sum(1)[:, None] + nz[None, :] - 2.0 * zc @ z.T).clamp_min_(0))
        idx = torch.arange(zc.shape[0], device="cuda")
        k[idx, idx + i0] = 0.0
        r[i0:i0 + 8192] = k.sum(1)
        KU[i0:i0 + 8192] = k @ U.T
        del k
    q = (U * KU.T).sum(1)
    R = U @ r
    T = r.sum()
    tt = (q / (n * (n - 1.0)) + (T - 2 * R + q) / (n * (n - 1.0)) - 2 * (R - q) / (n * float(n))).cpu().numpy()
    sd = float(np.std(got["null"]))                                              # the null's spread (the reference's to < 1 %)
    tau = TAU * sd
    kad = hip.kad(x, y, bandwidth=sigma)
    print(f"[kad-perm-err] config-3: |t0 - ref| / sd = {abs(got['mmd2'] - tt[0]) / sd:.2e}, "
          f"max |null[0:5] - ref| / sd = {np.max(np.abs(got['null'][:5] - tt[1:])) / sd:.2e}")
    assert abs(got["mmd2"] - tt[0]) <= tau and abs(got["mmd2"] - kad["mmd2"]) <= tau
    assert np.max(np.abs(got["null"][:5] - tt[1:])) <= tau
