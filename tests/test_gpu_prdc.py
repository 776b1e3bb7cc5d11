"""Precision, recall, density and coverage on the GPU (fad_prdc, csrc/kad.hip) against the float64 reference of tests/prdc_reference.py
on the same 16-bit values, upcast: exact on integer rows (ties, duplicates, strict comparisons, self excluded by index), inside the
reference's bracket on Gaussian rows, errors, determinism, numpy against torch, the config-3 size against torch float64 on the GPU, and
the command line end to end."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("prdc_reference", Path(__file__).resolve().parent / "prdc_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

# Margin of one float32 d^2 against float64, relative to |a|^2 + |b|^2: about 4x the largest radius error observed on the MI355X
# (3.2e-6 for float32 rows at D = 1024, 1.45e-6 for 16-bit rows).
TAU = 1.3e-5
TIGHT = 0.005          # widest bracket allowed on each of the four values (counts over their own m, n or k m)
METRICS = ("precision", "recall", "density", "coverage")


def _cast(a, dt):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"fp16": t.half(), "bf16": t.bfloat16(), "fp32": t}[dt]


def _host(t):
    return t.float().numpy().astype(np.float64)


def _int_rows(rng, n, d, dups):
    a = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    for i, j in dups:
        if i < n and j < n:
            a[j] = a[i]
    return a


EXACT = [  # n, m, d, k
    (2, 2, 3, 1), (6, 6, 17, 5), (17, 17, 1, 16), (127, 128, 17, 5), (129, 300, 128, 1), (300, 129, 130, 16), (1000, 127, 1, 5),
    (128, 1000, 3, 16), (1000, 1000, 128, 5), (300, 1000, 130, 1), (17, 129, 3, 16),
]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,m,d,k", EXACT)
def test_prdc_exact_on_integer_rows(n, m, d, k, dt):
    from fadtk_amd import hip
    rng = np.random.default_rng(n * 7 + m * 3 + d + k)
    x = _int_rows(rng, n, d, [(0, 1), (3, n - 1), (2, n // 2)])
    y = _int_rows(rng, m, d, [(1, 0), (4, m - 2)])
    if m > 5 and n > 5:
        y[5] = x[4]                                                # a y row on top of an x row
    xt, yt = _cast(x, dt), _cast(y, dt)
    got = hip.prdc(xt.numpy() if dt != "bf16" else xt.cuda(), yt.numpy() if dt != "bf16" else yt.cuda(), k=k, details=True)
    want = R.prdc(_host(xt), _host(yt), k)
    np.testing.assert_array_equal(got["radius2_x"].astype(np.float64), want["radius2_x"])
    np.testing.assert_array_equal(got["radius2_y"].astype(np.float64), want["radius2_y"])
    np.testing.assert_array_equal(got["balls_y"], want["balls_y"])
    np.testing.assert_array_equal(got["flags_x"], want["flags_x"])
    for key in METRICS:
        assert got[key] == want[key], (key, got[key], want[key])
    assert (got["n"], got["m"], got["k"]) == (n, m, k)


def _gauss(n, m, d, seed):
    """x standard normal; y scaled and shifted by amounts that shrink with D, so the two sets overlap about as much at every D (at a
    fixed scale, large D puts y on a shell apart from x's and every count is 0)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * (1.0 + 0.1 * (128 / d) ** 0.5) + 0.05 * (128 / d) ** 0.25).astype(np.float32)
    return x, y


def _check_bracket(got, x, y, k, label):
    """GPU radii within TAU of float64, every count and flag inside the reference's bracket, the bracket tight -> observed radius error."""
    br = R.bracket(x, y, k, TAU)
    sx, sy = (x ** 2).sum(1), (y ** 2).sum(1)
    errs = []
    for a, key, sq in ((x, "x", sx), (y, "y", sy)):
        r2, nn = R.radii2(a, k)
        err = np.abs(got[f"radius2_{key}"].astype(np.float64) - r2) / (sq + sq[nn])
        errs.append(float(err.max()))
        assert err.max() <= TAU, (label, key, float(err.max()))
    balls, flags = got["balls_y"], got["flags_x"]
    assert (br["balls_lo"] <= balls).all() and (balls <= br["balls_hi"]).all(), label
    rec, cov = (flags & 1).astype(bool), (flags & 2).astype(bool)
    assert (br["recalled_lo"] <= rec).all() and (rec <= br["recalled_hi"]).all(), label
    assert (br["covered_lo"] <= cov).all() and (cov <= br["covered_hi"]).all(), label
    for key in METRICS:                              # inside the bracket, and the bracket of every value narrower than TIGHT
        assert br[f"{key}_lo"] <= got[key] <= br[f"{key}_hi"], (label, key)
        assert br[f"{key}_hi"] - br[f"{key}_lo"] <= TIGHT, (label, key, br[f"{key}_lo"], br[f"{key}_hi"])
    print(f"[prdc-err] {label}: radius2 x {errs[0]:.2e} y {errs[1]:.2e}; "
          + " ".join(f"{key}={got[key]:.4f}" for key in METRICS))
    return max(errs)


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,m,d,k", [(1100, 900, 128, 5), (777, 1301, 512, 3), (1500, 500, 768, 16), (641, 1029, 1024, 1)])
def test_prdc_gaussian_rows_inside_the_bracket(n, m, d, k, dt):
    import torch
    from fadtk_amd import hip
    x, y = _gauss(n, m, d, seed=n + d)
    xt, yt = _cast(x, dt), _cast(y, dt)
    wide_x = torch.zeros((n, d + 24), dtype=xt.dtype, device="cuda")
    wide_y = torch.zeros((m, d + 8), dtype=xt.dtype, device="cuda")
    wide_x[:, :d] = xt.cuda()
    wide_y[:, :d] = yt.cuda()
    got = hip.prdc(wide_x[:, :d], wide_y[:, :d], k=k, details=True)          # ld > D on the device
    _check_bracket(got, _host(xt), _host(yt), k, f"{dt} n={n} m={m} D={d} k={k}")


def _raw_call(x, y, k):
    from fadtk_amd import _capi
    lib = _capi.load_library()
    res = _capi.FadPrdcResult()
    return lib.fad_prdc(x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, y.shape[0], y.shape[1], x.shape[1], _capi.FAD_F32, 0, k,
                        C.byref(res), None, 0, None), res


def test_prdc_errors():
    from fadtk_amd import _capi
    x, y = _gauss(300, 200, 64, seed=1)
    st, _ = _raw_call(x, y, 5)
    assert st == _capi.FAD_OK
    bad = x.copy()
    bad[123, 7] = np.nan
    assert _raw_call(bad, y, 5)[0] == _capi.FAD_ERR_NOT_FINITE
    bad = y.copy()
    bad[0, 0] = np.inf
    assert _raw_call(x, bad, 5)[0] == _capi.FAD_ERR_NOT_FINITE
    assert _raw_call(x[:5], y, 5)[0] == _capi.FAD_ERR_TOO_FEW_ROWS
    assert _raw_call(x, y[:16], 16)[0] == _capi.FAD_ERR_TOO_FEW_ROWS
    assert _raw_call(x, y, 17)[0] == _capi.FAD_ERR_INVALID
    assert _raw_call(x, y, 5)[0] == _capi.FAD_OK                  # the library is usable after the errors


def test_prdc_deterministic_and_numpy_equals_torch():
    import torch
    from fadtk_amd import hip
    x, y = _gauss(3000, 2500, 256, seed=4)
    x16, y16 = x.astype(np.float16), y.astype(np.float16)
    a = hip.prdc(x16, y16, k=5, details=True)
    b = hip.prdc(x16, y16, k=5, details=True)
    c = hip.prdc(torch.from_numpy(x16).cuda(), torch.from_numpy(y16).cuda(), k=5, details=True)
    for other in (b, c):
        for key in ("radius2_x", "radius2_y", "balls_y", "flags_x"):
            assert a[key].tobytes() == other[key].tobytes(), key
        for key in METRICS:
            assert a[key] == other[key], key


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_prdc_of_a_set_against_itself(dt):
    from fadtk_amd import calc_precision_recall_density_coverage as prdc
    x, _ = _gauss(2000, 2, 128, seed=9)
    xt = _cast(x, dt).numpy()
    got = prdc(xt, xt.copy(), k=5, details=True)
    assert got["precision"] == 1.0 and got["recall"] == 1.0 and got["coverage"] == 1.0, got
    assert got["covered_x"].all() and got["recalled_x"].all() and (got["balls_y"] >= 1).all()
    assert np.array_equal(got["radius_x"], got["radius_y"])


def test_prdc_config3_size_against_torch_float64():
    import torch
    from fadtk_amd import hip
    n = m = 100_000
    d, k = 512, 5
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((n, d), device="cuda", generator=g).half()
    y = (torch.randn((m, d), device="cuda", generator=g) * 1.05 + 0.03).half()
    got = hip.prdc(x, y, k=k, details=True)

    xd, yd = x.double(), y.double()
    sx, sy = (xd * xd).sum(1), (yd * yd).sum(1)

    def radii(a, sa):
        r2 = torch.empty(a.shape[0], dtype=torch.float64, device="cuda")
        nn = torch.empty(a.shape[0], dtype=torch.int64, device="cuda")
        for s in range(0, a.shape[0], 4096):
            e = min(s + 4096, a.shape[0])
            d2 = sa[s:e, None] + sa[None, :] - 2.0 * (a[s:e] @ a.T)
            d2[torch.arange(e - s, device="cuda"), torch.arange(s, e, device="cuda")] = float("inf")
            v, i = torch.kthvalue(d2, k, dim=1)
            r2[s:e], nn[s:e] = v, i
        return r2, nn
    r2x, nnx = radii(xd, sx)
    r2y, nny = radii(yd, sy)
    ex, ey = TAU * (sx + sx[nnx]), TAU * (sy + sy[nny])
    for r2, e, sq, nn, key in ((r2x, ex, sx, nnx, "x"), (r2y, ey, sy, nny, "y")):
        err = ((torch.from_numpy(got[f"radius2_{key}"]).cuda().double() - r2).abs() / (sq + sq[nn])).max().item()
        print(f"[prdc-err] config 3 radius2 {key}: {err:.2e}")
        assert err <= TAU, (key, err)

    balls_lo = torch.zeros(m, dtype=torch.int64, device="cuda")
    balls_hi = torch.zeros_like(balls_lo)
    flags_lo, flags_hi = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    for s in range(0, n, 4096):
        e = min(s + 4096, n)
        d2 = sx[s:e, None] + sy[None, :] - 2.0 * (xd[s:e] @ yd.T)
        pair = TAU * (sx[s:e, None] + sy[None, :])
        g1, m1 = d2 - r2x[s:e, None], pair + ex[s:e, None]
        g2, m2 = d2 - r2y[None, :], pair + ey[None, :]
        balls_lo += (g1 < -m1).sum(0)
        balls_hi += (g1 < m1).sum(0)
        flags_lo[s:e] = (g2 < -m2).any(1).long() | ((g1 < -m1).any(1).long() << 1)
        flags_hi[s:e] = (g2 < m2).any(1).long() | ((g1 < m1).any(1).long() << 1)
    balls = torch.from_numpy(got["balls_y"]).cuda().long()
    flags = torch.from_numpy(got["flags_x"]).cuda().long()
    assert bool(((balls_lo <= balls) & (balls <= balls_hi)).all())
    for bit in (1, 2):
        lo, hi, f = (flags_lo & bit) > 0, (flags_hi & bit) > 0, (flags & bit) > 0
        assert bool((lo <= f).all() & (f <= hi).all()), bit
        assert (hi.sum() - lo.sum()).item() <= TIGHT * n, bit
    assert (balls_hi - balls_lo).sum().item() <= TIGHT * k * m
    assert ((balls_hi > 0).sum() - (balls_lo > 0).sum()).item() <= TIGHT * m
    print(f"[prdc-err] config 3: " + " ".join(f"{key}={got[key]:.5f}" for key in METRICS))


def test_prdc_cli_end_to_end(tmp_path):
    from fadtk_amd import FrechetAudioDistance, calc_precision_recall_density_coverage
    rng = np.random.default_rng(6)
    for name, shift in (("base", 0.0), ("evl", 0.4)):
        d = tmp_path / name
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i in range(6):
            (d / f"s{i}.wav").write_bytes(b"")             # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"s{i}.npy", (rng.standard_normal((40 + 7 * i, 128)) + shift).astype(np.float32))
    csv = tmp_path / "prdc.csv"
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.prdc", "vggish", str(tmp_path / "base"), str(tmp_path / "evl"), str(csv),
                        "-k", "3", "-w", "2"], capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = csv.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,k,precision,recall,density,coverage,time" and len(lines) == 2
    row = lines[1].split(",")
    from fadtk_amd.model_loader import get_all_models
    ml = {m.name: m for m in get_all_models()}["vggish"]
    fad = FrechetAudioDistance(ml, load_model=False)
    x, y = fad.load_embeddings(tmp_path / "base"), fad.load_embeddings(tmp_path / "evl")
    res = calc_precision_recall_density_coverage(x, y, k=3)
    assert row[0] == "vggish" and int(row[3]) == 3
    assert [float(v) for v in row[4:8]] == [res[key] for key in METRICS]
    br = R.bracket(x.astype(np.float64), y.astype(np.float64), 3, TAU)
    for key in METRICS:
        assert br[f"{key}_lo"] <= res[key] <= br[f"{key}_hi"], key
    np.savez(tmp_path / "base.npz", **{"vggish.mu": x.mean(0), "vggish.cov": np.cov(x.T)})
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.prdc", "vggish", str(tmp_path / "base.npz"), str(tmp_path / "evl")],
                       capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode != 0 and "statistics" in r.stderr
