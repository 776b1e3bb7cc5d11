"""Kernel Audio Distance on the GPU (fad_kad / fad_kad_median_distance, csrc/kad.hip) against the float64 reference of
tests/kad_reference.py on the same 16-bit values, upcast: accuracy over D, ragged sizes, row pitches and dtypes; the exact median;
bitwise determinism; the config-3 size against torch float64 on the GPU; the command line end to end."""
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("kad_reference", Path(__file__).resolve().parent / "kad_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

# Tolerances: about 4x the largest errors observed on the MI355X (means 9.5e-8 relative, MMD^2 3.4e-8 of
# Kxx + Kyy + 2 Kxy, both at n = 2 / m = 3); each mean relative, MMD^2 against the scale of its terms.
MEAN_RTOL = 4e-7
MMD_TOL = 1.5e-7


def _sets(n, m, d, shift, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * (1.0 + 0.1 * shift) + 0.3 * shift).astype(np.float32)
    return x, y


def _check(got, want, label):
    errs = {k: abs(got[k] - want[k]) / abs(want[k]) for k in ("kxx_mean", "kyy_mean", "kxy_mean") if want[k] != 0}
    scale = want["kxx_mean"] + want["kyy_mean"] + 2 * want["kxy_mean"]
    errs["mmd2/scale"] = abs(got["mmd2"] - want["mmd2"]) / scale
    print(f"[kad-err] {label}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k in ("kxx_mean", "kyy_mean", "kxy_mean"):
        assert got[k] == pytest.approx(want[k], rel=MEAN_RTOL), (label, k, got[k], want[k])
    assert abs(got["mmd2"] - want["mmd2"]) <= MMD_TOL * scale, (label, got["mmd2"], want["mmd2"])
    return errs


CASES = [  # (d, n, m, shift)
    (1, 255, 257, 0), (17, 255, 257, 1), (128, 255, 257, 0), (512, 255, 257, 1), (768, 300, 200, 0), (1024, 255, 257, 1),
    (1280, 130, 129, 0), (128, 2, 3, 1), (128, 1000, 4097, 1), (512, 1000, 4097, 0),
]


@pytest.mark.parametrize("d,n,m,shift", CASES)
def test_kad_float16_matches_float64(d, n, m, shift):
    from fadtk_amd import hip
    x, y = _sets(n, m, d, shift, seed=d + n)
    x16, y16 = x.astype(np.float16), y.astype(np.float16)
    got = hip.kad(x16, y16)
    want = R.kad(x16, y16)
    assert got["bandwidth"] == pytest.approx(want["bandwidth"], rel=1e-5)
    _check(got, R.kad(x16, y16, sigma=got["bandwidth"]), f"f16 d={d} n={n} m={m} shift={shift}")


@pytest.mark.parametrize("dtype", ["bfloat16", "float32", "float16"])
@pytest.mark.parametrize("d,ld", [(17, 24), (128, 136), (512, 520)])
def test_kad_dtypes_and_row_pitch_on_device(dtype, d, ld):
    import torch
    from fadtk_amd import hip
    x, y = _sets(700, 333, d, 1, seed=ld)
    tdt = getattr(torch, dtype)
    xw = torch.zeros((700, ld), dtype=tdt, device="cuda")
    yw = torch.zeros((333, ld), dtype=tdt, device="cuda")
    xw[:, :d] = torch.from_numpy(x).to(tdt)
    yw[:, :d] = torch.from_numpy(y).to(tdt)
    xv, yv = xw[:, :d], yw[:, :d]                         # ld > D, used in place
    got = hip.kad(xv, yv)
    xr, yr = xv.float().cpu().numpy(), yv.float().cpu().numpy()
    _check(got, R.kad(xr, yr, sigma=got["bandwidth"]), f"{dtype} d={d} ld={ld}")
    assert got["bandwidth"] == pytest.approx(R.median_distance(xr), rel=1e-5)
    if dtype == "float32":                                # the host route of the same rows
        host = hip.kad(np.ascontiguousarray(xr), np.ascontiguousarray(yr))
        assert host == got


@pytest.mark.parametrize("n,d,dup", [(2, 8, False), (3, 8, False), (4, 5, False), (5, 64, False), (101, 128, False), (128, 33, True),
                                     (1000, 512, False), (2999, 128, True), (3000, 256, False)])
def test_kad_median_distance_exact(n, d, dup):
    from fadtk_amd import hip
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, d)).astype(np.float16)
    if dup:
        x[n // 2:] = x[: n - n // 2]                      # half the rows repeat: many pairs at distance 0
    want = R.median_distance(x)
    got = hip.kad_median_distance(x)
    print(f"[kad-err] median n={n} d={d} dup={dup}: rel={abs(got - want) / want if want else got:.2e}")
    assert got == pytest.approx(want, rel=1e-5)


def test_kad_errors_on_device():
    import torch
    from fadtk_amd import _capi, hip
    x = np.random.default_rng(0).standard_normal((50, 16)).astype(np.float16)
    bad = x.copy()
    bad[7, 3] = np.inf
    with pytest.raises(ValueError):
        hip.kad(bad, x)
    # every baseline distance is 0: integer-valued rows, so |x|^2 and x.x are exact in float32 whatever their summation order and d^2
    # is exactly 0 (rows that are only equal can leave a rounding residue of either sign in d^2, and a tiny positive median)
    same = np.repeat(np.round(x[:1] * 4), 10, axis=0).astype(np.float16)
    with pytest.raises(RuntimeError, match="must be > 0"):
        hip.kad(same, x)
    with pytest.raises(ValueError):
        hip.kad(x, x, bandwidth=-1.0)
    assert torch.cuda.is_available() and _capi.device_count() >= 1


def test_kad_is_deterministic_and_symmetric():
    import torch
    from fadtk_amd import hip
    x, y = _sets(3000, 2500, 256, 1, seed=11)
    _, z = _sets(10, 1700, 256, 0, seed=12)
    xd, yd, zd = (torch.from_numpy(a).half().cuda() for a in (x, y, z))
    a, b = hip.kad(xd, yd), hip.kad(xd, yd)
    assert a == b                                         # bitwise: no float atomics anywhere
    c = hip.kad(xd, zd)
    assert c["kxx_mean"] == a["kxx_mean"] and c["bandwidth"] == a["bandwidth"]
    s1 = hip.kad(xd, yd, bandwidth=a["bandwidth"])
    s2 = hip.kad(yd, xd, bandwidth=a["bandwidth"])
    assert s1["kxy_mean"] == pytest.approx(s2["kxy_mean"], rel=1e-12)
    assert s1["mmd2"] == pytest.approx(s2["mmd2"], rel=1e-12, abs=1e-15)
    assert s1["kxx_mean"] == s2["kyy_mean"] and s1["kyy_mean"] == s2["kxx_mean"]


def _torch_means_f64(x, y, sigma, chunk=4096):
    """K means and the share of baseline pairs with d^2 < sigma^2, in float64 on the GPU, chunk by chunk (test plumbing)."""
    import torch
    g = 1.0 / (2.0 * sigma * sigma)
    out = {}
    below = 0
    for name, a, b, same in (("kxx_mean", x, x, True), ("kyy_mean", y, y, True), ("kxy_mean", x, y, False)):
        nb = (b * b).sum(1)
        tot = torch.zeros((), dtype=torch.float64, device=a.device)
        for i0 in range(0, a.shape[0], chunk):
            ac = a[i0:i0 + chunk]
            d2 = ((ac * ac).sum(1)[:, None] + nb[None, :] - 2.0 * ac @ b.T).clamp_min_(0)
            if same:
                idx = torch.arange(ac.shape[0], device=a.device)
                d2[idx, idx + i0] = float("inf")          # i == j excluded by index
                if name == "kxx_mean":
                    upper = torch.arange(b.shape[0], device=a.device)[None, :] > (idx + i0)[:, None]
                    below += int(((d2 < sigma * sigma) & upper).sum())
            tot += torch.exp(-g * d2).sum()
            del d2
        n, m = a.shape[0], b.shape[0]
        out[name] = float(tot) / (n * (n - 1) if same else n * m)
    out["mmd2"] = out["kxx_mean"] + out["kyy_mean"] - 2 * out["kxy_mean"]
    n = x.shape[0]
    return out, below / (n * (n - 1) / 2)


def test_kad_config3_size_against_torch_float64():
    import torch
    from fadtk_amd import hip
    gen = torch.Generator(device="cuda").manual_seed(2025)
    x = torch.randn((100_000, 512), generator=gen, device="cuda").half()
    y = (torch.randn((100_000, 512), generator=gen, device="cuda") * 1.05 + 0.02).half()
    got = hip.kad(x, y)
    want, frac = _torch_means_f64(x.double(), y.double(), got["bandwidth"])
    _check(got, want, "config-3 100000 x 512 f16")
    print(f"[kad-err] config-3 share of baseline pairs below the median: {frac:.7f}")
    assert abs(frac - 0.5) <= 1e-4


def test_kad_cli_end_to_end(tmp_path):
    from fadtk_amd import FrechetAudioDistance, calc_kernel_audio_distance
    rng = np.random.default_rng(5)
    for name, shift in (("base", 0.0), ("evl", 0.4)):
        d = tmp_path / name
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i in range(6):
            (d / f"s{i}.wav").write_bytes(b"")             # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"s{i}.npy", (rng.standard_normal((40 + 7 * i, 128)) + shift).astype(np.float32))
    csv = tmp_path / "kad.csv"
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "vggish", str(tmp_path / "base"), str(tmp_path / "evl"), str(csv),
                        "--scale", "10", "-w", "2"], capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = csv.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,kad,bandwidth,scale,time" and len(lines) == 2
    row = lines[1].split(",")
    from fadtk_amd.model_loader import get_all_models
    ml = {m.name: m for m in get_all_models()}["vggish"]
    fad = FrechetAudioDistance(ml, load_model=False)
    x, y = fad.load_embeddings(tmp_path / "base"), fad.load_embeddings(tmp_path / "evl")
    value, res = calc_kernel_audio_distance(x, y, scale=10.0, details=True)
    assert float(row[3]) == value and float(row[4]) == res["bandwidth"] and float(row[5]) == 10.0
    assert value == pytest.approx(10 * R.kad(x, y)["mmd2"], rel=1e-4)
    np.savez(tmp_path / "base.npz", **{"vggish.mu": x.mean(0), "vggish.cov": np.cov(x.T)})
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "vggish", str(tmp_path / "base.npz"), str(tmp_path / "evl")],
                       capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode != 0 and "statistics" in r.stderr
