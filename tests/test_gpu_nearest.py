"""Nearest baseline rows and authenticity on the GPU (fad_nearest, csrc/kad.hip) against the float64 reference of
tests/nearest_reference.py on the same 16-bit values, upcast: exact on integer rows (ties by index, duplicates, exact copies), valid
k-NN lists inside the reference's bracket on Gaussian rows, errors, determinism, numpy against torch, the config-3 size against torch
float64 on the GPU, and the per-song copy detection end to end through score_individual and the command line."""
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
_spec = importlib.util.spec_from_file_location("nearest_reference", Path(__file__).resolve().parent / "nearest_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

# Margin of one float32 d^2 against float64, relative to |x_i|^2 + |y_j|^2: about 4x the largest error observed on the MI355X
# (DESIGN.md 4.11).
TAU = 1.3e-5


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
    (2, 1, 3, 1), (5, 7, 17, 5), (16, 16, 1, 16), (127, 128, 17, 5), (129, 300, 128, 1), (300, 129, 130, 16), (1000, 127, 1, 5),
    (128, 1000, 3, 16), (1000, 1000, 128, 5), (300, 1000, 130, 1), (17, 129, 3, 16), (1000, 1001, 17, 4),
]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,m,d,k", EXACT)
def test_nearest_exact_on_integer_rows(n, m, d, k, dt):
    from fadtk_amd import hip
    rng = np.random.default_rng(n * 5 + m * 3 + d + k)
    x = _int_rows(rng, n, d, [(0, 1), (3, n - 1), (2, n // 2)])
    y = _int_rows(rng, m, d, [(1, 0)])
    for j, i in ((0, 1), (2, n - 1), (m - 1, n // 2), (m // 2, 0)):        # y rows on top of x rows, duplicated ones among them
        if j < m:
            y[j] = x[i]
    xt, yt = _cast(x, dt), _cast(y, dt)
    got = hip.nearest(xt.numpy() if dt != "bf16" else xt.cuda(), yt.numpy() if dt != "bf16" else yt.cuda(), k=k, authenticity=True)
    idx, d2 = R.nearest(_host(xt), _host(yt), k)
    np.testing.assert_array_equal(got["index"], idx)
    np.testing.assert_array_equal(got["dist2"].astype(np.float64), d2)
    want = R.authenticity(_host(xt), _host(yt))
    np.testing.assert_array_equal(got["nn_radius2"].astype(np.float64), want["nn_radius2"])
    assert got["copied"] == want["copied"] and got["authenticity"] == want["authenticity"]
    assert want["copied_rows"][0]                                          # an exact copy of a duplicated row: d^2 = 0 = r1^2
    assert (got["n"], got["m"], got["k"]) == (n, m, k)


def _gauss(n, m, d, seed):
    """x standard normal; y a mix of near copies of x rows and fresh rows, so that both copied decisions occur at every D."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * 1.05 + 0.03).astype(np.float32)
    near = rng.choice(n, size=m // 3, replace=False) if m // 3 <= n else rng.integers(0, n, m // 3)
    y[: m // 3] = x[near] + 0.5 * rng.standard_normal((m // 3, d)).astype(np.float32)
    return x, y


def _check_bracket(got, x, y, k, label):
    """dist2 within TAU of float64, every list a valid k-NN inside the bracket, copied inside its bracket -> worst relative d^2 error."""
    br = R.bracket(x, y, k, TAU)
    sx, sy = (x ** 2).sum(1), (y ** 2).sum(1)
    idx = got["index"].astype(np.int64)
    err = np.abs(got["dist2"].astype(np.float64) - np.take_along_axis(br["d2"], idx, 1)) / (sy[:, None] + sx[idx])
    assert err.max() <= TAU, (label, float(err.max()))
    ok = R.valid_knn(idx, got["dist2"], br, k)
    assert ok.all(), (label, np.flatnonzero(~ok)[:10])
    assert br["copied_lo"] <= got["copied"] <= br["copied_hi"], (label, br["copied_lo"], got["copied"], br["copied_hi"])
    r1_err = np.abs(got["nn_radius2"].astype(np.float64) - br["r1"][idx[:, 0]]) <= br["r1_margin"][idx[:, 0]]
    assert r1_err.all(), label
    print(f"[nearest-err] {label}: d2 {err.max():.2e}; copied {got['copied']} in [{br['copied_lo']}, {br['copied_hi']}]")
    return float(err.max())


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,m,d,k", [(1100, 900, 128, 5), (777, 1301, 512, 3), (1500, 500, 768, 16), (641, 1029, 1024, 1)])
def test_nearest_gaussian_rows_inside_the_bracket(n, m, d, k, dt):
    import torch
    from fadtk_amd import hip
    x, y = _gauss(n, m, d, seed=n + d)
    xt, yt = _cast(x, dt), _cast(y, dt)
    wide_x = torch.zeros((n, d + 24), dtype=xt.dtype, device="cuda")
    wide_y = torch.zeros((m, d + 8), dtype=xt.dtype, device="cuda")
    wide_x[:, :d] = xt.cuda()
    wide_y[:, :d] = yt.cuda()
    got = hip.nearest(wide_x[:, :d], wide_y[:, :d], k=k, authenticity=True)          # ld > D on the device
    _check_bracket(got, _host(xt), _host(yt), k, f"{dt} n={n} m={m} D={d} k={k}")


def _raw_call(x, y, k, auth=1):
    from fadtk_amd import _capi
    lib = _capi.load_library()
    res = _capi.FadNearestResult()
    idx = np.zeros(y.shape[0] * k, np.int32)
    d2 = np.zeros(y.shape[0] * k, np.float32)
    return lib.fad_nearest(x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, y.shape[0], y.shape[1], x.shape[1], _capi.FAD_F32, 0,
                           k, auth, idx.ctypes.data, d2.ctypes.data, None, C.byref(res), 0, None), res


def test_nearest_errors():
    from fadtk_amd import _capi
    x, y = _gauss(300, 200, 64, seed=1)
    st, res = _raw_call(x, y, 5)
    assert st == _capi.FAD_OK and res.copied >= 0
    bad = x.copy()
    bad[123, 7] = np.nan
    assert _raw_call(bad, y, 5)[0] == _capi.FAD_ERR_NOT_FINITE
    bad = y.copy()
    bad[0, 0] = np.inf
    assert _raw_call(x, bad, 5)[0] == _capi.FAD_ERR_NOT_FINITE
    assert _raw_call(x[:4], y, 5)[0] == _capi.FAD_ERR_TOO_FEW_ROWS
    assert _raw_call(x, y, 17)[0] == _capi.FAD_ERR_INVALID
    st, res = _raw_call(x, y, 5, auth=0)
    assert st == _capi.FAD_OK and res.copied == -1 and np.isnan(res.authenticity)
    st, res = _raw_call(x[:1], y, 1, auth=0)                              # one baseline row: every row's nearest is row 0
    assert st == _capi.FAD_OK


def test_nearest_deterministic_numpy_equals_torch_and_authenticity_off():
    import torch
    from fadtk_amd import hip
    x, y = _gauss(3000, 2500, 256, seed=4)
    x16, y16 = x.astype(np.float16), y.astype(np.float16)
    a = hip.nearest(x16, y16, k=5)
    b = hip.nearest(x16, y16, k=5)
    c = hip.nearest(torch.from_numpy(x16).cuda(), torch.from_numpy(y16).cuda(), k=5)
    off = hip.nearest(x16, y16, k=5, authenticity=False)
    for other in (b, c, off):
        for key in ("index", "dist2"):
            assert a[key].tobytes() == other[key].tobytes(), key
    for other in (b, c):
        assert a["nn_radius2"].tobytes() == other["nn_radius2"].tobytes()
        assert a["copied"] == other["copied"] and a["authenticity"] == other["authenticity"]
    assert off["nn_radius2"] is None and off["copied"] == -1 and np.isnan(off["authenticity"])
    one = hip.nearest(x16, y16, k=1)                                       # the first of every k-list is the 1-NN
    assert one["index"][:, 0].tobytes() == a["index"][:, 0].tobytes()
    assert one["dist2"][:, 0].tobytes() == a["dist2"][:, 0].tobytes()


def test_nearest_of_a_set_against_itself():
    from fadtk_amd import calc_authenticity, calc_nearest_neighbours
    x, _ = _gauss(2000, 3, 128, seed=9)
    x16 = x.astype(np.float16)
    dist, idx = calc_nearest_neighbours(x16, x16.copy(), k=2)
    assert (idx[:, 0] == np.arange(2000)).all() and (idx[:, 1] != idx[:, 0]).all()
    res = calc_authenticity(x16, x16.copy(), details=True)
    assert res["copied"] == 2000 and res["authenticity"] == 0.0 and res["copied_rows"].all()


def test_nearest_config3_size_against_torch_float64():
    import torch
    from fadtk_amd import hip
    n = m = 100_000
    d = 512
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((n, d), device="cuda", generator=g).half()
    y = (torch.randn((m, d), device="cuda", generator=g) * 1.05 + 0.03).half()
    y[:1000] = x[5000:6000]                                                  # exact copies
    got = hip.nearest(x, y, k=1, authenticity=True)

    xd, yd = x.double(), y.double()
    sx, sy = (xd * xd).sum(1), (yd * yd).sum(1)
    r1 = torch.empty(n, dtype=torch.float64, device="cuda")
    nn1 = torch.empty(n, dtype=torch.int64, device="cuda")
    for s in range(0, n, 4096):
        e = min(s + 4096, n)
        d2 = sx[s:e, None] + sx[None, :] - 2.0 * (xd[s:e] @ xd.T)
        d2[torch.arange(e - s, device="cuda"), torch.arange(s, e, device="cuda")] = float("inf")
        r1[s:e], nn1[s:e] = d2.min(1)
    r1_marg = TAU * (sx + sx[nn1])
    idx = torch.from_numpy(got["index"][:, 0].astype(np.int64)).cuda()
    dist2 = torch.from_numpy(got["dist2"][:, 0]).cuda().double()
    nn_r2 = torch.from_numpy(got["nn_radius2"]).cuda().double()
    worst, lo, hi = 0.0, 0, 0
    for s in range(0, m, 4096):
        e = min(s + 4096, m)
        d2 = sy[s:e, None] + sx[None, :] - 2.0 * (yd[s:e] @ xd.T)
        marg = TAU * (sy[s:e, None] + sx[None, :])
        rows = torch.arange(e - s, device="cuda")
        mine = d2[rows, idx[s:e]]
        err = ((dist2[s:e] - mine).abs() / (sy[s:e] + sx[idx[s:e]])).max().item()
        worst = max(worst, err)
        assert err <= TAU, err
        assert bool(((mine - marg[rows, idx[s:e]]) <= (d2 + marg).min(1).values).all())       # a valid nearest row
        assert bool(((nn_r2[s:e] - r1[idx[s:e]]).abs() <= r1_marg[idx[s:e]]).all())
        g_ = mine - marg[rows, idx[s:e]] - (r1[idx[s:e]] + r1_marg[idx[s:e]])
        h_ = mine + marg[rows, idx[s:e]] - (r1[idx[s:e]] - r1_marg[idx[s:e]])
        lo += int((h_ <= 0).sum().item())
        hi += int((g_ <= 0).sum().item())
    assert lo <= got["copied"] <= hi, (lo, got["copied"], hi)
    assert got["copied"] >= 1000 and (got["index"][:1000, 0] == np.arange(5000, 6000)).all()
    print(f"[nearest-err] config 3: d2 {worst:.2e}; copied {got['copied']} in [{lo}, {hi}], authenticity {got['authenticity']:.5f}")


def _songs(tmp_path):
    """A baseline of songs whose frames cluster around a song centre (as real embeddings do), and an eval set of: an exact copy of
    base s0, a noisy copy of base s1, an excerpt of base s2, and three fresh songs."""
    rng = np.random.default_rng(12)
    base = tmp_path / "base"
    evl = tmp_path / "evl"
    emb = {}
    for name, d in (("base", base), ("evl", evl)):
        (d / "embeddings" / "vggish").mkdir(parents=True)
    for i in range(8):
        c = rng.standard_normal(128)
        emb[f"s{i}"] = (c + 0.3 * rng.standard_normal((30 + 5 * i, 128))).astype(np.float32)
        (base / f"s{i}.wav").write_bytes(b"")                  # the audio itself is never read: every file has its cache
        np.save(base / "embeddings" / "vggish" / f"s{i}.npy", emb[f"s{i}"])
    songs = {"copy": emb["s0"], "noisy": (emb["s1"] + 0.01 * rng.standard_normal(emb["s1"].shape)).astype(np.float32),
             "excerpt": emb["s2"][10:25].copy()}
    for i in range(3):
        songs[f"fresh{i}"] = (rng.standard_normal(128) + 0.3 * rng.standard_normal((35, 128))).astype(np.float32)
    for name, e in songs.items():
        (evl / f"{name}.wav").write_bytes(b"")
        np.save(evl / "embeddings" / "vggish" / f"{name}.npy", e)
    (evl / "wide.wav").write_bytes(b"")                         # dropped with a log line: wrong D
    np.save(evl / "embeddings" / "vggish" / "wide.npy", np.zeros((4, 64), np.float32))
    return base, evl


def _check_csv(path, base):
    lines = Path(path).read_text().splitlines()
    assert lines[0] == "path,copied_share,min_distance,nearest_baseline,match_share"
    rows = [line.split(",") for line in lines[1:]]
    assert len(rows) == 6
    names = [Path(r[0]).stem for r in rows]
    assert set(names[:3]) == {"copy", "noisy", "excerpt"}, names
    want = {"copy": "s0", "noisy": "s1", "excerpt": "s2"}
    for r in rows[:3]:
        assert Path(r[3]).stem == want[Path(r[0]).stem] and Path(r[3]).parent == base, r
        assert float(r[4]) >= 0.99, r
    assert float(rows[names.index("copy")][1]) == 1.0 and float(rows[names.index("copy")][2]) < 0.1
    for r in rows[3:]:
        assert Path(r[0]).stem.startswith("fresh") and float(r[1]) <= 0.05, r
    shares = [float(r[1]) for r in rows]
    assert shares == sorted(shares, reverse=True)


def test_nearest_score_individual_and_cli_end_to_end(tmp_path):
    from fadtk_amd import NearestNeighbours
    from fadtk_amd.model_loader import get_all_models
    base, evl = _songs(tmp_path)
    ml = {m.name: m for m in get_all_models()}["vggish"]
    nn = NearestNeighbours(ml, audio_load_worker=2)
    out = nn.score_individual(base, evl, tmp_path / "indiv.csv")
    _check_csv(out, base)

    env = dict(os.environ, PYTHONPATH=str(ROOT))
    csv = tmp_path / "cli_indiv.csv"
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.nearest", "vggish", str(base), str(evl), str(csv), "--indiv", "-w", "2"],
                       capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_csv(csv, base)
    assert csv.read_text() == Path(out).read_text()
    (evl / "wide.wav").unlink()                                # the set-level score concatenates every file of the directory
    res = nn.score(base, evl)
    assert 0 < res["copied"] < res["m"] and res["authenticity"] == 1 - res["copied"] / res["m"]
    set_csv = tmp_path / "set.csv"
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.nearest", "vggish", str(base), str(evl), str(set_csv), "-k", "3", "-w", "2"],
                       capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = set_csv.read_text().splitlines()
    assert lines[0].startswith("model,baseline,eval,k,authenticity,copied") and len(lines) == 2
    row = lines[1].split(",")
    assert row[0] == "vggish" and int(row[3]) == 3 and float(row[4]) == res["authenticity"] and int(row[5]) == res["copied"]
