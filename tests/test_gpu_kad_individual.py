"""Per-song Kernel Audio Distance on the GPU (fad_kad_individual, csrc/kad.hip): every song against the float64 reference of
tests/kad_reference.py and against fad_kad on the song alone; the baseline terms bit for bit those of fad_kad; bitwise determinism;
a non-finite row flags only its song; permuted songs; the scale check against torch float64; the command line end to end."""
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

MEAN_RTOL = 4e-7          # the tolerances of test_gpu_kad.py: each mean relative, MMD^2 against the scale of its terms
MMD_TOL = 1.5e-7
TOO_FEW, NOT_FINITE = -6, -7
LENGTHS = [0, 1, 2, 3, 127, 128, 129, 300]


def _ref_kxx(x, sigma):
    """Kxx of the float64 reference, by a float64 matmul (the cdist of kad_reference at n = 3000 and D = 1024 takes long)."""
    x = np.asarray(x, dtype=np.float64)
    nx = (x * x).sum(1)
    d2 = np.maximum(nx[:, None] + nx[None, :] - 2.0 * x @ x.T, 0.0)
    k = np.exp(-d2 / (2.0 * sigma * sigma))
    np.fill_diagonal(k, 0.0)
    n = x.shape[0]
    return float(k.sum() / (n * (n - 1)))


def _ref_song(kxx, x, y, sigma):
    kyy, kxy = R._kmean(y, y, sigma, True), R._kmean(x, y, sigma, False)
    return {"kxx_mean": kxx, "kyy_mean": kyy, "kxy_mean": kxy, "mmd2": kxx + kyy - 2.0 * kxy}


def _check_song(got, s, want, label):
    g = {k: got[k][s] for k in ("kyy_mean", "kxy_mean", "mmd2")}
    for k in ("kyy_mean", "kxy_mean"):
        assert g[k] == pytest.approx(want[k], rel=MEAN_RTOL), (label, s, k, g[k], want[k])
    scale = want["kxx_mean"] + want["kyy_mean"] + 2 * want["kxy_mean"]
    assert abs(g["mmd2"] - want["mmd2"]) <= MMD_TOL * scale, (label, s, g["mmd2"], want["mmd2"])
    return max(abs(g["kyy_mean"] - want["kyy_mean"]) / want["kyy_mean"], abs(g["kxy_mean"] - want["kxy_mean"]) / want["kxy_mean"])


def _songs(lengths, d, seed, shift=0.3):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((m, d)) * (1.0 + 0.05 * (s % 3)) + shift * (s % 2)).astype(np.float32) for s, m in enumerate(lengths)]


def _offsets(songs):
    return np.concatenate([[0], np.cumsum([len(y) for y in songs])]).astype(np.int64)


@pytest.mark.parametrize("d", [1, 17, 128, 768, 1024])
def test_kad_individual_float16_matches_float64_and_fad_kad(d):
    from fadtk_amd import hip
    rng = np.random.default_rng(d)
    x = rng.standard_normal((2999, d)).astype(np.float16)
    songs = [y.astype(np.float16) for y in _songs(LENGTHS, d, seed=d + 1)]
    rows = np.concatenate(songs)
    got = hip.kad_individual(x, rows, _offsets(songs))
    sigma = got["bandwidth"]
    assert sigma == hip.kad_median_distance(x)                                          # bit for bit
    assert sigma == pytest.approx(R.median_distance(x), rel=1e-5)
    kxx = _ref_kxx(x, sigma)
    assert got["kxx_mean"] == pytest.approx(kxx, rel=MEAN_RTOL) and got["n"] == 2999
    worst = 0.0
    for s, y in enumerate(songs):
        if len(y) < 2:
            assert got["status"][s] == TOO_FEW and np.isnan(got["mmd2"][s]) and np.isnan(got["kyy_mean"][s]), (s, len(y))
            continue
        assert got["status"][s] == 0
        worst = max(worst, _check_song(got, s, _ref_song(kxx, x, y, sigma), f"f16 d={d} m={len(y)}"))
        one = hip.kad(x, y, bandwidth=sigma)
        assert one["kxx_mean"] == got["kxx_mean"] and one["bandwidth"] == sigma            # the baseline term: bit for bit
        for k in ("kyy_mean", "kxy_mean"):
            assert got[k][s] == pytest.approx(one[k], rel=MEAN_RTOL), (d, s, k)
        assert abs(got["mmd2"][s] - one["mmd2"]) <= MMD_TOL * (one["kxx_mean"] + one["kyy_mean"] + 2 * one["kxy_mean"])
    print(f"[kad-indiv-err] f16 d={d}: worst mean rel {worst:.2e}")


@pytest.mark.parametrize("dtype", ["bfloat16", "float32", "float16"])
@pytest.mark.parametrize("d,ld", [(17, 24), (768, 776)])
def test_kad_individual_dtypes_and_row_pitch_on_device(dtype, d, ld):
    import torch
    from fadtk_amd import hip
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(ld)
    x = rng.standard_normal((700, d)).astype(np.float32)
    songs = _songs(LENGTHS, d, seed=ld + 1)
    rows = np.concatenate(songs)
    xw = torch.zeros((700, ld), dtype=tdt, device="cuda")
    yw = torch.zeros((len(rows), ld), dtype=tdt, device="cuda")
    xw[:, :d] = torch.from_numpy(x).to(tdt)
    yw[:, :d] = torch.from_numpy(rows).to(tdt)
    xv, yv = xw[:, :d], yw[:, :d]                                                       # ld > D, used in place
    bw = float(np.sqrt(2 * d))                                                          # about the median distance: a given bandwidth
    got = hip.kad_individual(xv, yv, _offsets(songs), bandwidth=bw)
    assert got["bandwidth"] == bw
    xr, yr = xv.float().cpu().numpy(), yv.float().cpu().numpy()
    kxx = _ref_kxx(xr, bw)
    off = _offsets(songs)
    for s in range(len(songs)):
        if off[s + 1] - off[s] < 2:
            assert got["status"][s] == TOO_FEW
            continue
        _check_song(got, s, _ref_song(kxx, xr, yr[off[s]:off[s + 1]], bw), f"{dtype} d={d} ld={ld}")
    if dtype == "float32":                                                              # the host route of the same rows
        host = hip.kad_individual(np.ascontiguousarray(xr), np.ascontiguousarray(yr), off, bandwidth=bw)
        for k in ("mmd2", "kyy_mean", "kxy_mean", "status"):
            assert host[k].tobytes() == got[k].tobytes(), k


def test_kad_individual_is_deterministic_and_isolates_a_nan_row():
    import torch
    from fadtk_amd import hip
    rng = np.random.default_rng(21)
    x = torch.from_numpy(rng.standard_normal((3000, 256)).astype(np.float16)).cuda()
    songs = _songs([5, 2, 140, 0, 300, 1, 129, 77, 2, 400], 256, seed=22)
    rows = torch.from_numpy(np.concatenate(songs)).half().cuda()
    off = _offsets(songs)
    a, b = hip.kad_individual(x, rows, off), hip.kad_individual(x, rows, off)
    for k in ("mmd2", "kyy_mean", "kxy_mean", "status"):
        assert a[k].tobytes() == b[k].tobytes(), k                                     # bitwise: no float atomics anywhere
    assert a["kxx_mean"] == b["kxx_mean"] and a["bandwidth"] == b["bandwidth"]
    full = hip.kad(x, rows)                                                           # the baseline term and sigma of fad_kad
    assert full["kxx_mean"] == a["kxx_mean"] and full["bandwidth"] == a["bandwidth"]

    bad = rows.clone()
    bad[off[4] + 17, 3] = float("nan")                                                 # one row of song 4
    c = hip.kad_individual(x, bad, off)
    assert c["status"][4] == NOT_FINITE and np.isnan(c["mmd2"][4]) and np.isnan(c["kyy_mean"][4]) and np.isnan(c["kxy_mean"][4])
    keep = np.arange(len(songs)) != 4
    for k in ("mmd2", "kyy_mean", "kxy_mean", "status"):
        assert c[k][keep].tobytes() == a[k][keep].tobytes(), k
    bad[off[4] + 17, 3] = float("inf")
    c = hip.kad_individual(x, bad, off)
    assert c["status"][4] == NOT_FINITE and (c["status"][keep] == a["status"][keep]).all()
    assert c["mmd2"][keep].tobytes() == a["mmd2"][keep].tobytes()


def test_kad_individual_permuted_songs_permute_the_results():
    from fadtk_amd import hip
    rng = np.random.default_rng(31)
    x = rng.standard_normal((1500, 128)).astype(np.float16)
    songs = [y.astype(np.float16) for y in _songs([3, 250, 2, 129, 64, 1, 300, 127, 128, 9], 128, seed=32)]
    perm = rng.permutation(len(songs))
    a = hip.kad_individual(x, np.concatenate(songs), _offsets(songs))
    p_songs = [songs[i] for i in perm]
    b = hip.kad_individual(x, np.concatenate(p_songs), _offsets(p_songs))
    assert a["kxx_mean"] == b["kxx_mean"]
    assert (b["status"] == a["status"][perm]).all()
    ok = a["status"][perm] == 0
    for k in ("kyy_mean", "kxy_mean"):
        np.testing.assert_allclose(b[k][ok], a[k][perm][ok], rtol=MEAN_RTOL)
    scale = a["kxx_mean"] + a["kyy_mean"][perm][ok] + 2 * a["kxy_mean"][perm][ok]
    assert (np.abs(b["mmd2"][ok] - a["mmd2"][perm][ok]) <= MMD_TOL * scale).all()


def test_kad_individual_scale_against_torch_float64():
    import torch
    from fadtk_amd import hip
    gen = torch.Generator(device="cuda").manual_seed(2026)
    x = torch.randn((100_000, 512), generator=gen, device="cuda").half()
    lens = np.random.default_rng(41).integers(2, 401, size=2000)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    M = int(off[-1])
    y = (torch.randn((M, 512), generator=gen, device="cuda") * 1.05 + 0.02).half()
    got = hip.kad_individual(x, y, off)
    sigma = got["bandwidth"]
    assert (got["status"] == 0).all()

    g = 1.0 / (2.0 * sigma * sigma)
    xd, yd = x.double(), y.double()
    nx, ny = (xd * xd).sum(1), (yd * yd).sum(1)
    col = torch.zeros(M, dtype=torch.float64, device="cuda")                            # sum over x of k(x, y_j), chunk by chunk
    kxx = torch.zeros((), dtype=torch.float64, device="cuda")
    for i0 in range(0, x.shape[0], 4096):
        xc = xd[i0:i0 + 4096]
        for j0 in range(0, M, 65536):
            d2 = (nx[i0:i0 + 4096, None] + ny[None, j0:j0 + 65536] - 2.0 * xc @ yd[j0:j0 + 65536].T).clamp_min_(0)
            col[j0:j0 + 65536] += torch.exp(-g * d2).sum(0)
        d2 = (nx[i0:i0 + 4096, None] + nx[None, :] - 2.0 * xc @ xd.T).clamp_min_(0)
        idx = torch.arange(xc.shape[0], device="cuda")
        d2[idx, idx + i0] = float("inf")
        kxx += torch.exp(-g * d2).sum()
        del d2
    n = x.shape[0]
    kxx = float(kxx) / (n * (n - 1))
    sid = torch.repeat_interleave(torch.arange(len(lens), device="cuda"), torch.from_numpy(lens).cuda())
    kxy = torch.zeros(len(lens), dtype=torch.float64, device="cuda").index_add_(0, sid, col).cpu().numpy() / (n * lens)
    kyy = np.empty(len(lens))
    for s in range(len(lens)):
        ys = yd[off[s]:off[s + 1]]
        d2 = (ny[off[s]:off[s + 1], None] + ny[None, off[s]:off[s + 1]] - 2.0 * ys @ ys.T).clamp_min_(0)
        d2.fill_diagonal_(float("inf"))
        kyy[s] = float(torch.exp(-g * d2).sum()) / (lens[s] * (lens[s] - 1))
    assert got["kxx_mean"] == pytest.approx(kxx, rel=MEAN_RTOL)
    rel_yy = np.abs(got["kyy_mean"] - kyy) / kyy
    rel_xy = np.abs(got["kxy_mean"] - kxy) / kxy
    mmd = kxx + kyy - 2 * kxy
    rel_mmd = np.abs(got["mmd2"] - mmd) / (kxx + kyy + 2 * kxy)
    print(f"[kad-indiv-err] 100000 x 512 f16, 2000 songs ({M} rows): kyy {rel_yy.max():.2e} kxy {rel_xy.max():.2e} "
          f"mmd2/scale {rel_mmd.max():.2e}")
    assert rel_yy.max() <= MEAN_RTOL and rel_xy.max() <= MEAN_RTOL and rel_mmd.max() <= MMD_TOL


def test_kad_individual_cli_end_to_end(tmp_path):
    from fadtk_amd import FrechetAudioDistance, calc_kernel_audio_distance_individual
    rng = np.random.default_rng(6)
    lens = {"base": [40 + 7 * i for i in range(6)], "evl": [33, 0, 2, 1, 150, 9, 61]}
    for name, shift in (("base", 0.0), ("evl", 0.4)):
        d = tmp_path / name
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i, m in enumerate(lens[name]):
            (d / f"s{i}.wav").write_bytes(b"")             # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"s{i}.npy", (rng.standard_normal((m, 128)) * (1 + 0.1 * i) + shift).astype(np.float32))
    csv = tmp_path / "indiv.csv"
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "vggish", str(tmp_path / "base"), str(tmp_path / "evl"), str(csv),
                        "--indiv", "--scale", "10", "-w", "2"], capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [line.split(",") for line in csv.read_text().splitlines()]
    names = [Path(p).name for p, _ in rows]
    assert sorted(names) == sorted(f"s{i}.wav" for i, m in enumerate(lens["evl"]) if m >= 2)
    scores = [float(v) for _, v in rows]
    assert scores == sorted(scores, key=abs)
    for dropped in ("s1.wav", "s3.wav"):
        assert dropped in r.stderr, r.stderr[-3000:]

    from fadtk_amd.model_loader import get_all_models
    ml = {m.name: m for m in get_all_models()}["vggish"]
    fad = FrechetAudioDistance(ml, load_model=False)
    x = fad.load_embeddings(tmp_path / "base")
    files = [f for f in (tmp_path / "evl").glob("*.*") if fad.read_embedding_file(f).shape[0] >= 2]
    values = calc_kernel_audio_distance_individual(x, [fad.read_embedding_file(f) for f in files], scale=10.0)
    want = {f.name: v for f, v in zip(files, values)}
    got = dict(zip(names, scores))
    assert got == want
    sigma = R.median_distance(x)
    for f in files:
        assert got[f.name] == pytest.approx(10 * R.kad(x, fad.read_embedding_file(f), sigma)["mmd2"], rel=1e-4, abs=1e-6)

    r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "vggish", str(tmp_path / "base"), str(tmp_path / "evl"), "--indiv"],
                       capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
    assert r.returncode == 0 and (tmp_path / "kad-individual-results.csv").is_file(), r.stderr[-3000:]
