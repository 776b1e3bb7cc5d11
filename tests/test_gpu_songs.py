"""Per-song FAD (fad_frechet_batched_vs_baseline, the --indiv path) over its routes, frame dtypes, row placements, mean modes and
non-finite songs, against the float64 reference of songs_reference.py.

Routes by a song's frame count n at feature dimension D: n = 2 closed form; 3 <= n <= 64 (n - 1 < D) Gram + Jacobi; 65 <= n <= D Gram +
Newton-Schulz; n >= D + 1: the batched low-precision chain (D in CHAIN_D), the symmetric cov(Xc sqrt(Sigma_b)) route (D + 1 .. 8 D frames,
D >= 64) or the D x D product route.  The statistics kernel follows the call's average frame count (>= 64 or not), the dtype and the row
alignment; host rows are staged to ld = D, device rows keep their pitch."""
import logging

import numpy as np
import pytest

import songs_reference as SR
from oracle import fad_oracle as O

pytestmark = pytest.mark.gpu
logging.getLogger("fad_oracle").setLevel(logging.CRITICAL)

CHAIN_D = (128, 256, 384, 512, 768, 1024)
DTYPES = ("float16", "bfloat16", "float32", "float64")
PLACEMENTS = ("host", "dev", "pitch8", "odd")
FAD_ERR_TOO_FEW_ROWS, FAD_ERR_NOT_FINITE = -6, -7


@pytest.fixture(scope="module")
def hip():
    from fadtk_amd import _capi, hip
    _capi.require_gpu(0)
    return hip


def route(n, d):
    if n < 2:
        return "none"
    if n == 2:
        return "closed"
    if n - 1 < d:
        return "gram" if n <= 64 else "gram_ns"
    if d in CHAIN_D:
        return "chain"
    return "sym" if d >= 64 and n <= 8 * d else "product"


def rtol_of(n, d):
    """No looser than test_gpu_parity.py on the same route: 1e-6 off the chain, 2e-6 on it, 2e-5 for songs of D + 1 .. D + 15 frames."""
    if d + 1 <= n <= d + 15:
        return 2e-5
    return 2e-6 if route(n, d) == "chain" else 1e-6


def baseline(seed, d):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((4 * d + 8, d)) * (0.6 + rng.random(d)) + 0.5 + 0.2 * rng.standard_normal(d)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def songs64(seed, counts, d):
    """float64 frames with column gains and an offset (the mean modes then differ); one constant song and one of repeated frames."""
    rng = np.random.default_rng(seed)
    out = [rng.standard_normal((n, d)) * (0.6 + rng.random(d)) + 0.5 + 0.2 * rng.standard_normal(d) for n in counts]
    return out


def store(x, dtype):
    if dtype == "bfloat16":
        import torch
        return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16)
    return np.ascontiguousarray(x).astype(dtype)


def concat(stored):
    if type(stored[0]).__module__.split(".")[0] == "torch":
        import torch
        return torch.cat(stored, 0)
    return np.concatenate(stored, axis=0)


def place(rows, placement):
    """host rows as stored (numpy, or a CPU bfloat16 tensor); device rows contiguous, with a pitch that keeps the 16-byte vector paths
    (ld % 8 == 0, aligned base) or one that defeats them (base one column in, ld = d + 2).  Padding columns hold NaN."""
    import torch
    if placement == "host":
        return rows
    t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(rows)
    if placement == "dev":
        return t.cuda()
    n, d = t.shape
    if placement == "pitch8":
        ld = 8 * ((d + 8) // 8)
        big = torch.full((n, ld), float("nan"), dtype=t.dtype, device="cuda")
        big[:, :d] = t.cuda()
        return big[:, :d]
    big = torch.full((n, d + 2), float("nan"), dtype=t.dtype, device="cuda")
    big[:, 1:d + 1] = t.cuda()
    return big[:, 1:d + 1]


def offsets_of(stored):
    return np.concatenate([[0], np.cumsum([s.shape[0] for s in stored])]).astype(np.int64)


def vector_paths_differ(dtype, d, placement):
    """float16 rows take one-pass 16-byte kernels (song_stats_f16 / song_cov_f16) only when d % 8 == 0, ld % 8 == 0 and the base is aligned:
    the `odd` placement then runs other kernels than contiguous rows and is held to the reference only."""
    return dtype == "float16" and d % 8 == 0 and placement == "odd"


def counts_for(d):
    if d >= 384:                                        # the big D: two or three songs
        return [3, d + 1, 3 * d]
    c = sorted({n for n in (2, 3, 64, 65, d, d + 1, 8 * d, 8 * d + 1, 300) if n >= 2})
    return c


def case_songs(d):
    counts = counts_for(d)
    sg = songs64(1000 + d, counts, d)
    if d < 384:
        flat = np.tile(sg[0][:1], (d + 5, 1))           # Sigma_s = 0
        rep = songs64(2000 + d, [40], d)[0]
        rep[10:] = rep[9]                               # repeated frames
        sg = sg + [flat, rep]
    return sg


class Worst:
    def __init__(self):
        self.err = {}

    def add(self, key, got, want):
        e = abs(got - want) / abs(want)
        self.err[key] = max(self.err.get(key, 0.0), e)
        return e

    def show(self, title):
        print(f"\n[{title}] worst relative error per route: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(self.err.items())))


# --------------------------------------------------------------------------------- a + b: routes x dtypes x placements x mean modes
@pytest.mark.parametrize("d", [1, 17, 63, 65, 130, 200] + list(CHAIN_D))
def test_routes_dtypes_placements_against_the_reference(hip, d):
    mu_b, cov_b = baseline(10 + d, d)
    base = SR.Baseline(mu_b, cov_b)
    sg64 = case_songs(d)
    worst = Worst()
    bad = []
    for dtype in DTYPES:
        stored = [store(x, dtype) for x in sg64]
        parts = [base.parts(s) for s in stored]
        ns = [s.shape[0] for s in stored]
        # call A: every song (average >= 64 frames: the long-song statistics kernels, deferred mean terms);
        # call B: the short songs and the D + 1 song padded with two-frame songs to an average under 64 (per-song statistics, no deferral)
        short = [i for i, n in enumerate(ns) if n <= 65 or n == d + 1]
        pad2 = [i for i, n in enumerate(ns) if n == 2]
        while pad2 and sum(ns[i] for i in short) >= 64 * len(short):
            short.append(pad2[0])
        calls = {"A": list(range(len(stored))), "B": short}
        for cname, idx in calls.items():
            rows = concat([stored[i] for i in idx])
            offs = offsets_of([stored[i] for i in idx])
            for mode in (0, 1):
                got = {}
                for pl in PLACEMENTS:
                    scores, status = hip.frechet_batched(mu_b, cov_b, place(rows, pl), offs, mean_mode=mode)
                    got[pl] = scores
                    for j, i in enumerate(idx):
                        n = ns[i]
                        want = parts[i][0][mode] + parts[i][1]
                        if status[j] != 0:
                            bad.append((dtype, cname, mode, pl, n, "status", int(status[j])))
                            continue
                        e = worst.add(route(n, d), scores[j], want)
                        if not e <= rtol_of(n, d):
                            bad.append((dtype, cname, mode, pl, n, route(n, d), e))
                for pl in ("host", "pitch8", "odd"):         # b: the same bits wherever the rows live, unless other kernels ran
                    if vector_paths_differ(dtype, d, pl):
                        continue
                    if not np.array_equal(got[pl], got["dev"]):
                        bad.append((dtype, cname, mode, pl, "bits differ from contiguous device rows",
                                    float(np.nanmax(np.abs(got[pl] - got["dev"]) / np.abs(got["dev"])))))
    worst.show(f"D={d}")
    assert not bad, bad[:20]


@pytest.mark.parametrize("d", CHAIN_D)
def test_chain_against_the_float64_routes_and_strict_mode(hip, monkeypatch, d):
    """FAD_SONG_FAST=0 (float64 routes only) gives the same scores to the chain's tolerance; FAD_SONG_FAST=2 raises if the chain takes no
    song, so a call that passes under it had songs on the chain -- and gives the same bits as the default."""
    import torch
    mu_b, cov_b = baseline(10 + d, d)
    sg = [s for s in case_songs(d) if s.shape[0] >= d + 1 and np.ptp(s, axis=0).max() > 0]
    for dtype in ("float16", "float32"):
        stored = [store(x, dtype) for x in sg]
        rows = torch.from_numpy(concat(stored)).cuda()
        offs = offsets_of(stored)
        scores, status = hip.frechet_batched(mu_b, cov_b, rows, offs, mean_mode=1)
        monkeypatch.setenv("FAD_SONG_FAST", "2")
        strict, st2 = hip.frechet_batched(mu_b, cov_b, rows, offs, mean_mode=1)
        monkeypatch.setenv("FAD_SONG_FAST", "0")
        f64, st0 = hip.frechet_batched(mu_b, cov_b, rows, offs, mean_mode=1)
        monkeypatch.delenv("FAD_SONG_FAST")
        assert (status == 0).all() and (st2 == 0).all() and (st0 == 0).all(), (status, st2, st0)
        assert np.array_equal(strict, scores)
        for s, a, b in zip(stored, scores, f64):
            assert abs(a - b) <= rtol_of(s.shape[0], d) * abs(b), (dtype, s.shape[0], a, b)


@pytest.mark.parametrize("d", [17, 65, 130, 128, 256, 768])
def test_offsets_inside_the_rows_and_permuted_songs_give_the_same_bits(hip, d):
    """Songs whose offsets start after row 0 and end before n_rows (the rows around them NaN) score as the same songs passed alone, and
    permuting the songs permutes the scores and statuses bit for bit: no kernel reads outside a song, and no song's bits depend on its
    slot in the batch."""
    import torch
    mu_b, cov_b = baseline(10 + d, d)
    sg = case_songs(d) + [np.zeros((1, d))]                          # a one-frame song rides along
    for dtype in ("float16", "bfloat16", "float32", "float64"):
        stored = [store(x, dtype) for x in sg]
        rows = concat(stored)
        t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(rows)
        offs = offsets_of(stored)
        for mode in (0, 1):
            alone, st_alone = hip.frechet_batched(mu_b, cov_b, t.cuda(), offs, mean_mode=mode)
            framed = torch.full((t.shape[0] + 8, d), float("nan"), dtype=t.dtype, device="cuda")
            framed[3:3 + t.shape[0]] = t.cuda()
            inside, st_inside = hip.frechet_batched(mu_b, cov_b, framed, offs + 3, mean_mode=mode)
            assert np.array_equal(st_inside, st_alone) and np.array_equal(inside, alone, equal_nan=True), (dtype, mode)
            perm = np.random.default_rng(d).permutation(len(stored))
            pst = [stored[i] for i in perm]
            prow = concat(pst)
            pt = prow if isinstance(prow, torch.Tensor) else torch.from_numpy(prow)
            ps, pstat = hip.frechet_batched(mu_b, cov_b, pt.cuda(), offsets_of(pst), mean_mode=mode)
            assert np.array_equal(pstat, st_alone[perm]), (dtype, mode)
            assert np.array_equal(ps, alone[perm], equal_nan=True), (dtype, mode, np.nanmax(np.abs(ps - alone[perm]) / np.abs(alone[perm])))


# --------------------------------------------------------------------------------- c: non-finite songs
def _bad_songs(x):
    """x float64 [n x d] -> four songs of the same length with non-finite frames, and the finite songs that replace them."""
    n, d = x.shape
    c = d // 2
    out = []
    for kind in ("nan_first", "nan_last", "inf", "pm_inf"):
        b = x.copy()
        if kind == "nan_first":
            b[0, c] = np.nan
        elif kind == "nan_last":
            b[-1, c] = np.nan
        elif kind == "inf":
            b[n // 2, c] = np.inf
        else:
            b[0, c] = np.inf
            b[-1, c] = -np.inf
        out.append((b, np.where(np.isfinite(b), b, 0.25)))
    return out


def _nonfinite_case(d):
    lengths = sorted({n for n in (2, 3, 40, 65, d + 1, 8 * d + 1) if n >= 2})
    good = songs64(3000 + d, lengths, d)
    songs, clean, is_bad = [], [], []
    for g in good:
        songs.append(g); clean.append(g); is_bad.append(False)
        for b, c in _bad_songs(g + 0.125):
            songs.append(b); clean.append(c); is_bad.append(True)
    return songs, clean, np.array(is_bad)


def _check_nonfinite(hip, mu_b, cov_b, songs, clean, is_bad, dtype, pl, mode, what):
    st_s = [store(x, dtype) for x in songs]
    st_c = [store(x, dtype) for x in clean]
    offs = offsets_of(st_s)
    scores, status = hip.frechet_batched(mu_b, cov_b, place(concat(st_s), pl), offs, mean_mode=mode)
    ref, ref_st = hip.frechet_batched(mu_b, cov_b, place(concat(st_c), pl), offs, mean_mode=mode)
    ns = [s.shape[0] for s in st_s]
    msg = (what, dtype, pl, mode)
    bad_routes = sorted({route(ns[i], mu_b.shape[0]) for i in np.flatnonzero(is_bad) if status[i] != FAD_ERR_NOT_FINITE or not np.isnan(scores[i])})
    assert not bad_routes, (msg, "non-finite songs scored", bad_routes, status[is_bad], scores[is_bad])
    assert (ref_st == 0).all(), (msg, ref_st)
    assert np.array_equal(status[~is_bad], ref_st[~is_bad]), (msg, status, ref_st)
    # At a chain D the bad songs leave the chain for the float64 D x D routes while their finite stand-ins stay on it, so a good song the
    # chain declines shares float64 launches with a different number of problems -- and gemm_f64_launch picks its tile and wave split by
    # that number (pick_bt), which orders the sums differently.  Those songs are held to 1e-12; every other song to the bit.
    d = mu_b.shape[0]
    moved = [(ns[i], route(ns[i], d), abs(scores[i] - ref[i]) / abs(ref[i])) for i in np.flatnonzero(~is_bad) if scores[i] != ref[i]]
    moved = [m for m in moved if not (m[1] == "chain" and m[2] <= 1e-12)]
    assert not moved, (msg, "good songs whose bits follow the bad songs of the batch", moved)


@pytest.mark.parametrize("d", [1, 17, 65, 130])
def test_non_finite_songs_every_route_dtype_and_placement(hip, d):
    """One NaN in the first frame, one in the last, +Inf in one column, +Inf and -Inf in one column: status FAD_ERR_NOT_FINITE and a NaN
    score in every route (the reference's eig raises and score_individual drops the song), and every other song of the batch keeps the
    bits it has when the bad songs' frames are replaced by finite ones."""
    mu_b, cov_b = baseline(20 + d, d)
    songs, clean, is_bad = _nonfinite_case(d)
    for dtype in DTYPES:
        for pl in ("host", "dev"):
            for mode in (0, 1):
                _check_nonfinite(hip, mu_b, cov_b, songs, clean, is_bad, dtype, pl, mode, f"D={d}")


@pytest.mark.parametrize("d", [128, 256])
def test_non_finite_songs_on_the_chain(hip, monkeypatch, d):
    """The same on the chain's dimensions, in batches on both sides of FAD_SONG_BIG and, at D = 128, with FAD_SONG_RES on and off."""
    mu_b, cov_b = baseline(20 + d, d)
    songs, clean, is_bad = _nonfinite_case(d)
    for dtype in DTYPES:
        for pl in ("host", "dev"):
            for mode in (0, 1):
                _check_nonfinite(hip, mu_b, cov_b, songs, clean, is_bad, dtype, pl, mode, f"D={d}")
    variants = [(big, res) for big in ("1", "0") for res in (("0", "2") if d == 128 else ("2",))]
    for big, res in variants:
        monkeypatch.setenv("FAD_SONG_BIG", big)
        monkeypatch.setenv("FAD_SONG_RES", res)
        for dtype in ("float16", "float32"):
            _check_nonfinite(hip, mu_b, cov_b, songs, clean, is_bad, dtype, "dev", 1, f"D={d} BIG={big} RES={res}")


@pytest.mark.parametrize("d", [17, 65, 130, 256])
def test_baseline_with_a_nan_off_the_diagonal(hip, d):
    """tr Sigma_b stays finite, yet no song of two or more frames can be scored: all get FAD_ERR_NOT_FINITE, the one-frame song -6."""
    mu_b, cov_b = baseline(30 + d, d)
    cov_b = cov_b.copy()
    cov_b[0, 1] = np.nan
    lengths = sorted({n for n in (1, 2, 3, 40, 65, d + 1, 3 * d) if n >= 1})
    sg = songs64(4000 + d, lengths, d)
    for dtype in ("float16", "float32"):
        for pl in ("host", "dev"):
            stored = [store(x, dtype) for x in sg]
            scores, status = hip.frechet_batched(mu_b, cov_b, place(concat(stored), pl), offsets_of(stored), mean_mode=1)
            want = np.array([FAD_ERR_TOO_FEW_ROWS if n < 2 else FAD_ERR_NOT_FINITE for n in lengths])
            assert np.array_equal(status, want), (dtype, pl, list(zip(lengths, status, scores)))
            assert np.isnan(scores).all()


# --------------------------------------------------------------------------------- d: end to end through score_individual
class _Toy:
    def __init__(self, name):
        self.name = name
        self.sr = 16000

    def load_model(self):
        raise AssertionError("not needed")


def test_score_individual_mixed_dtypes_short_and_non_finite_files(tmp_path):
    import fadtk_amd as F
    from fadtk_amd import _capi
    _capi.require_gpu(0)
    model, d = "toy", 48
    rng = np.random.default_rng(5)
    mu_b, cov_b = baseline(6, d)
    spec = {"a.wav": (200, np.float16), "b.wav": (50, np.float32), "c.wav": (3, np.float16), "one.wav": (1, np.float32),
            "nan.wav": (30, np.float16), "e.wav": (2, np.float32), "f.wav": (90, np.float32), "g.wav": (64, np.float16)}
    evald = tmp_path / "eval"
    (evald / "embeddings" / model).mkdir(parents=True)
    paths, arrays = [], []
    for nm, (n, dt) in spec.items():
        x = (rng.standard_normal((n, d)) * (0.6 + rng.random(d)) + 0.5).astype(dt)
        if nm == "nan.wav":
            x[7, 3] = np.nan
        (evald / nm).write_bytes(b"")
        np.save(evald / "embeddings" / model / (nm[:-4] + ".npy"), x)
        paths.append(evald / nm); arrays.append(x)
    np.savez(tmp_path / "base.npz", **{f"{model}.mu": mu_b, f"{model}.cov": cov_b})
    fad = F.FrechetAudioDistance(_Toy(model), audio_load_worker=2, load_model=False)
    out = fad.score_individual(str(tmp_path / "base.npz"), evald, tmp_path / "indiv.csv")
    want = O.individual_csv_text(paths, O.individual_scores(mu_b, cov_b, arrays, run_sqrtm=False))
    got = [ln.rsplit(",", 1) for ln in out.read_text().split("\n")]
    wantl = [ln.rsplit(",", 1) for ln in want.split("\n")]
    assert [a for a, _ in got] == [a for a, _ in wantl]
    assert len(got) == len(spec) - 2                                  # the one-frame and the NaN file dropped
    np.testing.assert_allclose([float(b) for _, b in got], [float(b) for _, b in wantl], rtol=1e-6)
