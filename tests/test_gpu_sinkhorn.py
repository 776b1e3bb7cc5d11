"""The Sinkhorn divergence on the GPU (fad_sinkhorn; csrc/kad.hip) against the float64 reference of
tests/sinkhorn_reference.py on the same values, upcast.  Standard normal rows rounded to the dtype; the shapes are the smallest that
reach a ragged k step (D = 37), one row in a second tile (129), a padding column (127), exact tiles (128), three row ranges to merge
(257: cross_rows_per_unit gives one row block per unit at these sizes) and a single pair (1, 1).

Potentials, the three OT terms and the divergence are compared in units of
    U = 2^-24 (max |x_i|^2 + max |y_j|^2) + 2^-24 eps log(max(n, m)),
the float32 formation error of C plus that of exp / log; the divergence is a difference of terms of that size, so it has no relative
tolerance.  TOL_U is 4 x the worst ratio error / U measured on an MI355X over this file's cases (the [sinkhorn-err] lines; soft-min is
1-Lipschitz in the sup norm, so the error grows at most linearly in L).  Measured, worst of f, g, F, G over the rows and the four terms:
    blur 0.25 x median (L = 1, 2, 30), 1 x and 1000 x median (L = 2):  fp16 0.74 U, bf16 0.74 U, fp32 0.92 U at most
    blur 0.02 x median (L = 1, 2):  fp16 2.9 U, bf16 2.7 U, fp32 6.7 U at most (129 x 127 x 128, L = 2, F of one row)
    the single pair (1, 1, 5):  1.3 U at most;   the divergence: 0.17 U at most, 0.54 U on the single pair
At the smallest blur the soft-min is the minimum, so a potential carries the formation error of ONE C_ij undamped -- the float32
accumulation over D, longest on the float32 MFMA's k steps of 2 -- where a larger blur averages it over many pairs.
"""
import ctypes as C
import functools
import logging

import numpy as np
import pytest

import sinkhorn_reference as SR

pytestmark = pytest.mark.gpu
TOO_FEW, NOT_FINITE, INVALID = -6, -7, -1
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16", "fp32": "float32"}
MEASURED_WORST_RATIO = 6.675          # 129 x 127 x 128 fp32, L = 2, blur 0.02 x median
TOL_U = 4 * MEASURED_WORST_RATIO
# (L, factor): every L at the default blur, every blur at L = 2, and the first step at the smallest blur (the unshifted float32 sum
# of exp(-C_ij / eps) is exactly 0 for every row there: a missing max shift shows as -inf or NaN)
RUNS = ((1, 0.25), (2, 0.25), (30, 0.25), (2, 0.02), (2, 1.0), (2, 1000.0), (1, 0.02))
POTS = ("f", "g", "pot_x", "pot_y")
TERMS = ("ot_xy", "ot_xx", "ot_yy", "divergence")


def _dev(a, dt, ld=None):
    """float32 values -> a torch CUDA tensor of dtype dt; with ld, a view of a wider buffer (row pitch ld > D) whose pitch bytes are 7"""
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, TORCH_DT[dt]))
    if ld is None:
        return t
    wide = torch.full((t.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _median(n, m, d, dt):
    return SR.median_distance(SR.rows(n, m, d, dt)[0]) if n > 1 else 1.0


@functools.lru_cache(maxsize=None)
def _reference(n, m, d, dt, factor, L):
    x, y = SR.rows(n, m, d, dt)
    return SR.sinkhorn(x, y, (factor * _median(n, m, d, dt)) ** 2, L)


def _ratios(got, want, U):
    """error / U of the four potentials (the worst row) and of the four terms"""
    out = {k: float(np.abs(got[k] - want[k]).max()) / U for k in POTS}
    out.update({k: abs(got[k] - want[k]) / U for k in TERMS})
    return out


def _marginal_tol(want, U, eps):
    """|d/dt |e^t - 1|| = e^t <= 1 + |e^t - 1|, and t = (f - f') / eps carries the error of two potentials"""
    return float(np.expm1(min(2 * TOL_U * U / eps, 50.0))) * (1.0 + want)


def _check(got, want, x, y, tag):
    eps = want["epsilon"]
    U = SR.unit(x, y, eps)
    for k in POTS + TERMS + ("marginal_error", "marginal_error_xx", "marginal_error_yy"):
        assert np.all(np.isfinite(got[k])), (tag, k)
    r = _ratios(got, want, U)
    worst = max(r.values())
    print(f"[sinkhorn-err] {tag}: U {U:.2e} worst {worst:.3f} | " + " ".join(f"{k} {v:.3f}" for k, v in r.items())
          + f" | marginal {got['marginal_error']:.3e} (ref {want['marginal_error']:.3e})")
    assert abs(got["epsilon"] - eps) <= 1e-15 * eps
    assert worst <= TOL_U, (tag, r)
    for k in ("marginal_error", "marginal_error_xx", "marginal_error_yy"):
        assert abs(got[k] - want[k]) <= _marginal_tol(want[k], U, eps), (tag, k, got[k], want[k])
    assert abs(got["pot_x"].mean() + got["pot_y"].mean() - got["divergence"]) <= 1e-12 * max(1.0, abs(got["ot_xy"]))
    return worst


# ----------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("shape", SR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_float64_reference(shape, dt):
    """f, g, F, G row by row, the three OT terms, S and the marginal errors, on device tensors with a row pitch D + 3"""
    from fadtk_amd import hip
    n, m, d = shape
    x, y = SR.rows(n, m, d, dt)
    xd, yd = _dev(x, dt, d + 3), _dev(y, dt, d + 3)
    assert xd.stride(0) == d + 3
    med = _median(n, m, d, dt)
    for L, factor in RUNS:
        eps = (factor * med) ** 2
        got = hip.sinkhorn(xd, yd, epsilon=eps, iterations=L, potentials=True)
        want = _reference(n, m, d, dt, factor, L)
        assert (got["n"], got["m"], got["iterations"]) == (n, m, L)
        _check(got, want, x, y, f"{n}x{m}x{d} {dt} L={L} blur={factor}")
        if (L, factor) == (1, 0.02):                       # f of L = 1 is the first half-step: 0 <= f_i - min_j C_ij <= eps log m
            U = SR.unit(x, y, eps)
            gap = got["f"] - SR.cost(x, y).min(axis=1)
            assert gap.min() >= -TOL_U * U and gap.max() <= eps * np.log(m) + TOL_U * U, (gap.min(), gap.max())


def test_nan_row_is_refused_and_outputs_stay():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(129, 127, 128, "fp32")
    bad = y.copy()
    bad[5, 7] = np.nan
    res = _capi.FadSinkhornResult()
    res.divergence = -5.0
    for a, b in ((x, bad), (bad, x)):
        st = lib.fad_sinkhorn(a.ctypes.data, len(a), 128, b.ctypes.data, len(b), 128, 128, _capi.FAD_F32, 0, 1.0, 3, C.byref(res), None, 0, None)
        assert st == NOT_FINITE and res.divergence == -5.0
    inf = y.copy()
    inf[0, 0] = np.inf
    st = lib.fad_sinkhorn(x.ctypes.data, 129, 128, inf.ctypes.data, 127, 128, 128, _capi.FAD_F32, 0, 1.0, 3, C.byref(res), None, 0, None)
    assert st == NOT_FINITE and res.divergence == -5.0


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_identical_sets_give_exactly_zero(dt):
    """The three problems run the same arithmetic on the same bits."""
    from fadtk_amd import hip
    x, _ = SR.rows(257, 130, 64, dt)
    xd = _dev(x, dt)
    for L, eps in ((1, None), (7, None), (3, 0.5)):
        got = hip.sinkhorn(xd, xd.clone(), epsilon=eps, iterations=L, potentials=True)
        assert got["divergence"] == 0.0 and got["ot_xy"] == got["ot_xx"] == got["ot_yy"]
        assert got["marginal_error"] == got["marginal_error_xx"] == got["marginal_error_yy"]
        assert abs(got["pot_x"].mean() + got["pot_y"].mean()) <= 1e-14 * abs(got["ot_xy"])


def _same_bits(a, b):
    for k in POTS:
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    for k in TERMS + ("epsilon", "marginal_error", "marginal_error_xx", "marginal_error_yy"):
        assert np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64), k


@pytest.mark.parametrize("dt", ("fp16", "fp32"))
def test_repeatable_and_host_equals_device(dt):
    from fadtk_amd import hip
    x, y = SR.rows(300, 200, 37, dt)
    npdt = np.float16 if dt == "fp16" else np.float32
    xh, yh = x.astype(npdt), y.astype(npdt)
    xd, yd = _dev(x, dt, 48), _dev(y, dt)
    for eps in (None, 2.0):
        a = hip.sinkhorn(xd, yd, epsilon=eps, iterations=5, potentials=True)
        b = hip.sinkhorn(xd, yd, epsilon=eps, iterations=5, potentials=True)
        c = hip.sinkhorn(xh, yh, epsilon=eps, iterations=5, potentials=True)
        _same_bits(a, b)
        _same_bits(a, c)
    plain = hip.sinkhorn(xd, yd, epsilon=2.0, iterations=5)                                # no detail: the same result
    assert plain["divergence"] == a["divergence"] and plain["marginal_error"] == a["marginal_error"] and "f" not in plain


@pytest.mark.parametrize("dt", ("fp16", "fp32"))
def test_launch_cut_changes_no_bit(monkeypatch, dt):
    """n = 1200, m = 1100, D = 16: 90 tiles a pass, above the floor of 64 a launch.  A small budget cuts every pass in two; every
    output equals the uncut call bit for bit, and the reference within tolerance."""
    from fadtk_amd import hip
    n, m, d, L = 1200, 1100, 16, 3
    x, y = SR.rows(n, m, d, dt)
    xd, yd = _dev(x, dt), _dev(y, dt)
    monkeypatch.delenv("FAD_KAD_LAUNCH_BUDGET", raising=False)
    whole = hip.sinkhorn(xd, yd, iterations=L, potentials=True)
    plan = hip.kad_last_plan()
    assert plan["max_launches"] == 1 and plan["passes"] == 7                               # the median and 2 directions x 3 problems
    monkeypatch.setenv("FAD_KAD_LAUNCH_BUDGET", "1000")
    cut = hip.sinkhorn(xd, yd, iterations=L, potentials=True)
    plan = hip.kad_last_plan()
    assert plan["max_launches"] >= 2 and plan["passes"] == 7, plan
    monkeypatch.delenv("FAD_KAD_LAUNCH_BUDGET")
    _same_bits(whole, cut)
    want = SR.sinkhorn(x, y, whole["epsilon"], L)
    assert abs(whole["epsilon"] - (SR.BLUR_FACTOR * SR.median_distance(x)) ** 2) <= 1e-6 * whole["epsilon"]
    _check(cut, want, x, y, f"{n}x{m}x{d} {dt} L={L} cut")


# ------------------------------------------------------------------------------------------------------ Python layer
def test_default_epsilon_is_a_quarter_of_the_median_squared():
    from fadtk_amd import hip
    from fadtk_amd.sinkhorn import calc_sinkhorn_divergence
    x, y = SR.rows(300, 200, 37, "fp16")
    xh, yh = x.astype(np.float16), y.astype(np.float16)
    med = hip.kad_median_distance(xh)
    res = calc_sinkhorn_divergence(xh, yh, iterations=4, potentials=True)
    assert res["epsilon"] == (0.25 * med) ** 2 and res["blur"] == np.sqrt(res["epsilon"])
    assert set(res) == {"divergence", "ot_xy", "ot_xx", "ot_yy", "blur", "epsilon", "marginal_error", "iterations", "n", "m",
                        "w2_estimate", "pot_x", "pot_y", "f", "g"}
    raw = hip.sinkhorn(xh, yh, epsilon=None, iterations=4)
    assert res["divergence"] == raw["divergence"] and res["w2_estimate"] == np.sqrt(2 * max(raw["divergence"], 0.0))
    assert res["marginal_error"] == max(raw["marginal_error"], raw["marginal_error_xx"], raw["marginal_error_yy"])
    half = calc_sinkhorn_divergence(xh, yh, blur_factor=0.5, iterations=4)                 # a factor of one's own: the same median
    assert half["epsilon"] == (0.5 * med) ** 2
    same = calc_sinkhorn_divergence(xh, yh, blur=0.25 * med, iterations=4)
    assert abs(same["divergence"] - res["divergence"]) <= 1e-12 * abs(res["ot_xy"])
    mixed = calc_sinkhorn_divergence(xh, y, blur=3.0, iterations=2)                        # mixed dtypes go to float32
    assert mixed["n"] == 300 and mixed["m"] == 200 and np.isfinite(mixed["divergence"])


def test_score_individual_on_a_small_cache(tmp_path, caplog):
    from fadtk_amd import SinkhornDivergence, calc_sinkhorn_divergence
    from fadtk_amd.model_loader import get_all_models
    from fadtk_amd.sinkhorn import INDIV_CSV_HEADER
    rng = np.random.default_rng(3)
    base, evl = tmp_path / "base", tmp_path / "evl"
    for d in (base, evl):
        (d / "embeddings" / "vggish").mkdir(parents=True)
    for i in range(4):
        (base / f"b{i}.wav").write_bytes(b"")                   # the audio itself is never read: every file has its cache
        np.save(base / "embeddings" / "vggish" / f"b{i}.npy", rng.standard_normal((40 + i, 128)).astype(np.float32))
    songs = {"near": rng.standard_normal((25, 128)), "far": rng.standard_normal((31, 128)) + 1.0, "one": rng.standard_normal((1, 128))}
    for name, e in songs.items():
        (evl / f"{name}.wav").write_bytes(b"")
        np.save(evl / "embeddings" / "vggish" / f"{name}.npy", e.astype(np.float32))
    (evl / "wide.wav").write_bytes(b"")                         # dropped with a log line: wrong D
    np.save(evl / "embeddings" / "vggish" / "wide.npy", np.zeros((4, 64), np.float32))
    ml = {m.name: m for m in get_all_models()}["vggish"]
    sd = SinkhornDivergence(ml, audio_load_worker=2, iterations=20)
    out = sd.score_individual(base, evl, tmp_path / "indiv.csv")
    lines = out.read_text().splitlines()
    assert lines[0] + "\n" == INDIV_CSV_HEADER and len(lines) == 4
    rows = {line.split(",")[0].rsplit("/", 1)[-1]: line.split(",")[1:] for line in lines[1:]}
    assert {k: int(v[0]) for k, v in rows.items()} == {"near.wav": 25, "far.wav": 31, "one.wav": 1}
    shares = [float(line.split(",")[3]) for line in lines[1:]]
    assert shares == sorted(shares, reverse=True) and lines[1].split(",")[0].endswith("far.wav")
    # the baseline's rows in the order the loader reads its directory, so that the two calls see the same bits
    x = np.concatenate([np.load(base / "embeddings" / "vggish" / (f.stem + ".npy")) for f in base.glob("*.*")])
    order = [p.stem for p in sorted(evl.glob("*.*")) if p.stem != "wide"]
    y = np.concatenate([songs[k].astype(np.float32) for k in order])
    whole = calc_sinkhorn_divergence(x, y, iterations=20, potentials=True)
    m = len(y)
    assert abs(sum(int(v[0]) * float(v[1]) for v in rows.values()) / m - whole["pot_y"].mean()) <= 1e-12 * abs(whole["ot_xy"])
    assert abs(sum(shares) - whole["pot_y"].mean()) <= 1e-12 * abs(whole["ot_xy"])
    at = 0
    for k in order:                                            # every file's mean is the mean of G over its rows, from one call
        assert abs(float(rows[k + ".wav"][1]) - whole["pot_y"][at:at + len(songs[k])].mean()) <= 1e-12 * abs(whole["ot_xy"])
        at += len(songs[k])
    with caplog.at_level(logging.INFO, logger="fadtk_amd"):
        assert sd.score_individual(base, evl, tmp_path / "indiv.csv") == out              # an existing CSV is left as it is
    (evl / "wide.wav").unlink()
    res = sd.score(base, evl)
    assert res["n"] == len(x) and res["m"] == m                # the directory's own file order: another order of the same rows
    assert abs(res["divergence"] - whole["divergence"]) <= TOL_U * SR.unit(x, y, whole["epsilon"])


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(300, 200, 37, "fp32")
    res = _capi.FadSinkhornResult()
    res.divergence = -5.0

    def call(n=300, m=200, d=37, ld=37, dt=_capi.FAD_F32, eps=1.0, it=10, out=C.byref(res), xp=x.ctypes.data, yp=y.ctypes.data):
        return lib.fad_sinkhorn(xp, n, ld, yp, m, ld, d, dt, 0, eps, it, out, None, 0, None)
    assert call() == 0 and res.divergence >= 0 and res.n == 300 and res.m == 200 and res.iterations == 10 and res.epsilon == 1.0
    res.divergence = -5.0
    assert call(dt=_capi.FAD_F64) == INVALID and b"cast" in lib.fad_last_error()
    assert call(dt=9) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID
    assert call(d=37, ld=36) == INVALID
    assert call(it=0) == INVALID and call(it=100001) == INVALID and call(it=-1) == INVALID
    assert call(eps=float("nan")) == INVALID and call(eps=float("inf")) == INVALID
    assert call(eps=1e-60) == INVALID and call(eps=1e60) == INVALID                       # log2(e) / eps outside float32
    assert call(out=None) == INVALID
    assert call(xp=None) == INVALID and call(yp=None) == INVALID
    assert call(n=0) == TOO_FEW and call(m=0) == TOO_FEW and call(n=-1) == TOO_FEW
    assert call(n=1, eps=0.0) == TOO_FEW                                                   # the default epsilon needs a median
    assert call(n=1, m=1) == 0                                                             # with an epsilon one row each is enough
    same = np.ones((5, 37), np.float32)
    res.divergence = -5.0
    assert call(n=5, eps=0.0, xp=same.ctypes.data) == INVALID and b"identical" in lib.fad_last_error()      # a median of 0
    assert call(n=5, eps=-1.0, xp=same.ctypes.data) == INVALID
    assert res.divergence == -5.0
    bf = np.zeros((4, 8), np.float64)
    from fadtk_amd import hip
    with pytest.raises(ValueError, match="cast"):
        hip.sinkhorn(bf, bf, epsilon=1.0)
