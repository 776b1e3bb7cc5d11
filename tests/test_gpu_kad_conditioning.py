"""The KAD family on the GPU (fad_kad, fad_kad_median_distance, fad_kad_individual, fad_kad_uncertainty, fad_kad_permutation_test,
fad_prdc, fad_nearest; csrc/kad.hip) on rows far from the origin and at extreme scales, where kappa = (|x|^2 + |y|^2) / (2 sigma^2)
is large and the float32 accumulator that starts at -(|x|^2 + |y|^2) / 2 decides the accuracy (Conditioning):

  a. integer rows at an offset of 40 and 200 (|x|^2 up to 2e6), for which every float32 quantity of the kernels is exact: the k-NN
     outputs equal the float64 reference, and the kernel means keep the tolerances of the zero-mean tests;
  b. Gaussian rows with a common offset of 4 and 16 standard deviations (kappa 9 and 130): every mean inside the float64 bracket at
     TAU and within MEAN_RTOL + 4 A kappa of float64, A from the float32 emulation of tests/kad_conditioning_reference.py;
  c. rows scaled by powers of two down to fp16 subnormals and up to 2^50: the same bits as the unscaled call;
  d. rows whose |x|^2 leaves the float32 range: refused, never answered wrongly.
The references and their own checks: tests/kad_conditioning_reference.py, tests/test_kad_conditioning_host.py."""
import numpy as np
import pytest

import kad_conditioning_reference as CR
import kad_permutation_reference as PMR
import kad_reference as R
import kad_uncertainty_reference as U
import nearest_reference as NR
import prdc_reference as PR
import test_gpu_kad as TK
import test_gpu_kad_individual as TI
import test_gpu_kad_permutation as TP
import test_gpu_kad_uncertainty as TU
import test_gpu_nearest as TN
from test_gpu_kad import MEAN_RTOL, MMD_TOL
from test_gpu_prdc import METRICS, TAU

pytestmark = pytest.mark.gpu
DTYPES = ("fp16", "bf16", "fp32")
SONG_LENGTHS = [0, 1, 2, 127, 129, 300]
assert TAU == CR.TAU and TN.TAU == TAU


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _rows(a, dt, pad=0):
    """float32 values that are exact in dt -> the rows as the library takes them: fp16 and fp32 numpy on the host, bf16 a torch tensor
    on the device; pad > 0: on the device for every dtype, inside a wider matrix (ld = D + pad)."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert np.array_equal(CR.round_to(a, dt), a), dt
    if dt != "bf16" and not pad:
        return a.astype(np.float16) if dt == "fp16" else a
    t = torch.from_numpy(a).cuda().to({"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[dt])
    if not pad:
        return t
    wide = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=t.dtype, device="cuda")
    wide[:, :a.shape[1]] = t
    return wide[:, :a.shape[1]]


def _means(got, s=None):
    """-> the four values of one set (or of song / set s) as test_gpu_kad._check takes them."""
    if s is None:
        return {k: float(got[k]) for k in CR.MEANS + ("mmd2",)}
    return {"kxx_mean": float(got["kxx_mean"]), "kyy_mean": float(got["kyy_mean"][s]), "kxy_mean": float(got["kxy_mean"][s]),
            "mmd2": float(got["mmd2"][s])}


# ------------------------------------------------------------------------------------- a. exact rows far from the origin
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,m,d,off", CR.EXACT_CASES)
def test_exact_offset_rows_prdc_and_nearest_equal_float64(n, m, d, off, dt):
    from fadtk_amd import hip
    x, y = CR.exact_sets(n, m, d, off)
    xt, yt = _rows(x, dt), _rows(y, dt)
    k = 5
    got = hip.prdc(xt, yt, k=k, details=True)
    want = PR.prdc(_f64(x), _f64(y), k)
    np.testing.assert_array_equal(got["radius2_x"].astype(np.float64), want["radius2_x"])
    np.testing.assert_array_equal(got["radius2_y"].astype(np.float64), want["radius2_y"])
    np.testing.assert_array_equal(got["balls_y"], want["balls_y"])
    np.testing.assert_array_equal(got["flags_x"], want["flags_x"])
    for key in METRICS:
        assert got[key] == want[key], (key, got[key], want[key])

    near = hip.nearest(xt, yt, k=k, authenticity=True)
    idx, d2 = NR.nearest(_f64(x), _f64(y), k)
    np.testing.assert_array_equal(near["index"], idx)
    np.testing.assert_array_equal(near["dist2"].astype(np.float64), d2)
    auth = NR.authenticity(_f64(x), _f64(y))
    np.testing.assert_array_equal(near["nn_radius2"].astype(np.float64), auth["nn_radius2"])
    assert near["copied"] == auth["copied"] and near["authenticity"] == auth["authenticity"]
    assert auth["copied_rows"][5] and d2[5, 0] == 0                           # the y row on top of an x row


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,m,d,off", CR.EXACT_CASES)
def test_exact_offset_rows_kad_family_keeps_the_zero_mean_tolerances(n, m, d, off, dt):
    """d^2 is exact, so only exp2 and the summation remain: the tolerances of the zero-mean tests, unchanged, at |x|^2 up to 2e6."""
    from fadtk_amd import hip
    x, y = CR.exact_sets(n, m, d, off)
    xt, yt, x64, y64 = _rows(x, dt), _rows(y, dt), _f64(x), _f64(y)
    label = f"exact {dt} n={n} m={m} d={d} off={off}"
    sigma = R.median_distance(x64)
    med = hip.kad_median_distance(xt)
    print(f"[kad-cond] {label}: kappa {CR.kappa(x, y, sigma):.0f}; median rel {abs(med - sigma) / sigma:.2e}")
    assert med == pytest.approx(sigma, rel=1e-7)                               # only the final sqrt and mean remain

    TK._check(hip.kad(xt, yt, bandwidth=sigma), R.kad(x64, y64, sigma), label)
    TU._check(hip.kad_uncertainty(xt, [yt], bandwidth=sigma, rows=True), U.uncertainty(x64, [y64], sigma), label)

    rng = np.random.default_rng(d + off)
    songs = CR.offset_int_rows(rng, sum(SONG_LENGTHS), d, off, [(3, 4), (140, 400)])
    cuts = np.concatenate([[0], np.cumsum(SONG_LENGTHS)]).astype(np.int64)
    ind = hip.kad_individual(xt, _rows(songs, dt), cuts, bandwidth=sigma)
    kxx = TI._ref_kxx(x64, sigma)
    assert ind["kxx_mean"] == pytest.approx(kxx, rel=MEAN_RTOL) and ind["bandwidth"] == sigma
    for s, length in enumerate(SONG_LENGTHS):
        if length < 2:
            assert ind["status"][s] == TI.TOO_FEW and np.isnan(ind["mmd2"][s])
            continue
        assert ind["status"][s] == 0
        TI._check_song(ind, s, TI._ref_song(kxx, x64, _f64(songs[cuts[s]:cuts[s + 1]]), sigma), label)

    TP._check(xt, yt, x64, y64, 64, seed=n + d, label=label, bandwidth=sigma)


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_offset_rows_with_the_bandwidth_of_the_library(dt):
    from fadtk_amd import hip
    n, m, d, off = CR.EXACT_CASES[1]
    x, y = CR.exact_sets(n, m, d, off)
    xt, yt = _rows(x, dt), _rows(y, dt)
    got = hip.kad(xt, yt)
    assert got["bandwidth"] == pytest.approx(R.median_distance(_f64(x)), rel=1e-7)
    TK._check(got, R.kad(_f64(x), _f64(y), got["bandwidth"]), f"exact {dt} d={d} off={off}, the library's sigma")
    assert hip.kad_median_distance(xt) == got["bandwidth"]
    unc = hip.kad_uncertainty(xt, [yt])
    assert unc["bandwidth"] == got["bandwidth"] and unc["kxx_mean"] == pytest.approx(got["kxx_mean"], rel=MEAN_RTOL)
    ind = hip.kad_individual(xt, yt, [0, m])
    assert ind["bandwidth"] == got["bandwidth"] and ind["kxx_mean"] == got["kxx_mean"]


# ------------------------------------------------------------------------------------- b. Gaussian rows with a common offset
def _check_conditioned(got, want, bracket, tol, label):
    """Every mean and mmd2 inside the bracket; every mean within tol relative of float64, mmd2 within tol of kxx + kyy + 2 kxy."""
    err = CR.mean_errors(got, want)
    for k in CR.MEANS + ("mmd2",):
        assert CR.inside(got[k], bracket[k]), (label, k, bracket[k][0], got[k], bracket[k][1])
        assert err[k] <= tol, (label, k, err[k], tol)
    return err


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d,off", CR.GAUSS_CASES)
def test_gaussian_offset_means_within_what_float32_allows(d, off, dt):
    """fad_kad, fad_kad_uncertainty (one set) and fad_kad_individual (the set cut into songs of 1, 2, 127 and 127 rows) at
    kappa = 9 and 130.  The tolerance of every mean, of the sets and of the songs of 127 rows, is MEAN_RTOL + 4 A kappa with A from
    chain32_means over the Gaussian cases.  The song of two rows alone takes the constant of chain32 on that song: its Kyy is one
    pair, which no average helps, and the emulation itself is past the set-level tolerance there (CR.song_constants)."""
    from fadtk_amd import hip
    c = CR.gauss_case(d, off, dt)
    A, A_songs = CR.conditioning_constant(dt), CR.song_constants(dt)
    sigma, kap = c["sigma"], c["kappa"]
    pad = 8 if dt == "bf16" else 0                                             # bf16 on the device with ld > D
    xt, yt = _rows(c["x"], dt, pad), _rows(c["y"], dt, pad)
    label = f"{dt} d={d} off={off}"
    kad = _means(hip.kad(xt, yt, bandwidth=sigma))
    unc = _means(hip.kad_uncertainty(xt, [yt], bandwidth=sigma, rows=True), 0)
    ind = hip.kad_individual(xt, yt, np.array(CR.SONG_CUTS, dtype=np.int64), bandwidth=sigma)
    songs = CR.song_case(d, off, dt)

    tol = MEAN_RTOL + 4 * A * kap
    err, err_unc = CR.mean_errors(kad, c["want"]), CR.mean_errors(unc, c["want"])
    width = {k: (c["bracket"][k][1] - c["bracket"][k][0]) / c["want"][k] for k in CR.MEANS}
    song_err = [None if q is None else CR.mean_errors(_means(ind, s), q["want"]) for s, q in enumerate(songs)]
    print(f"[kad-cond] {label}: kappa {kap:.1f} tol {tol:.2e}; kad " + " ".join(f"{k}={v:.2e}" for k, v in err.items())
          + "; chain32 " + " ".join(f"{v:.2e}" for v in c["chain_err"].values())
          + "; uncertainty " + " ".join(f"{v:.2e}" for v in err_unc.values())
          + "; songs kyy/kxy/mmd2 " + " ".join("-" if e is None else f"[{e['kyy_mean']:.2e} {e['kxy_mean']:.2e} {e['mmd2']:.2e}]" for e in song_err)
          + "; bracket width " + " ".join(f"{v:.2e}" for v in width.values()))

    _check_conditioned(kad, c["want"], c["bracket"], tol, label + " kad")
    _check_conditioned(unc, c["want"], c["bracket"], tol, label + " uncertainty")
    assert ind["kxx_mean"] == kad["kxx_mean"]                                   # the same launches, slots and sum
    for s, q in enumerate(songs):
        if q is None:
            assert ind["status"][s] == TI.TOO_FEW
            continue
        assert ind["status"][s] == 0
        _check_conditioned(_means(ind, s), q["want"], q["bracket"], MEAN_RTOL + 4 * A_songs[s] * kap, f"{label} song {s}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d,off", CR.GAUSS_CASES)
def test_gaussian_offset_median(d, off, dt):
    """An order statistic moves by no more than the largest perturbation of a pair: |sigma_gpu^2 - sigma_ref^2| <= TAU max(|a|^2 + |b|^2)."""
    from fadtk_amd import hip
    c = CR.gauss_case(d, off, dt)
    got = hip.kad_median_distance(_rows(c["x"], dt, 8 if dt == "bf16" else 0))
    bound = TAU * CR.max_pair_norms(c["x"])
    print(f"[kad-cond] median {dt} d={d} off={off}: |sigma^2 - ref| = {abs(got ** 2 - c['sigma'] ** 2):.2e}, bound {bound:.2e}, "
          f"sigma rel {abs(got - c['sigma']) / c['sigma']:.2e}")
    assert abs(got ** 2 - c["sigma"] ** 2) <= bound


def _check_prdc_bracket(got, x, y, k, label):
    """_check_bracket of test_gpu_prdc.py with the cap of this offset on the width of each value's bracket."""
    br = PR.bracket(x, y, k, TAU)
    sx, sy = (x ** 2).sum(1), (y ** 2).sum(1)
    errs = []
    for a, key, sq in ((x, "x", sx), (y, "y", sy)):
        r2, nn = PR.radii2(a, k)
        err = np.abs(got[f"radius2_{key}"].astype(np.float64) - r2) / (sq + sq[nn])
        errs.append(float(err.max()))
    width = {key: br[f"{key}_hi"] - br[f"{key}_lo"] for key in METRICS}
    print(f"[kad-cond] prdc {label}: radius2 x {errs[0]:.2e} y {errs[1]:.2e}; bracket width " + " ".join(f"{key}={v:.4f}" for key, v in width.items()))
    assert max(errs) <= TAU, (label, errs)
    balls, flags = got["balls_y"], got["flags_x"]
    assert (br["balls_lo"] <= balls).all() and (balls <= br["balls_hi"]).all(), label
    rec, cov = (flags & 1).astype(bool), (flags & 2).astype(bool)
    assert (br["recalled_lo"] <= rec).all() and (rec <= br["recalled_hi"]).all(), label
    assert (br["covered_lo"] <= cov).all() and (cov <= br["covered_hi"]).all(), label
    for key in METRICS:
        assert br[f"{key}_lo"] <= got[key] <= br[f"{key}_hi"], (label, key)
        assert width[key] <= CR.PRDC_CAP, (label, key, width[key])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,m,d,k", CR.PRDC_CASES)
def test_gaussian_offset_prdc_inside_the_bracket(n, m, d, k, dt):
    from fadtk_amd import hip
    x, y = CR.prdc_gauss(n, m, d, seed=n + d)
    x, y = CR.round_to(x + np.float32(CR.PRDC_OFFSET), dt), CR.round_to(y + np.float32(CR.PRDC_OFFSET), dt)
    got = hip.prdc(_rows(x, dt, 24), _rows(y, dt, 8), k=k, details=True)          # ld > D on the device
    _check_prdc_bracket(got, _f64(x), _f64(y), k, f"{dt} n={n} m={m} D={d} k={k} off={CR.PRDC_OFFSET}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,m,d,k", CR.PRDC_CASES)
def test_gaussian_offset_nearest_inside_the_bracket(n, m, d, k, dt):
    from fadtk_amd import hip
    x, y = TN._gauss(n, m, d, seed=n + d)
    x, y = CR.round_to(x + np.float32(CR.PRDC_OFFSET), dt), CR.round_to(y + np.float32(CR.PRDC_OFFSET), dt)
    got = hip.nearest(_rows(x, dt, 24), _rows(y, dt, 8), k=k, authenticity=True)
    TN._check_bracket(got, _f64(x), _f64(y), k, f"{dt} n={n} m={m} D={d} k={k} off={CR.PRDC_OFFSET}")


# ------------------------------------------------------------------------------------- c. scale by powers of two
@pytest.mark.parametrize("dt,e", CR.SCALES)
@pytest.mark.parametrize("d", [17, 128])
def test_power_of_two_scale_gives_the_same_bits(d, dt, e):
    """Every step of the chain is exact under a power-of-two scale while no float32 quantity leaves the normal range (the host test
    asserts that it does not): h and the products scale by s^2, sigma by s, c = log2 e / sigma^2 by s^-2, and c S' is unchanged."""
    from fadtk_amd import hip
    x, y = CR.pow2_rows(CR.GAUSS_N, CR.GAUSS_M, d, seed=d)
    s = np.float32(2.0 ** e)
    base = hip.kad(_rows(x, dt), _rows(y, dt))
    got = hip.kad(_rows(x * s, dt), _rows(y * s, dt))
    label = f"scale {dt} d={d} s=2^{e}"
    print(f"[kad-cond] {label}: bandwidth {got['bandwidth']:.6e} = s * {got['bandwidth'] / 2.0 ** e:.9f} (unscaled {base['bandwidth']:.9f}); "
          + " ".join(f"{k} {got[k]!r} / {base[k]!r}" for k in CR.MEANS + ("mmd2",)))
    TK._check(got, R.kad(_f64(x) * 2.0 ** e, _f64(y) * 2.0 ** e, sigma=got["bandwidth"]), label)            # mandatory
    assert got["bandwidth"] == pytest.approx(2.0 ** e * base["bandwidth"], rel=1e-7)
    for k in CR.MEANS + ("mmd2",):
        assert got[k] == base[k], (label, k, got[k], base[k])                  # bit for bit


@pytest.mark.parametrize("d", [17, 128])
def test_fp16_subnormal_rows_prdc_and_nearest(d):
    from fadtk_amd import hip
    x, y = CR.pow2_rows(CR.GAUSS_N, CR.GAUSS_M, d, seed=d)
    s = np.float32(2.0 ** -14)
    s2 = np.float32(2.0 ** -28)
    a = hip.prdc(_rows(x, "fp16"), _rows(y, "fp16"), k=5, details=True)
    b = hip.prdc(_rows(x * s, "fp16"), _rows(y * s, "fp16"), k=5, details=True)
    assert a["radius2_x"].max() > 0
    for key in ("balls_y", "flags_x"):
        np.testing.assert_array_equal(a[key], b[key])
    for key in ("radius2_x", "radius2_y"):
        np.testing.assert_array_equal(a[key] * s2, b[key])
    for key in METRICS:
        assert a[key] == b[key], key
    a = hip.nearest(_rows(x, "fp16"), _rows(y, "fp16"), k=5, authenticity=True)
    b = hip.nearest(_rows(x * s, "fp16"), _rows(y * s, "fp16"), k=5, authenticity=True)
    np.testing.assert_array_equal(a["index"], b["index"])
    np.testing.assert_array_equal(a["dist2"] * s2, b["dist2"])
    np.testing.assert_array_equal(a["nn_radius2"] * s2, b["nn_radius2"])
    assert a["copied"] == b["copied"] and a["authenticity"] == b["authenticity"]


# ------------------------------------------------------------------------------------- d. past the range: refuse
def _labels(n, m, count=4):
    from fadtk_amd import hip
    return hip.pack_labels(PMR.random_labellings(n, m, count, np.random.default_rng(0)))


def _entry_points(x, y, bandwidth):
    """(name, call) of the seven entry points on the sets x and y; the four that take a bandwidth come first."""
    from fadtk_amd import hip
    m = y.shape[0]
    return [("kad", lambda: _means(hip.kad(x, y, bandwidth=bandwidth))),
            ("kad_individual", lambda: _means(hip.kad_individual(x, y, [0, m], bandwidth=bandwidth), 0)),
            ("kad_uncertainty", lambda: _means(hip.kad_uncertainty(x, [y], bandwidth=bandwidth), 0)),
            ("kad_permutation_test", lambda: _means(hip.kad_permutation_test(x, y, _labels(x.shape[0], m), bandwidth=bandwidth))),
            ("kad_median_distance", lambda: hip.kad_median_distance(x)),
            ("prdc", lambda: hip.prdc(x, y, k=5)),
            ("nearest", lambda: hip.nearest(x, y, k=5))]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_rows_whose_norm_overflows_float32_are_refused(dt):
    from fadtk_amd import hip
    x, y = CR.pow2_rows(CR.GAUSS_N, CR.GAUSS_M, 17, seed=17)
    s = np.float32(2.0 ** CR.OVERFLOW_EXP)
    xt, yt = _rows(x * s, dt), _rows(y * s, dt)
    for name, call in _entry_points(xt, yt, None):
        with pytest.raises(ValueError, match="NaN/Inf norm"):                  # FAD_ERR_NOT_FINITE
            call()
    got = hip.kad(_rows(x, dt), _rows(y, dt))                                  # the library answers a normal call afterwards
    TK._check(got, R.kad(_f64(x), _f64(y), got["bandwidth"]), f"after the refusals, {dt}")


def test_rows_whose_norm_underflows_float32_are_refused_or_right():
    """fp32 rows at 2^-80: every |x|^2 is 0 in float32.  Without a bandwidth the median is 0 and the call raises; with the scaled
    float64 bandwidth the call raises (c = log2 e / sigma^2 is past float32) or agrees with float64 -- never mmd2 = 0 from k = 1."""
    x, y = CR.pow2_rows(CR.GAUSS_N, CR.GAUSS_M, 17, seed=17)
    e = CR.UNDERFLOW_EXP
    xs, ys = _rows(x * np.float32(2.0 ** e), "fp32"), _rows(y * np.float32(2.0 ** e), "fp32")
    for name, call in _entry_points(xs, ys, None)[:4]:
        with pytest.raises((ValueError, RuntimeError), match="must be > 0"):
            call()
    sigma = R.median_distance(_f64(x)) * 2.0 ** e
    want = R.kad(_f64(x) * 2.0 ** e, _f64(y) * 2.0 ** e, sigma)
    assert want["mmd2"] > 1e-3                                                 # a silent k = 1 everywhere would give 0
    for name, call in _entry_points(xs, ys, sigma)[:4]:
        try:
            got = call()
        except (ValueError, RuntimeError) as err:
            print(f"[kad-cond] underflow {name}: refused ({err})")
            continue
        if name == "kad_permutation_test":                                     # its statistic: the tolerance of its own tests
            assert abs(got["mmd2"] - want["mmd2"]) <= MMD_TOL * (want["kxx_mean"] + want["kyy_mean"] + 2 * want["kxy_mean"])
        else:
            TK._check(got, want, f"underflow {name}")
    from fadtk_amd import hip
    got = hip.kad(_rows(x, "fp32"), _rows(y, "fp32"))
    TK._check(got, R.kad(_f64(x), _f64(y), got["bandwidth"]), "after the refusals, fp32")
