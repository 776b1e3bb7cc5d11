"""The references of the KAD conditioning tests (kad_conditioning_reference.py) held to float64 on the host: the exact rows are exact
under the float32 chain, the bracket holds the float64 means and the chain's, the caps and tolerances that the GPU tests use follow from
the reference alone, and the scales of the power-of-two cases keep every float32 quantity normal.  No GPU needed."""
import numpy as np
import pytest
from scipy.spatial.distance import cdist, pdist

import kad_conditioning_reference as CR
import prdc_reference as PR
from test_gpu_kad import MEAN_RTOL          # the bound on a mean at kappa = 1 (importing that module needs no GPU)

DTYPES = ("fp16", "bf16", "fp32")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ exact rows
@pytest.mark.parametrize("n,m,d,off", CR.EXACT_CASES)
def test_exact_rows_are_exact_under_the_float32_chain(n, m, d, off):
    assert CR.exact_condition(d, off)
    x, y = CR.exact_sets(n, m, d, off)
    assert x.min() >= off - 3 and x.max() <= off + 3 and np.array_equal(x, np.round(x))
    for dt in DTYPES:                                             # the values themselves: exact in every dtype
        assert np.array_equal(CR.round_to(x, dt), x) and np.array_equal(CR.round_to(y, dt), y), dt
    assert np.array_equal(x[0], x[1]) and np.array_equal(y[5], x[4])            # duplicates, and a y row on top of an x row
    for a in (x, y):                                              # h = -|row|^2 / 2 in the pack kernel's order
        assert np.array_equal(CR.h32(a).astype(np.float64), -0.5 * (_f64(a) ** 2).sum(1))
    for step in sorted(set(CR.STEP.values())):
        for a, b in ((x, x), (y, y), (x, y)):
            assert np.array_equal(CR.chain32_d2(a, b, step), cdist(_f64(a), _f64(b), "sqeuclidean")), (step, a.shape, b.shape)
    norms = (_f64(x) ** 2).sum(1)
    print(f"[kad-cond-host] exact n={n} m={m} d={d} off={off}: |x|^2 in [{norms.min():.0f}, {norms.max():.0f}], d^2 exact for K = 16 and 2")


def test_exactness_condition_refuses_rows_that_are_not_exact():
    assert not CR.exact_condition(2048, 43) and not CR.exact_condition(17, 254) and CR.exact_condition(17, 253)
    with pytest.raises(AssertionError):
        CR.offset_int_rows(np.random.default_rng(0), 4, 2048, 43, [])
    # outside the condition the chain does round: Gaussian rows at an offset are not exact
    x, y = CR.gauss_sets(128, 16, "fp16")
    assert not np.array_equal(CR.chain32_d2(x, y, 16), cdist(_f64(x), _f64(y), "sqeuclidean"))


def test_round_to_bfloat16_is_round_to_nearest_even():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 + 3 * 2.0 ** -8, 203.0, 256.0, 257.0, -0.1], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, 203.0, 256.0, 256.0, -0.10009765625], dtype=np.float32)
    assert np.array_equal(CR.round_to(a, "bf16"), want)
    torch = pytest.importorskip("torch")
    r = np.random.default_rng(1).standard_normal(4096).astype(np.float32) * 37
    assert np.array_equal(CR.round_to(r, "bf16"), torch.from_numpy(r).bfloat16().float().numpy())


# ------------------------------------------------------------------------------------------------------- Gaussian rows
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d,off", CR.GAUSS_CASES)
def test_bracket_holds_float64_and_the_float32_chain(d, off, dt):
    c = CR.gauss_case(d, off, dt)
    x, y, sigma = c["x"], c["y"], c["sigma"]
    assert np.array_equal(CR.round_to(x, dt), x)
    zero = CR.bracket_means(x, y, sigma, 0.0)                     # tau = 0: the float64 means themselves
    for k in CR.MEANS + ("mmd2",):
        lo, hi = c["bracket"][k]
        assert lo < c["want"][k] < hi, (k, lo, c["want"][k], hi)
        assert lo < c["chain"][k] < hi, (k, lo, c["chain"][k], hi)
        assert zero[k][0] == pytest.approx(c["want"][k], rel=1e-14) and zero[k][1] == pytest.approx(c["want"][k], rel=1e-14), k
    songs = CR.song_case(d, off, dt)
    assert [q is None for q in songs] == [True, False, False, False]             # the song of one row has no Kyy
    for q in songs[1:]:
        for k in ("kyy_mean", "kxy_mean", "mmd2"):
            assert q["bracket"][k][0] <= q["want"][k] <= q["bracket"][k][1], k
    # the median: an order statistic moves by no more than the largest perturbation of a pair
    iu = np.triu_indices(x.shape[0], 1)
    med32 = float(np.median(np.maximum(CR.chain32_d2(x, x, CR.STEP[dt])[iu], 0.0)))
    assert abs(med32 - sigma ** 2) <= CR.TAU * CR.max_pair_norms(x)
    assert sigma == pytest.approx(float(np.median(pdist(_f64(x)))), rel=1e-15)
    width = {k: (c["bracket"][k][1] - c["bracket"][k][0]) / c["want"][k] for k in CR.MEANS}
    print(f"[kad-cond-host] {dt} d={d} off={off}: kappa {c['kappa']:.1f}; chain32 "
          + " ".join(f"{k}={v:.2e}" for k, v in c["chain_err"].items()) + "; bracket width " + " ".join(f"{v:.2e}" for v in width.values()))


@pytest.mark.parametrize("dt", DTYPES)
def test_conditioning_constant_and_tolerances(dt):
    """A per dtype, from the reference alone: at most two units of 2^-24 per unit of kappa (one rounding of an accumulator of size
    (|x|^2 + |y|^2) / 2 moves the exponent of k by at most 2^-24 kappa, and the means average over pairs and steps).  The tolerance
    MEAN_RTOL + 4 A kappa that the GPU tests hold lies well inside the bracket, so it is the tighter of the two checks at every case;
    and the emulation of every song with an averaged Kyy meets it with the set-level A, while the song of two rows does not."""
    A = CR.conditioning_constant(dt)
    A_songs = CR.song_constants(dt)
    rows = [CR.SONG_CUTS[s + 1] - CR.SONG_CUTS[s] for s in range(len(CR.SONG_CUTS) - 1)]
    print(f"[kad-cond-host] {dt}: A = {A:.3e}; chain32 per song of {rows} rows: "
          + " ".join("-" if r < 2 else f"{CR.song_chain_constant(dt, s):.3e}" for s, r in enumerate(rows)))
    assert 0 < A <= 2 * 2.0 ** -24, A
    assert A_songs[0] is None and A_songs[2] == A and A_songs[3] == A and A_songs[1] == CR.song_chain_constant(dt, 1)
    worst_pair = 0.0
    for d, off in CR.GAUSS_CASES:
        c = CR.gauss_case(d, off, dt)
        tol = MEAN_RTOL + 4 * A * c["kappa"]
        for k in CR.MEANS:
            half = (c["bracket"][k][1] - c["bracket"][k][0]) / (2 * c["want"][k])
            assert tol < half / 4, (d, off, k, tol, half)
        for s, q in enumerate(CR.song_case(d, off, dt)):
            if q is None:
                continue
            err = max(q["chain_err"]["kyy_mean"], q["chain_err"]["kxy_mean"])
            if rows[s] > 2:
                assert err <= tol and q["chain_err"]["mmd2"] <= tol, (d, off, s, err, tol)
            else:
                worst_pair = max(worst_pair, err / tol)
                half = (q["bracket"]["kyy_mean"][1] - q["bracket"]["kyy_mean"][0]) / (2 * q["want"]["kyy_mean"])
                assert MEAN_RTOL + 4 * A_songs[s] * c["kappa"] < half, (d, off, s)
    assert worst_pair > 1, worst_pair                # one pair: the emulation itself is past the set-level tolerance


# ------------------------------------------------------------------------------------------------- PRDC bracket at an offset
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,m,d,k", CR.PRDC_CASES)
def test_prdc_bracket_width_at_the_offset(n, m, d, k, dt):
    x, y = CR.prdc_gauss(n, m, d, seed=n + d)
    x, y = CR.round_to(x + np.float32(CR.PRDC_OFFSET), dt), CR.round_to(y + np.float32(CR.PRDC_OFFSET), dt)
    br = PR.bracket(_f64(x), _f64(y), k, CR.TAU)
    width = {key: br[f"{key}_hi"] - br[f"{key}_lo"] for key in ("precision", "recall", "density", "coverage")}
    print(f"[kad-cond-host] prdc {dt} n={n} m={m} d={d} k={k} off={CR.PRDC_OFFSET}: bracket width "
          + " ".join(f"{key}={v:.4f}" for key, v in width.items()))
    assert max(width.values()) <= CR.PRDC_CAP, width
    assert min(width.values()) >= 0


# ------------------------------------------------------------------------------------------------------ powers of two
@pytest.mark.parametrize("dt,e", CR.SCALES)
@pytest.mark.parametrize("d", [17, 128])
def test_scaled_rows_stay_exact_and_normal_in_float32(d, dt, e):
    x, y = CR.pow2_rows(CR.GAUSS_N, CR.GAUSS_M, d, seed=d)
    s = np.float32(2.0 ** e)
    assert np.abs(x).max() <= 8 and np.array_equal(x * 8, np.round(x * 8))
    for a in (x, y):
        assert np.array_equal(CR.round_to(a, dt), a) and np.array_equal(CR.round_to(a * s, dt), a * s)          # exact before and after
        if dt == "fp16":
            assert np.array_equal((a * s).astype(np.float16).astype(np.float64), _f64(a) * 2.0 ** e)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    nz = np.abs(np.concatenate([x, y]))[np.concatenate([x, y]) != 0]
    assert (nz.min() * 2.0 ** e) ** 2 >= tiny                     # the smallest product of two elements
    norms = (_f64(np.concatenate([x, y])) ** 2).sum(1) * 4.0 ** e
    assert norms.max() * 2 <= huge and norms.min() >= tiny
    sigma = float(np.median(pdist(_f64(x)))) * 2.0 ** e
    c = 1.4426950408889634 / sigma ** 2
    assert tiny <= c <= huge and tiny <= sigma ** 2 <= huge
    if dt == "fp16" and e < 0:                                    # what the case is for: most elements are fp16 subnormals
        sub = np.abs(_f64(x) * 2.0 ** e) < 2.0 ** -14
        assert sub.mean() > 0.6


def test_rows_past_the_float32_range():
    x, _ = CR.pow2_rows(CR.GAUSS_N, CR.GAUSS_M, 17, seed=17)
    big = (x * np.float32(2.0 ** CR.OVERFLOW_EXP)).astype(np.float32)
    assert np.isfinite(big).all() and np.array_equal(CR.round_to(big, "bf16"), big)
    with np.errstate(over="ignore"):
        assert np.isinf((big * big).sum(1, dtype=np.float32)).all()           # every |x|^2 overflows float32
    small = (x * np.float32(2.0 ** CR.UNDERFLOW_EXP)).astype(np.float32)
    assert np.array_equal(small.astype(np.float64), _f64(x) * 2.0 ** CR.UNDERFLOW_EXP)
    assert ((small * small).sum(1, dtype=np.float32) == 0).all()               # every |x|^2 underflows to 0
