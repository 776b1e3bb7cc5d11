"""fad_sinkhorn (csrc/kad.hip) where tests/test_gpu_sinkhorn.py does not go: several row blocks per unit, rows far from
the origin, separated sets, depth up to the limit, thin shapes, special rows and scales by powers of two.

Errors are counted in the same unit as there, U = 2^-24 (max |x_i|^2 + max |y_j|^2) + 2^-24 eps log(max(n, m)).  The bounds:
  (a) the large case: TOL_U of test_gpu_sinkhorn.py -- the same distribution at a smaller D than the cases it was set on.  A lost or
      doubled tile in a column of 93 blocks moves a potential by about eps ln(93 / 92), thousands of U: the bound is not what makes it
      sharp;
  (b) - (e): bound_U = 4 x (the worst ratio of sinkhorn_chain32 against float64 ON THAT CASE AND RUN) + 1, computed here on the CPU.
      sinkhorn_chain32 emulates the documented float32 arithmetic (the rounding of h + p, one rounding per MFMA k step, the float32
      exponent and sums); the factor 4 is the margin the project gives its float32 emulations (MEAN_RTOL + 4 A kappa in the KAD
      conditioning tests) and covers the summation order the emulation does not reproduce; the + 1 U is one rounding at the scale U was
      defined for.  The marginal errors keep _marginal_tol's form with this bound in place of TOL_U;
  (f) powers of two: bit for bit, no bound.
No bound is taken from the GPU's output.  Every run prints a [sinkhorn-edge] line with the GPU's worst ratio beside the emulated one
(profiles/sinkhorn_edges_err.txt holds those of one full run on an MI355X).  Every case uses device rows, one operand with a row pitch
> D, and potentials=True.
"""
import functools

import numpy as np
import pytest

import kad_conditioning_reference as KR
import sinkhorn_reference as SR
from test_gpu_sinkhorn import TOL_U, _dev, _same_bits

pytestmark = pytest.mark.gpu
MARGINALS = ("marginal_error", "marginal_error_xx", "marginal_error_yy")
OFFSET_RUNS = ((30, 0.25), (2, 0.02), (2, 1.0))                  # (L, blur factor)
DEPTH_RUNS = ((2, 0.02), (10, 0.25))
DEPTH_CASES = ((129, 127, 512, "fp16"), (130, 129, 1280, "bf16"), (129, 127, 2047, "fp32"))
BIG = (11800, 11700, 16)                                        # 93 x 92 blocks: two row blocks per unit, a last range of one


# --------------------------------------------------------------------------------------------------------------- cases
# A case is a hashable spec; its rows, median, float64 reference and emulated ratio are each computed once.
@functools.lru_cache(maxsize=None)
def _rows(spec):
    kind = spec[0]
    if kind == "edge":                                          # ("edge", n, m, d, dt, off, sep)
        return SR.edge_rows(*spec[1:])
    dt = spec[1]
    if kind == "translated":                                    # y = x + 2 on a grid of 2^-3, |v| <= 10: exact in every dtype
        x, _ = KR.pow2_rows(257, 257, 64, seed=11)
        y = x + np.float32(2.0)
        assert np.array_equal(SR.round_to(x, dt), x) and np.array_equal(SR.round_to(y, dt), y) and np.array_equal(y - np.float32(2.0), x)
    else:                                                       # "special": an all-zero row; one row three times in x and once in y
        assert kind == "special"
        x, y = (a.copy() for a in SR.rows(257, 130, 64, dt))
        x[77] = 0.0
        x[130] = x[256] = x[3]
        y[129] = x[3]
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _median(spec):
    """of x; of y where x is a single row, which has none"""
    x, y = _rows(spec)
    return SR.median_distance(x if len(x) > 1 else y)


@functools.lru_cache(maxsize=None)
def _reference(spec, factor, L):
    x, y = _rows(spec)
    return SR.sinkhorn(x, y, (factor * _median(spec)) ** 2, L)


@functools.lru_cache(maxsize=None)
def _emulated(spec, factor, L):
    """the worst ratio of the float32 emulation against float64 on this case and run, over what _run compares"""
    x, y = _rows(spec)
    want = _reference(spec, factor, L)
    emu = SR.sinkhorn_chain32(x, y, want["epsilon"], L, spec[4] if spec[0] == "edge" else spec[1])
    return max(SR.ratios(emu, want, SR.unit(x, y, want["epsilon"])).values())


def _marginal_tol(want, bound_u, U, eps):
    """test_gpu_sinkhorn._marginal_tol with the case's bound: |d/dt |e^t - 1|| = e^t <= 1 + |e^t - 1|, t carries two potentials"""
    return float(np.expm1(min(2 * bound_u * U / eps, 50.0))) * (1.0 + want)


def _compare(got, want, x, y, bound_u, emulated, tag):
    eps = want["epsilon"]
    U = SR.unit(x, y, eps)
    for k in SR.POTS + SR.TERMS + MARGINALS:
        assert np.all(np.isfinite(got[k])), (tag, k)
    r = SR.ratios(got, want, U)
    worst = max(r.values())
    emu = "n/a" if emulated is None else f"{emulated:.3f}"
    print(f"[sinkhorn-edge] {tag}: U {U:.2e} gpu {worst:.3f} emulated {emu} bound {bound_u:.2f} | " + " ".join(f"{k} {v:.3f}" for k, v in r.items())
          + f" | marginal {got['marginal_error']:.3e} (ref {want['marginal_error']:.3e})")
    assert abs(got["epsilon"] - eps) <= 1e-15 * eps
    assert worst <= bound_u, (tag, r)
    for k in MARGINALS:
        assert abs(got[k] - want[k]) <= _marginal_tol(want[k], bound_u, U, eps), (tag, k, got[k], want[k])
    assert abs(got["pot_x"].mean() + got["pot_y"].mean() - got["divergence"]) <= 1e-12 * max(1.0, abs(got["ot_xy"]))
    return worst


def _run(spec, dt, runs, tag, pitch_on="x"):
    """every (L, blur) of `runs` on device rows, the operand `pitch_on` with a row pitch of D + 5 -> the results"""
    from fadtk_amd import hip
    x, y = _rows(spec)
    d = x.shape[1]
    xd, yd = _dev(x, dt, d + 5 if pitch_on == "x" else None), _dev(y, dt, d + 5 if pitch_on == "y" else None)
    assert (xd if pitch_on == "x" else yd).stride(0) == d + 5
    out = []
    for L, factor in runs:
        want = _reference(spec, factor, L)
        got = hip.sinkhorn(xd, yd, epsilon=want["epsilon"], iterations=L, potentials=True)
        assert (got["n"], got["m"], got["iterations"]) == (len(x), len(y), L)
        emulated = _emulated(spec, factor, L)
        _compare(got, want, x, y, 4.0 * emulated + 1.0, emulated, f"{tag} {dt} L={L} blur={factor}")
        out.append(got)
    return out


# ------------------------------------------------------------------------------------- (a) several row blocks per unit
@functools.lru_cache(maxsize=None)
def _big_epsilons(dt):
    x, _ = SR.rows(*BIG, dt)
    med = SR.median_distance(x[:2000])
    return tuple((f * med) ** 2 for f in (0.25, 0.02))


@pytest.mark.parametrize("dt", ("fp16", "fp32"))
def test_several_row_blocks_per_unit(monkeypatch, dt):
    """n = 11 800, m = 11 700, D = 16: 93 x 92 blocks, so cross_rows_per_unit gives rr = 2 in both directions of all three problems,
    with a last range of a single block where 93 blocks are reduced (test_sinkhorn_host.py proves the plan).  A lane's (M, S) is
    carried from one tile into the next, the slot row of a unit is u / TJ for ranges of two blocks.  Against the blocked float64
    reference on the GPU; then (fp16) the same call cut into several launches changes no bit."""
    import torch
    from fadtk_amd import hip
    n, m, d = BIG
    L = 2
    assert SR.cross_plan(n, m)[2] == 2 and SR.cross_plan(m, n)[2] == 2 and SR.cross_plan(n, n)[2] == 2 and SR.cross_plan(m, m)[2] == 2
    x, y = SR.rows(n, m, d, dt)
    xd, yd = _dev(x, dt), _dev(y, dt, d + 8)
    assert yd.stride(0) == d + 8
    monkeypatch.delenv("FAD_KAD_LAUNCH_BUDGET", raising=False)
    whole = None
    for factor, eps in zip((0.25, 0.02), _big_epsilons(dt)):
        got = hip.sinkhorn(xd, yd, epsilon=eps, iterations=L, potentials=True)
        assert hip.kad_last_plan()["max_launches"] == 1
        want = SR.sinkhorn_blocked(x, y, eps, L, "cuda")
        torch.cuda.synchronize()
        _compare(got, want, x, y, TOL_U, None, f"{n}x{m}x{d} {dt} L={L} blur={factor} rr=2")
        whole = whole or got
    if dt != "fp16":
        return
    monkeypatch.setenv("FAD_KAD_LAUNCH_BUDGET", "200000")                              # some hundreds of tiles a launch, rr stays 2
    cut = hip.sinkhorn(xd, yd, epsilon=_big_epsilons(dt)[0], iterations=L, potentials=True)
    plan = hip.kad_last_plan()
    monkeypatch.delenv("FAD_KAD_LAUNCH_BUDGET")
    assert plan["max_launches"] >= 2 and plan["passes"] == 6, plan
    _same_bits(whole, cut)


# ------------------------------------------------------------------------------------------ (b) far from the origin
@pytest.mark.parametrize("off", (4, 16))
@pytest.mark.parametrize("dt", SR.DTYPES)
def test_rows_far_from_the_origin(dt, off):
    """h = -|x|^2 / 2 is about -D off^2 / 2 (-16 000 at off = 16) and the potential is added to it in float32 at every half-step"""
    _run(("edge", 129, 127, 128, dt, float(off), 0.0), dt, OFFSET_RUNS, f"129x127x128 off={off}")


# --------------------------------------------------------------------------------------------------- (c) separated sets
@pytest.mark.parametrize("dt", SR.DTYPES)
def test_separated_sets(dt):
    """y moved by 2 in every coordinate: no overlap, f and g are of the size of C (256 and more)"""
    _run(("edge", 129, 127, 128, dt, 0.0, 2.0), dt, OFFSET_RUNS + ((2, 1000.0),), "129x127x128 sep=2", pitch_on="y")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_translated_copy(dt):
    """y = x + 2 exactly: the two self problems are one problem, so OT(x, x) = OT(y, y) in exact arithmetic; on the GPU y's rows are
    further from the origin than x's, so the two differ by what float32 costs, within the case's bound"""
    spec = ("translated", dt)
    x, y = _rows(spec)
    for (L, factor), got in zip(OFFSET_RUNS, _run(spec, dt, OFFSET_RUNS, "257x257x64 y=x+2")):
        want = _reference(spec, factor, L)
        assert abs(want["ot_xx"] - want["ot_yy"]) <= 1e-12 * abs(want["ot_xx"])
        bound_u = 4.0 * _emulated(spec, factor, L) + 1.0
        assert abs(got["ot_xx"] - got["ot_yy"]) <= bound_u * SR.unit(x, y, want["epsilon"]), (dt, L, factor)


# ---------------------------------------------------------------------------------------------------------- (d) depth
@pytest.mark.parametrize("case", DEPTH_CASES, ids=lambda c: "x".join(map(str, c[:3])) + "-" + c[3])
def test_depth(case):
    """up to D = 2047 (the entry's limit is 2048; a ragged k tail above one chunk): 1024 float32 MFMA k steps per pair at fp32, and at
    the smallest blur one pair's accumulation error reaches a potential undamped"""
    n, m, d, dt = case
    _run(("edge", n, m, d, dt, 0.0, 0.0), dt, DEPTH_RUNS, f"{n}x{m}x{d}", pitch_on="y")


# ----------------------------------------------------------------------------------- (e) thin shapes and special rows
@pytest.mark.parametrize("dt", ("fp16", "fp32"))
@pytest.mark.parametrize("shape", ((1, 300, 37), (300, 1, 37)), ids=lambda s: "x".join(map(str, s)))
def test_one_row_against_many(shape, dt):
    """127 of a tile's 128 rows are padding on one side, a single column on the other; eps from the 300-row set's median"""
    n, m, d = shape
    _run(("edge", n, m, d, dt, 0.0, 0.0), dt, DEPTH_RUNS, f"{n}x{m}x{d}", pitch_on="x" if n > 1 else "y")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_zero_row_and_repeated_rows(dt):
    """an all-zero row (h = 0) and a row three times in x and once in y (C = 0 off the diagonal, equal potentials)"""
    got = _run(("special", dt), dt, DEPTH_RUNS, "257x130x64 special")[0]
    assert got["f"][3] == got["f"][130] == got["f"][256] and got["pot_x"][3] == got["pot_x"][130] == got["pot_x"][256]


# -------------------------------------------------------------------------------------------------- (f) powers of two
@functools.lru_cache(maxsize=None)
def _pow2_reference(dt):
    """the unscaled rows (the same values in every dtype): float64, and the emulated worst ratio for rows of dtype dt"""
    x, y = KR.pow2_rows(129, 127, 64, seed=5)
    eps = (0.25 * SR.median_distance(x)) ** 2
    want = SR.sinkhorn(x, y, eps, 3)
    return want, max(SR.ratios(SR.sinkhorn_chain32(x, y, eps, 3, dt), want, SR.unit(x, y, eps)).values())


@pytest.mark.parametrize("dt,e", KR.SCALES, ids=lambda v: str(v))
def test_rows_scaled_by_a_power_of_two(dt, e):
    """Rows on a grid of 2^-3 scaled by 2^e, eps by 4^e: c = log2(e) / eps, v and M scale exactly, (v - M) c keeps its bits, so every
    exponential and float32 sum is the same number, and the float64 tail scales by a power of two.  Potentials, terms and S are the
    unscaled call's times 4^e and the marginal errors the unscaled call's, bit for bit."""
    from fadtk_amd import hip
    n, m, d, L = 129, 127, 64, 3
    x, y = KR.pow2_rows(n, m, d, seed=5)
    eps = (0.25 * SR.median_distance(x)) ** 2
    s, s2 = np.float32(2.0 ** e), 4.0 ** e
    xs, ys = x * s, y * s
    assert np.array_equal(SR.round_to(xs, dt), xs) and np.array_equal(SR.round_to(ys, dt), ys) and np.array_equal(xs / s, x)
    base = hip.sinkhorn(_dev(x, dt, d + 5), _dev(y, dt), epsilon=eps, iterations=L, potentials=True)
    got = hip.sinkhorn(_dev(xs, dt, d + 5), _dev(ys, dt), epsilon=eps * s2, iterations=L, potentials=True)
    want, emulated = _pow2_reference(dt)
    _compare(base, want, x, y, 4.0 * emulated + 1.0, emulated, f"{n}x{m}x{d} pow2 {dt} 2^{e} (unscaled)")
    assert got["epsilon"] == eps * s2
    for k in SR.POTS:
        assert np.array_equal(got[k], base[k] * s2), (k, np.abs(got[k] / s2 - base[k]).max())
    for k in SR.TERMS:
        assert got[k] == base[k] * s2, (k, got[k] / s2, base[k])
    for k in MARGINALS:
        assert got[k] == base[k], (k, got[k], base[k])
    print(f"[sinkhorn-edge] {n}x{m}x{d} pow2 {dt} 2^{e}: every output equals the unscaled call's times 4^{e} bit for bit")
