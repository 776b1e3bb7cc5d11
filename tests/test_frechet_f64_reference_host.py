"""The host reference of the float64 square-root iteration (tests/frechet_f64_reference.py) against itself and the oracle: the
emulation reaches the eigenvalue value on every case the GPU tests use, the oracle's distance agrees, every iteration count the
GPU tests assert has its margin (or the case is marked "count may differ by one"), and the negative-eigenvalue family takes the
exits its eigenvalues call for (runaway guard, non-finite at iterations 24, 18 and 8, the eps that rescues each).  No GPU.  `pytest -s` prints the tolerance table of DESIGN.md 4.3.1."""
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("frechet_f64_reference", Path(__file__).resolve().parent / "frechet_f64_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

EPS = 2.0 ** -52
MARGIN_ROOM = 10.0          # the branch of the scale rule: alternatives this many bounds away


def _value_bound(d, deficient, C1, C2, x):
    """What the iteration itself may be off by.  Full rank: it closes with ||I - Z Y||_F (or its bound) <= 1e-13 d, and with
    y_i = sqrt(a_i (1 - e_i)) that is a relative error of at most 1e-13 d; rounding adds at most d eps per product over <= 64 of them.
    Rank-deficient: each of the d - rank null eigenvalues of C1 C2 is perturbed to at most d eps lambda_max by the rounding of the
    product, and contributes the square root of that."""
    b = (1e-13 * d + 64 * d * EPS) * x
    if deficient:
        A = C1 @ C2
        null = d - max(1, d // 2 - 1)
        b += null * math.sqrt(d * EPS * R.scale_rule(A)["u"])
    return b


@pytest.mark.parametrize("d,deficient,scale", R.VALUE_CASES)
def test_emulation_reaches_the_eigenvalue_value_and_the_oracle(d, deficient, scale):
    from oracle.fad_oracle import frechet_distance
    mu1, C1, mu2, C2 = R.value_case(d, deficient, scale)
    e, x, bound = R.value_reference(d, deficient, scale)
    print(f"d={d} deficient={deficient} scale={scale:g}: rule {e['rule']} iters {e['iters']} |emulation - exact| / exact "
          f"{abs(e['tr_sqrt'] - x) / x:.2e}  device bound / exact {bound / x:.2e}  firm {e['firm']}")
    assert e["conv"] == (2 if deficient else 1) and not e["nonfinite"]
    own = _value_bound(d, deficient, C1, C2, x)
    assert abs(e["tr_sqrt"] - x) <= own
    assert bound <= 16 * own                                    # the GPU tests' tolerance is never wider than 16x the derived one
    if d <= 200:                                                # (the oracle's general eigensolver at 512: seconds, and nothing new)
        try:
            want = frechet_distance(mu1, C1, mu2, C2, run_sqrtm=False)
        except ValueError:
            # fad.py:102-106 refuses a root whose diagonal has an imaginary part above 1e-3 ABSOLUTE: roundoff-negative null
            # eigenvalues of a rank-deficient product at scale 1e6.  Only there; the eigenvalue value above stands.
            assert deficient and scale > 1.0
            return
        got = R.mean_term(mu1, mu2) + np.trace(C1) + np.trace(C2) - 2 * e["tr_sqrt"]
        assert abs(got - want) <= 4 * own + 8 * EPS * (np.trace(C1) + np.trace(C2))


@pytest.mark.parametrize("d,deficient,scale", R.VALUE_CASES)
def test_every_asserted_count_has_its_margin(d, deficient, scale):
    e, _, _ = R.value_reference(d, deficient, scale)
    print(f"d={d} deficient={deficient} scale={scale:g}: {e['rule']} after {e['iters']}; per-check margins: increments {e['margin']:.3g}, "
          f"residual {e['margin_res']:.3g}; firm {e['firm']}, per check {e['firm_per_check']}")
    assert e["firm"] or (d, deficient) in R.COUNT_MAY_DIFFER_BY_ONE, (e["rule"], e["iters"], e["margin"], e["margin_res"])
    _, C1, _, C2 = R.value_case(d, deficient, scale)
    _, room = R.scale_bound(C1, C2)
    # (d = 1: tr(A^2) / tr A and U are one product and one quotient each, the same IEEE operations on both sides, so the branch
    #  cannot differ although the two candidates coincide)
    assert room > MARGIN_ROOM or d == 1


def test_marks_are_not_stale():
    """Every marked (d, rank-deficient) really has a scale at which the emulation is not firm."""
    for d, deficient in R.COUNT_MAY_DIFFER_BY_ONE:
        scales = [s for (dd, df, s) in R.VALUE_CASES if (dd, df) == (d, deficient)]
        assert scales and any(not R.value_reference(d, deficient, s)[0]["firm"] for s in scales), (d, deficient)


@pytest.mark.parametrize("d,p,same", R.DECAY_CASES)
def test_decaying_spectra_take_the_scaled_steps(d, p, same):
    _, C1, _, C2 = R.decay_case(d, p, same)
    e = R.emulate(C1, C2)
    plain = R.emulate(C1, C2, allow_scaled=False)
    x = R.tr_sqrt_exact(C1, C2)
    assert e["scaled"] and e["choice"] == "u" and e["mu"][0] > 1.0 and 1e-5 <= e["l0"] <= 0.5
    assert e["conv"] == 1 and e["firm"] and e["iters"] < plain["iters"]
    assert abs(e["tr_sqrt"] - x) <= (1e-13 * d + 64 * d * EPS) * x
    assert R.scale_bound(C1, C2)[1] > MARGIN_ROOM


def test_limits_case():
    d, deficient, scale = R.LIMIT_CASE
    _, C1, _, C2 = R.value_case(d, deficient, scale)
    full, x, _ = R.value_reference(d, deficient, scale)
    cut = R.emulate(C1, C2, max_iter=3)
    assert (cut["conv"], cut["iters"], cut["rule"]) == (0, 3, "max_iter") and cut["firm"]
    assert abs(cut["tr_sqrt"] - x) > 0.1 * x                       # far from converged: the third iterate is a value of its own
    wide = R.emulate(C1, C2, max_iter=3, dtype=np.longdouble, c=cut["c"])
    assert abs(wide["tr_sqrt"] - cut["tr_sqrt"]) <= d * EPS * cut["tr_sqrt"]


def test_tol_case_has_the_margin_on_every_check():
    """tol = 1e-3: the residual of every check, and the bound on its successor, are 10x away from the tolerance on the side they fall
    (the closing residual sits in the window [1e-2, 1.15e-2] the reference describes), so the count is asserted exactly on the GPU."""
    d = R.TOL_CASE[0]
    _, C1, _, C2 = R.tol_case()
    early, full, x = R.emulate(C1, C2, tol=1e-3), R.emulate(C1, C2), R.tr_sqrt_exact(C1, C2)
    print(f"tol=1e-3: {early['rule']} after {early['iters']}, residuals {early['res']}, margins {early['margin']:.3g} / {early['margin_res']:.3g}; "
          f"default: {full['rule']} after {full['iters']}, margins {full['margin']:.3g} / {full['margin_res']:.3g}")
    assert early["firm"] and early["firm_per_check"] and early["margin_res"] >= R.MARGIN and early["margin"] >= R.MARGIN
    assert full["firm"] and full["firm_per_check"]
    assert (early["conv"], early["rule"], early["iters"]) == (1, "predicted", 6) and (full["conv"], full["iters"]) == (1, 8)
    assert 1e-2 <= early["res"][early["iters"] - 2] <= 1.15e-2
    assert R.scale_bound(C1, C2)[1] > MARGIN_ROOM
    assert abs(early["tr_sqrt"] - full["tr_sqrt"]) <= early["bound"] * x      # |y_i - sqrt a_i| <= sqrt a_i |e_i|, |e_i| <= ||E||_F
    assert abs(early["tr_sqrt"] - full["tr_sqrt"]) > 100 * R.tr_sqrt_bound(full["tr_sqrt"], x, d)    # and a value of its own


# eigenvalue -> (exit without retry, iteration at which it leaves the floats or None, smallest eps of (1e-6, 1e-3, 0.5) that converges)
NEGATIVE_EXITS = {-1e-12: ("runaway", None, 1e-6), -1e-9: ("runaway", None, 1e-6), -5e-7: ("nonfinite", 24, 1e-6),
                  -1e-4: ("nonfinite", 18, 1e-3), -0.3: ("nonfinite", 8, 0.5)}


@pytest.mark.parametrize("lam", R.NEGATIVE_LAMBDAS)
def test_negative_eigenvalue_family(lam):
    rule, at, first_eps = NEGATIVE_EXITS[lam]
    _, C1, _, C2 = R.negative_case(lam)
    assert np.min(np.linalg.eigvalsh(C1)) == pytest.approx(lam, rel=1e-3, abs=1e-15)
    e = R.emulate(C1, C2)
    assert e["rule"] == rule and e["firm"], (e["rule"], e["margin"])
    if at is None:
        assert e["conv"] == 2 and not e["nonfinite"]
        clamped = R.tr_sqrt_exact(C1, C2)                        # (tr_sqrt_exact clamps the negative eigenvalue of C1)
        assert abs(e["tr_sqrt"] - clamped) <= math.sqrt(33 * EPS * R.scale_rule(C1 @ C2)["u"]) + math.sqrt(-lam) * 2
    else:
        assert e["nonfinite"] and len(e["res"]) - 1 == at
    for eps in (1e-6, 1e-3, 0.5):
        _, E1, _, E2 = R.shifted_case(lam, eps)
        r = R.emulate(E1, E2)
        if eps >= first_eps:
            assert r["conv"] == 1 and abs(r["tr_sqrt"] - R.tr_sqrt_exact(E1, E2)) <= (1e-13 * 33 + 64 * 33 * EPS) * r["tr_sqrt"]
        else:
            assert r["nonfinite"]


def test_history_problems_have_their_lengths():
    for name, (iters, _) in R.HISTORY_PROBLEMS.items():
        _, C1, _, C2 = R.history_problem(name)
        e = R.emulate(C1, C2)
        assert e["iters"] == iters and e["rule"] == "predicted" and e["firm"], (name, e["iters"], e["rule"], e["margin_res"])


def test_scale_rule_takes_each_branch():
    rng = np.random.default_rng(5)
    d = 33
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    flat = (Q * np.linspace(0.9, 1.1, d)) @ Q.T
    assert R.scale_rule(flat)["choice"] == "wmean"
    decay = (Q * np.arange(1.0, d + 1) ** -2.0) @ Q.T
    assert R.scale_rule(decay)["choice"] == "u" and R.scale_rule(decay, allow_scaled=False)["choice"] in ("u/2.5", "wmean")
    nonnormal = np.eye(d) + np.triu(np.ones((d, d)), 1)           # tr(A^2) / tr A = 1 although every norm is ~d: U / 2.5 wins
    sr = R.scale_rule(nonnormal)
    assert sr["choice"] == "u/2.5" and sr["wmean"] < sr["c"]
    assert R.scale_rule(np.zeros((d, d)))["c"] == 0.0


def test_participation_exponent_inverts_the_power_law():
    for d in (33, 100, 512):
        for p in (0.5, 1.0, 2.0, 4.0):
            pr = R._trapezoid_power_sum(p, d) ** 2 / R._trapezoid_power_sum(2 * p, d)
            assert R.participation_exponent(pr, d) == pytest.approx(p, abs=1e-7)      # (the closed form cancels near p = 1)
    mu = R.schedule_from_l0(1e-5)
    assert mu[0] == pytest.approx(math.sqrt(3.0), rel=1e-5) and np.all(mu[20:] == 1.0) and np.all(mu >= 1.0)
