"""The all-float64 Newton-Schulz route (csrc/frechet_f64.hip, ns_check.h, the tail of frechet_single in frechet.hip) through the public
entries, against tests/frechet_f64_reference.py: values, traces, scale, stop code and iteration count over d = 1 .. 512, full-rank and
rank-deficient, at three overall scales; max_iter and tol; degenerate inputs; the eps retry taken, failing and not needed; errors and
the call after them; independence of the thread's history; fad_frechet_from_moments.

`max_iter` / `tol` pin the float64 route at every d; without them d % 64 != 0 does.  Tolerances: tests/frechet_f64_reference.py
(tr_sqrt_bound: 16x the emulation's own error, floored at d 2^-52; sum_bound and scale_bound: derived); DESIGN.md 4.3.1 lists them with
the ratios measured on the MI355X.  An iteration count is asserted exactly where the emulation decides it with a margin of 10
(`firm`), and to one iteration where the case is marked in the reference."""
import ctypes as C
import importlib.util
import logging
import math
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
_spec = importlib.util.spec_from_file_location("frechet_f64_reference", Path(__file__).resolve().parent / "frechet_f64_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

U = 2.0 ** -53


def _raw(mu1, C1, mu2, C2, eps=1e-6, max_iter=0, tol=0.0):
    """lib.fad_frechet on host arrays -> (status, distance, diag dict): status and diag are read after an error as well."""
    from fadtk_amd import _capi
    lib = _capi.load_library()
    _capi.require_gpu(0)
    mu1, mu2 = _capi.f64_host(mu1), _capi.f64_host(mu2)
    d = mu1.shape[0]
    C1, C2 = _capi.f64_host(C1, (d, d)), _capi.f64_host(C2, (d, d))
    out, diag = C.c_double(float("nan")), _capi.FadDiag()
    st = lib.fad_frechet(d, mu1.ctypes.data, C1.ctypes.data, mu2.ctypes.data, C2.ctypes.data, float(eps), int(max_iter), float(tol), 0, 0,
                         _capi.current_stream_ptr(0), C.byref(out), C.byref(diag))
    return st, float(out.value), diag.as_dict()


def _check_count(got, e, loose):
    if e["firm"] and not loose:
        assert got == e["iters"], (got, e["iters"], e["rule"])
    else:
        assert abs(got - e["iters"]) <= 1, (got, e["iters"], e["rule"], e["margin"], e["margin_res"])


def _check_parts(diag, out, mu1, C1, mu2, C2, tr_sqrt_want, tr_sqrt_bound, what=""):
    """tr_sqrt, tr1, tr2, mean_term and the distance against the host's, each at its derived bound; prints err / bound."""
    gap = np.asarray(mu1) - np.asarray(mu2)
    want = dict(tr_sqrt=tr_sqrt_want, tr1=float(np.trace(C1)), tr2=float(np.trace(C2)), mean_term=float(gap @ gap))
    bound = dict(tr_sqrt=tr_sqrt_bound, tr1=R.sum_bound(np.diag(C1)), tr2=R.sum_bound(np.diag(C2)), mean_term=R.sum_bound(gap * gap, each=8 * U))
    ratios = {}
    for k in want:
        err = abs(diag[k] - want[k])
        ratios[k] = err / bound[k] if bound[k] > 0 else (0.0 if err == 0 else math.inf)
    dist = want["mean_term"] + want["tr1"] + want["tr2"] - 2 * want["tr_sqrt"]
    mag = want["mean_term"] + abs(want["tr1"]) + abs(want["tr2"]) + 2 * abs(want["tr_sqrt"])
    b_dist = bound["mean_term"] + bound["tr1"] + bound["tr2"] + 2 * bound["tr_sqrt"] + 8 * U * mag
    ratios["distance"] = abs(out - dist) / b_dist
    print(what, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (what, k, v)
    # the distance is assembled from the parts the call reports
    parts = diag["mean_term"] + diag["tr1"] + diag["tr2"] - 2 * diag["tr_sqrt"]
    assert abs(out - parts) <= 8 * U * mag
    return ratios


# ---------------------------------------------------------------------------------------------------------------- values
VALUE_RUNS = [(d, deficient, s, pinned) for (d, deficient, s) in R.VALUE_CASES for pinned in (True, False) if pinned or d % 64 != 0]


@pytest.mark.parametrize("d,deficient,scale,pinned", VALUE_RUNS)
def test_values_scale_code_and_count(d, deficient, scale, pinned):
    mu1, C1, mu2, C2 = R.value_case(d, deficient, scale)
    e, x, bound = R.value_reference(d, deficient, scale)
    st, out, diag = _raw(mu1, C1, mu2, C2, max_iter=64 if pinned else 0)
    assert st == 0 and diag["route"] == 0 and diag["used_eps"] == 0
    _check_parts(diag, out, mu1, C1, mu2, C2, x, bound, f"d={d} deficient={deficient} scale={scale:g}: err / bound")
    c_bound, _ = R.scale_bound(C1, C2)
    print(f"  scale: err / bound {abs(diag['scale'] - e['c']) / c_bound:.3f}   iters {diag['iters']} (emulation {e['iters']}, {e['rule']})")
    assert abs(diag["scale"] - e["c"]) <= c_bound
    assert diag["converged"] == (2 if deficient else 1)
    _check_count(diag["iters"], e, (d, deficient) in R.COUNT_MAY_DIFFER_BY_ONE)


@pytest.mark.parametrize("d,p,same", R.DECAY_CASES)
def test_decaying_spectra_on_the_scaled_steps(d, p, same):
    mu1, C1, mu2, C2 = R.decay_case(d, p, same)
    e, x = R.emulate(C1, C2), R.tr_sqrt_exact(C1, C2)
    plain = R.emulate(C1, C2, allow_scaled=False)
    st, out, diag = _raw(mu1, C1, mu2, C2)
    assert st == 0 and diag["route"] == 0 and diag["converged"] == 1
    _check_parts(diag, out, mu1, C1, mu2, C2, x, R.tr_sqrt_bound(e["tr_sqrt"], x, d), f"d={d} k^-{p:g} same={same}: err / bound")
    c_bound, _ = R.scale_bound(C1, C2)
    assert abs(diag["scale"] - e["c"]) <= c_bound                 # c = U: the scaled start
    # the device's x_min estimate comes from float exp2 / log2 and 20 bisection steps, the emulation's from float64: the schedules
    # differ in their last digits, the count by at most one -- and it stays well below the plain iteration's
    assert abs(diag["iters"] - e["iters"]) <= 1 and diag["iters"] + 1 < plain["iters"]


# ---------------------------------------------------------------------------------------------------------------- limits
def test_max_iter_returns_the_third_iterate_with_a_warning(caplog):
    from fadtk_amd import _capi, hip
    d = R.LIMIT_CASE[0]
    mu1, C1, mu2, C2 = R.value_case(*R.LIMIT_CASE)
    st, out, diag = _raw(mu1, C1, mu2, C2, max_iter=3)
    assert st == _capi.FAD_ERR_NOT_CONVERGED and diag["converged"] == 0 and diag["iters"] == 3 and diag["used_eps"] == 0
    c_bound, _ = R.scale_bound(C1, C2)
    e = R.emulate(C1, C2, max_iter=3)
    assert abs(diag["scale"] - e["c"]) <= c_bound
    # an unconverged iterate depends on the scale it started from, so the emulation starts from the device's (held to the host's just
    # above); its own rounding error is what separates it from the same steps in long double
    e = R.emulate(C1, C2, max_iter=3, c=diag["scale"])
    wide = R.emulate(C1, C2, max_iter=3, c=diag["scale"], dtype=np.longdouble)
    assert (e["conv"], e["iters"]) == (0, 3)
    _check_parts(diag, out, mu1, C1, mu2, C2, e["tr_sqrt"], R.tr_sqrt_bound(e["tr_sqrt"], wide["tr_sqrt"], d), "max_iter=3: err / bound")
    with caplog.at_level(logging.WARNING):
        got, gd = hip.frechet(mu1, C1, mu2, C2, max_iter=3)       # the wrapper hands the value on
    assert got == out and gd["converged"] == 0 and any("max_iter" in r.getMessage() for r in caplog.records)


def test_tol_closes_earlier_within_the_predicted_residual():
    """tol = 1e-3 on the input made for it (R.tol_case: every check of the emulation 10x from the tolerance, proved by the host test):
    exactly the emulation's count, and exactly the emulation's count without it."""
    d = R.TOL_CASE[0]
    mu1, C1, mu2, C2 = R.tol_case()
    e, full, x = R.emulate(C1, C2, tol=1e-3), R.emulate(C1, C2), R.tr_sqrt_exact(C1, C2)
    assert e["firm_per_check"] and full["firm_per_check"]
    bound = R.tr_sqrt_bound(full["tr_sqrt"], x, d)
    st, out, diag = _raw(mu1, C1, mu2, C2, tol=1e-3)
    st0, out0, diag0 = _raw(mu1, C1, mu2, C2, max_iter=64)
    assert st == 0 and st0 == 0 and diag["converged"] == 1 and diag0["converged"] == 1 and diag["route"] == 0
    print(f"tol=1e-3: iters {diag['iters']} (emulation {e['iters']}), default {diag0['iters']} (emulation {full['iters']})")
    assert diag["iters"] == e["iters"] and diag0["iters"] == full["iters"] and diag["iters"] < diag0["iters"]
    _check_parts(diag0, out0, mu1, C1, mu2, C2, x, bound, "  default: err / bound")
    # y_i = sqrt(a_i (1 - e_i)) and |e_i| <= ||E||_F: the early answer is within (the bound 3/4 r^2 + 1/4 r^3 the host predicted the finish
    # with) x tr_sqrt of the converged one -- and, being the same iterate, within the 16x rule of the emulation's early answer
    print(f"  |early - converged| {abs(diag['tr_sqrt'] - diag0['tr_sqrt']):.3e}  allowed {e['bound'] * x + bound:.3e};  "
          f"|early - emulation's| {abs(diag['tr_sqrt'] - e['tr_sqrt']):.3e}  allowed {bound:.3e}")
    assert e["bound"] <= 1e-3
    assert abs(diag["tr_sqrt"] - diag0["tr_sqrt"]) <= e["bound"] * x + bound
    assert abs(diag["tr_sqrt"] - e["tr_sqrt"]) <= bound


# ------------------------------------------------------------------------------------------------------- degenerate inputs
@pytest.mark.parametrize("d", [1, 33, 64, 100])
def test_zero_first_covariance(d):
    mu1, _, mu2, C2 = R.value_case(d, False, 1.0)
    Z = np.zeros((d, d))
    st, out, diag = _raw(mu1, Z, mu2, C2, max_iter=64)
    assert st == 0 and diag["iters"] == 1 and diag["converged"] == 1 and diag["tr_sqrt"] == 0.0 and diag["scale"] == 1.0
    _check_parts(diag, out, mu1, Z, mu2, C2, 0.0, 0.0, f"C1 = 0, d={d}: err / bound")


@pytest.mark.parametrize("which", ["value33", "value64", "decay100"])
def test_equal_covariances_give_zero(which):
    mu, C1 = {"value33": R.value_case(33, False, 1.0), "value64": R.value_case(64, False, 1e6), "decay100": R.decay_case(100, 2.0, True)}[which][:2]
    d = C1.shape[0]
    e, x = R.emulate(C1, C1), float(np.trace(C1))                 # sqrt(C C) = C
    st, out, diag = _raw(mu, C1, mu, C1, max_iter=64)
    assert st == 0 and diag["converged"] == 1 and diag["mean_term"] == 0.0
    b = R.tr_sqrt_bound(e["tr_sqrt"], x, d)
    print(f"C1 = C2 {which}: distance {out:.3e}, bound {2 * b + 2 * R.sum_bound(np.diag(C1)) + 16 * U * x:.3e}")
    assert abs(out) <= 2 * b + 2 * R.sum_bound(np.diag(C1)) + 16 * U * x


@pytest.mark.parametrize("a,b,m1,m2", [(2.0, 3.0, 0.5, -0.25), (1e-6, 4e6, 1.0, 1.0), (7.0, 7.0, 0.0, 3.0)])
def test_one_dimension_is_the_closed_form(a, b, m1, m2):
    st, out, diag = _raw(np.array([m1]), np.array([[a]]), np.array([m2]), np.array([[b]]), max_iter=64)
    want = (math.sqrt(a) - math.sqrt(b)) ** 2 + (m1 - m2) ** 2
    assert st == 0 and diag["converged"] == 1
    assert abs(diag["tr_sqrt"] - math.sqrt(a * b)) <= 8 * U * math.sqrt(a * b)
    assert abs(out - want) <= 16 * U * (a + b + 2 * math.sqrt(a * b) + (m1 - m2) ** 2)


# --------------------------------------------------------------------------------------------------------------- eps retry
def _after_an_error():
    """the next call on the same thread is right"""
    mu1, C1, mu2, C2 = R.value_case(33, False, 1.0)
    e, x, bound = R.value_reference(33, False, 1.0)
    st, out, diag = _raw(mu1, C1, mu2, C2, max_iter=64)
    assert st == 0 and diag["converged"] == 1 and diag["used_eps"] == 0 and diag["iters"] == e["iters"]
    _check_parts(diag, out, mu1, C1, mu2, C2, x, bound, "  call after the error: err / bound")


def test_eps_retry_succeeds_and_takes_the_shift_back_out():
    """(tr1 / tr2 are held to the derived bound of the sum, ~45 ulps at d = 33, not to "a few ulps": see below)"""
    lam, eps, d = -5e-7, 1e-6, 33
    mu1, C1, mu2, C2 = R.negative_case(lam)
    _, E1, _, E2 = R.shifted_case(lam, eps)
    first, e, x = R.emulate(C1, C2), R.emulate(E1, E2), R.tr_sqrt_exact(E1, E2)
    assert first["nonfinite"] and first["firm"] and e["conv"] == 1
    st, out, diag = _raw(mu1, C1, mu2, C2, eps=eps)
    assert st == 0 and diag["used_eps"] == 1 and diag["converged"] == 1
    _check_count(diag["iters"], e, loose=False)
    # tr_sqrt is the shifted pair's; tr1 and tr2 are the CALLER's: the sum of the shifted diagonal, then eps d taken off.  Their bound is
    # the derived one of a d-term sum in any order plus the product and the subtraction, (d + 8) u sum |c_ii + eps| + 4 u (|tr| + eps d):
    # about 45 ulps of the trace at d = 33 -- looser than "a few ulps", and eight orders below what a shift left in would be (eps (d - 1))
    assert abs(diag["tr_sqrt"] - x) <= R.tr_sqrt_bound(e["tr_sqrt"], x, d)
    for key, M, S in (("tr1", C1, E1), ("tr2", C2, E2)):
        b = R.sum_bound(np.diag(S)) + 4 * U * (abs(np.trace(S)) + eps * d)
        print(f"eps retry {key}: err {abs(diag[key] - np.trace(M)):.3e} bound {b:.3e}")
        assert abs(diag[key] - np.trace(M)) <= b
    gap = mu1 - mu2
    want = float(gap @ gap) + np.trace(C1) + np.trace(C2) - 2 * x
    assert abs(out - (diag["mean_term"] + diag["tr1"] + diag["tr2"] - 2 * diag["tr_sqrt"])) <= 16 * U * abs(want)
    assert abs(out - want) <= 2 * R.tr_sqrt_bound(e["tr_sqrt"], x, d) + 64 * U * (abs(want) + 2 * x)
    _after_an_error()


@pytest.mark.parametrize("eps,used", [(1e-6, 1), (0.0, 0)])
def test_eps_retry_fails_or_is_not_taken(eps, used):
    from fadtk_amd import _capi
    mu1, C1, mu2, C2 = R.negative_case(-0.3)
    assert R.emulate(C1, C2)["nonfinite"] and (eps == 0.0 or R.emulate(*R.shifted_case(-0.3, eps)[1::2])["nonfinite"])
    st, out, diag = _raw(mu1, C1, mu2, C2, eps=eps)
    assert st == _capi.FAD_ERR_NOT_FINITE and diag["used_eps"] == used and diag["iters"] == 0 and diag["converged"] == 0
    assert math.isnan(out)                                        # nothing is written on this error
    _after_an_error()


@pytest.mark.parametrize("lam", [-1e-12, -1e-9])
def test_roundoff_negative_eigenvalue_needs_no_retry(lam):
    mu1, C1, mu2, C2 = R.negative_case(lam)
    e, x = R.emulate(C1, C2), R.tr_sqrt_exact(C1, C2)             # (exact: that eigenvalue clamped to 0)
    assert e["rule"] == "runaway" and e["firm"]
    st, out, diag = _raw(mu1, C1, mu2, C2, eps=1e-6)
    assert st == 0 and diag["used_eps"] == 0 and diag["converged"] == 2
    _check_count(diag["iters"], e, loose=False)
    _check_parts(diag, out, mu1, C1, mu2, C2, x, R.tr_sqrt_bound(e["tr_sqrt"], x, 33), f"eigenvalue {lam:g}: err / bound")


@pytest.mark.parametrize("where", ["cov1", "cov2", "mu1"])
def test_nan_input_is_an_error_and_a_value_error_above(where):
    from fadtk_amd import _capi, calc_frechet_distance
    mu1, C1, mu2, C2 = (np.array(a) for a in R.value_case(33, False, 1.0))
    {"cov1": C1, "cov2": C2, "mu1": mu1}[where][(5, 7) if where != "mu1" else 5] = np.nan
    st, out, diag = _raw(mu1, C1, mu2, C2, eps=1e-6)
    assert st == _capi.FAD_ERR_NOT_FINITE
    with pytest.raises(ValueError):
        calc_frechet_distance(mu1, C1, mu2, C2)
    _after_an_error()


# ----------------------------------------------------------------------------------------------------- history independence
# (first call of a fresh thread: the first chunk is 6 checks, later ones what the previous call needed + 1, then 4 at a time.  A
#  predicted finish -- at check iters - 2 -- falls on the LAST check of a chunk for P7 first in its thread (5), P23 first in its thread
#  (5 + 16) and P23 after P9 (9 + 12), and inside a chunk everywhere else.)
SEQUENCES = [["P24", "P7", "P24"], ["P7", "P24", "P7"], ["P9", "P23", "P7", "P23"], ["P23", "P9"]]


def test_result_does_not_depend_on_the_threads_previous_calls():
    seen, errors = {}, []

    def run(seq):
        try:
            for pos, name in enumerate(seq):
                mu1, C1, mu2, C2 = R.history_problem(name)
                st, out, diag = _raw(mu1, C1, mu2, C2, eps=0.0, max_iter=64)
                seen.setdefault(name, []).append(("/".join(seq) + f"[{pos}]", st, diag["iters"], np.float64(diag["tr_sqrt"]).tobytes(), np.float64(out).tobytes()))
        except Exception as exc:       # noqa: BLE001 - reported by the assertion below
            errors.append(exc)

    for seq in SEQUENCES:              # one fresh thread per sequence, one after the other
        t = threading.Thread(target=run, args=(seq,))
        t.start()
        t.join()
    assert not errors, errors
    for name, runs in seen.items():
        want = R.HISTORY_PROBLEMS[name][0]
        print(name, [(r[0], r[2]) for r in runs])
        assert len(runs) >= 2
        for where, st, iters, bits, out_bits in runs:
            assert st == 0 and iters == want, (name, where, st, iters, want)
            assert bits == runs[0][3] and out_bits == runs[0][4], (name, where, "differs from", runs[0][0])


# --------------------------------------------------------------------------------------------------------------- from moments
def test_from_moments_agrees_with_the_finalized_pair():
    from fadtk_amd import _capi, hip
    d = 100
    rng = np.random.default_rng(11)
    x1 = rng.standard_normal((700, d)) * np.linspace(0.5, 2.0, d)
    x2 = rng.standard_normal((450, d)) * np.linspace(2.0, 0.5, d) + 0.1
    with hip.Moments(d) as m1, hip.Moments(d) as m2, hip.Moments(d) as one:
        m1.update(x1)
        m2.update(x2)
        mu1, C1, n1 = m1.finalize()
        mu2, C2, n2 = m2.finalize()
        assert (n1, n2) == (700, 450)
        got, gd = hip.frechet_from_moments(m1, m2, max_iter=64)
        st, out, diag = _raw(mu1, C1, mu2, C2, max_iter=64)
        e, x = R.emulate(C1, C2), R.tr_sqrt_exact(C1, C2)
        assert st == 0 and gd["route"] == 0 and gd["converged"] == diag["converged"] == e["conv"] == 1
        _check_parts(gd, got, mu1, C1, mu2, C2, x, R.tr_sqrt_bound(e["tr_sqrt"], x, d), "from moments: err / bound")
        _check_parts(diag, out, mu1, C1, mu2, C2, x, R.tr_sqrt_bound(e["tr_sqrt"], x, d), "finalized pair: err / bound")
        assert gd["iters"] == diag["iters"]
        one.update(x1[:1])
        lib = _capi.load_library()
        o, dg = C.c_double(), _capi.FadDiag()
        for a, b in ((one, m2), (m1, one)):
            st = lib.fad_frechet_from_moments(a._h, b._h, 1, 1e-6, 64, 0.0, -1, _capi.current_stream_ptr(0), C.byref(o), C.byref(dg))
            assert st == _capi.FAD_ERR_TOO_FEW_ROWS
        with pytest.raises(AssertionError):
            hip.frechet_from_moments(one, m2, max_iter=64)
        got2, gd2 = hip.frechet_from_moments(m1, m2, max_iter=64)          # and the handles are as they were
        assert got2 == got and gd2["iters"] == gd["iters"]
