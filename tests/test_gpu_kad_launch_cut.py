"""The KAD family's passes cut into several launches, on the GPU (csrc/kad.hip: every loop over kad::launches).

At the production budget of 2^30 cost units a launch holds millions of tiles, so at every size the rest of the suite runs a pass is one
launch: u0 > 0, the slot offset of a second launch, a histogram added up over launches, the top-k slots of a second launch's row
ranges and kad_slots_sum_kernel over several launches' slots never run.  Here FAD_KAD_LAUNCH_BUDGET (read at the start of every
entry) makes small passes take several launches, and fad_kad_last_plan (hip.kad_last_plan) reports what the call really planned, so no
case trusts a copy of the cost formula: every case asserts on the tally of its cut call before anything else.

Every case runs its entry twice, the variable unset and then set, and holds the cut call
  * to the float64 numpy reference of the entry's own test file (tests/*_reference.py) at that file's tolerance -- exactly, on integer
    rows, for the median, PRDC, the k-NN entries and KID;
  * to the uncut call: bit for bit where the output is integer-exact; elsewhere within CUT_RTOL = 1e-12 of the mean of |k| of the
    block.  That bound is derived, not measured: in every sum kernel a tile's float32 lane sum depends on the tile alone
    (kad_pass_kernel, kad_sweep_kernel, col_sums, kad_perm_kernel, kid_pass_kernel: `d += (double)s` once per tile), so the cut only
    moves tiles between float64 partials; fewer than 2^12 float64 additions lie on any value's path at these sizes, and
    4096 * 2^-53 = 4.5e-13.  No entry carries a float32 partial across tiles.  (On the MI355X every difference is 0: float64 sums of
    so few float32 lane sums of like magnitude are exact, whatever their order.)
Regime A (budget 1: the floor of 64 tiles per launch) puts every pass of every entry in at least two launches at n = 1290, m = 1410
(11 and 12 row blocks).  Regime B (n = 5800, m = 1300; a budget per case) cuts a pass into launches of more than 512 tiles, so that a
persistent workgroup of a cut launch walks a second slot (L += G).  One more case runs fad_kad at the production budget on a shape
whose baseline triangle needs two launches.  Each case prints a [kad-cut] line (profiles/kad_cut_err.txt)."""
import ctypes as C
import functools
import hashlib
import time

import numpy as np
import pytest
from scipy.spatial.distance import cdist as _scipy_cdist

import kad_aggregate_reference as AR
import kad_conditioning_reference as CR
import kad_kernels_reference as KR
import kid_reference as KID
import nearest_reference as NR
import nn_test_reference as NT
import prdc_reference as PRDC
import test_gpu_kad as TK
import test_gpu_kad_individual as TI
import test_gpu_kad_uncertainty as TU
import test_gpu_kid as TKID
import test_gpu_nn_test as TNN
from test_gpu_kad import MEAN_RTOL, MMD_TOL
from test_gpu_kad_permutation import TAU
from test_gpu_kad_uncertainty import COV_RTOL

pytestmark = pytest.mark.gpu
PR = AR.PR
ENV = "FAD_KAD_LAUNCH_BUDGET"
CUT_RTOL = 1e-12
NOT_FINITE = -7
assert MEAN_RTOL == 4e-7 and MMD_TOL == 1.5e-7 and TAU == 1e-2 and COV_RTOL == 1e-4
MEANS = ("kxx_mean", "kyy_mean", "kxy_mean")

# regime A: (dtype, D, row pitch of the device rows or None for host rows); 1290 and 1410 rows are 11 and 12 row blocks: 66 and 78
# triangle tiles, 132 rectangle tiles, 253 triangle tiles of the 2700 pooled rows -- every pass more than 64 tiles or units
N_A, M_A = 1290, 1410
CASES_A = [("fp16", 128, None), ("bf16", 72, 80), ("fp32", 17, None)]
IDS_A = [c[0] for c in CASES_A]
SONG_LENGTHS = (0, 1, 2, 127, 129, 300)                    # and the rest of the 1410 rows as the last song
P_LABELS = 33                                              # with the observed labelling 34: two label words, the second partial
# regime B: 5800 rows are 46 row blocks (1081 triangle tiles, 2116 tiles of X x X), 1300 rows 11; 7100 pooled rows 56 blocks
N_B, M_B = 5800, 1300
CASES_B = [("fp16", 128), ("fp32", 17)]


# ------------------------------------------------------------------------------------------------------------------- plumbing
def _rows(a, dt, ld=None):
    """float32 values that are exact in dt -> fp16 / fp32 numpy rows on the host; bf16 (or any dt with a pitch) a torch tensor on the
    device, a view of a wider buffer whose pitch bytes are never read"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert np.array_equal(CR.round_to(a, dt), a), dt
    if dt == "bf16" or ld is not None:
        import torch
        t = torch.from_numpy(a).cuda().to({"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[dt])
        if ld is None:
            return t
        wide = torch.full((a.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")
        wide[:, :a.shape[1]] = t
        return wide[:, :a.shape[1]]
    return a.astype(np.float16) if dt == "fp16" else a


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


@functools.lru_cache(maxsize=None)
def _gauss(n, m, d, dt):
    """test_gpu_kad._sets with the second set shifted, rounded to dt (float32 values)"""
    x, y = TK._sets(n, m, d, 1, seed=n + d)
    return CR.round_to(x, dt), CR.round_to(y, dt)


@functools.lru_cache(maxsize=None)
def _ints(n, m, d):
    """integer rows in [-3, 3] with duplicates inside each set and a y row on an x row: exact in every dtype, every d^2 exact"""
    return CR.exact_sets(n, m, d, 0)


@functools.lru_cache(maxsize=None)
def _labels(n, m, seed=5):
    return PR.random_labellings(n, m, P_LABELS, np.random.default_rng(seed))


class _Distances:
    """What the reference modules call as scipy's cdist, memoised over a case's blocks (a case asks for the same block once per
    bandwidth).  gemm: |a|^2 + |b|^2 - 2 a.b in float64 instead -- exact on integer rows, within 1e-13 of |a|^2 + |b|^2 on Gaussian
    ones (as _ref_kxx of test_gpu_kad_individual.py) -- for regime B, where cdist alone would take each case tens of seconds."""

    def __init__(self, gemm):
        self.gemm, self.memo = gemm, {}

    def __call__(self, a, b, metric):
        assert metric == "sqeuclidean"
        a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        key = tuple(hashlib.sha1(v.tobytes()).hexdigest() + str(v.shape) for v in (a, b))
        if key not in self.memo:
            if self.gemm:
                self.memo[key] = np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T), 0.0)
            else:
                self.memo[key] = _scipy_cdist(a, b, "sqeuclidean")
        return self.memo[key].copy()                       # the references fill diagonals in place


@pytest.fixture
def distances(monkeypatch):
    def use(gemm=False):
        f = _Distances(gemm)
        for mod in (KR, PRDC, NR, NR.P, NT, NT.NR, NT.NR.P, PR, NT.PR):
            monkeypatch.setattr(mod, "cdist", f)
        return f
    return use


def _twice(monkeypatch, budget, call):
    """call() with the variable unset and then at `budget` -> (uncut result, cut result, the cut call's tally); the uncut call must be one
    launch per pass"""
    from fadtk_amd import hip
    monkeypatch.delenv(ENV, raising=False)
    uncut = call()
    plan0 = hip.kad_last_plan()
    monkeypatch.setenv(ENV, str(budget))
    cut = call()
    plan = hip.kad_last_plan()
    monkeypatch.delenv(ENV)
    assert plan0["passes"] == plan["passes"] >= 1 and plan0["max_launches"] == 1, (plan0, plan)
    return uncut, cut, plan


def _tally_a(plan):
    """regime A: every pass of the call in at least two launches"""
    assert plan["min_launches"] >= 2 and plan["launches"] >= 2 * plan["passes"], plan


def _tally_b(plan):
    """regime B: a pass in at least two launches, and a launch whose workgroups walk a second slot"""
    assert plan["max_launches"] >= 2 and plan["slots_per_workgroup"] >= 2, plan


def _line(entry, dt, budget, plan, err64, err_cut):
    t = plan
    print(f"[kad-cut] {entry} {dt} budget={budget} passes={t['passes']} launches={t['launches']} min={t['min_launches']} "
          f"max={t['max_launches']} slots/wg={t['slots_per_workgroup']} err_f64={err64:.2e} err_uncut={err_cut:.2e}")


def _means_near_uncut(cut, uncut):
    """each mean within CUT_RTOL of the uncut one (every kernel value is > 0: the mean of |k| is the mean), MMD^2 within CUT_RTOL of
    Kxx + Kyy + 2 Kxy; the bandwidth (an exact median of counted float32 values) bit for bit -> worst relative difference"""
    assert cut["bandwidth"] == uncut["bandwidth"] and cut["n"] == uncut["n"] and cut["m"] == uncut["m"]
    scale = uncut["kxx_mean"] + uncut["kyy_mean"] + 2 * uncut["kxy_mean"]
    worst = abs(cut["mmd2"] - uncut["mmd2"]) / scale
    assert worst <= CUT_RTOL, ("mmd2", cut["mmd2"], uncut["mmd2"])
    for k in MEANS:
        rel = abs(cut[k] - uncut[k]) / uncut[k]
        assert rel <= CUT_RTOL, (k, cut[k], uncut[k])
        worst = max(worst, rel)
    return worst


def _entry(sweep, b):
    return {k: (sweep[k] if k in ("n", "m") else float(sweep[k][b])) for k in ("mmd2",) + MEANS + ("bandwidth", "n", "m")}


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif isinstance(a[k], float) and np.isnan(a[k]):
            assert np.isnan(b[k]), k
        elif hasattr(a[k], "shape"):
            assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


# -------------------------------------------------------------------------------------------------- the sums, on Gaussian rows
def _check_kad(monkeypatch, regime, dt, d, ld, n, m, budget, kernel):
    from fadtk_amd import hip
    xv, yv = _gauss(n, m, d, dt)
    x, y = _rows(xv, dt, ld), _rows(yv, dt, ld)
    uncut, cut, plan = _twice(monkeypatch, budget, lambda: hip.kad(x, y, kernel=kernel))
    regime(plan)
    assert plan["passes"] == 4                              # the median's histogram rounds (one plan), XX, YY, XY
    errs = TK._check(cut, KR.kad(xv, yv, cut["bandwidth"], kernel), f"cut {kernel} {dt} n={n} m={m} budget={budget}")
    _line(f"kad[{kernel}]", dt, budget, plan, max(errs.values()), _means_near_uncut(cut, uncut))


@pytest.mark.parametrize("kernel", KR.KERNELS)
@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_kad(monkeypatch, distances, dt, d, ld, kernel):
    distances()
    _check_kad(monkeypatch, _tally_a, dt, d, ld, N_A, M_A, 1, kernel)


def _check_sweep(monkeypatch, regime, dt, d, ld, n, m, budget, n_bw, kernel="gaussian"):
    from fadtk_amd import hip
    xv, yv = _gauss(n, m, d, dt)
    x, y = _rows(xv, dt, ld), _rows(yv, dt, ld)
    factors = [float(f) for f in 2.0 ** np.linspace(-1.0, 1.0, n_bw)]
    uncut, cut, plan = _twice(monkeypatch, budget, lambda: hip.kad_sweep(x, y, factors=factors, kernel=kernel))
    regime(plan)
    groups = -(-n_bw // 8)
    assert plan["passes"] == 1 + 3 * groups                 # the median, then XX, YY, XY per group of up to 8 bandwidths
    med = hip.kad_median_distance(x)
    worst64 = worst_cut = 0.0
    for b, f in enumerate(factors):
        assert cut["bandwidth"][b] == f * med
        got = _entry(cut, b)
        errs = TK._check(got, KR.kad(xv, yv, got["bandwidth"], kernel), f"cut sweep {dt} B={n_bw} b={b} budget={budget}")
        worst64 = max(worst64, max(errs.values()))
        worst_cut = max(worst_cut, _means_near_uncut(got, _entry(uncut, b)))
    _line(f"kad_sweep[B={n_bw}]", dt, budget, plan, worst64, worst_cut)


@pytest.mark.parametrize("n_bw", [3, 8, 9])                 # the kernels of 4 and of 8 bandwidths, and a group of 8 with a rest of one
@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_kad_sweep(monkeypatch, distances, dt, d, ld, n_bw):
    distances()
    _check_sweep(monkeypatch, _tally_a, dt, d, ld, N_A, M_A, 1, n_bw)


@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_kad_individual(monkeypatch, distances, dt, d, ld):
    """Songs of 0, 1, 2, 127, 129, 300 rows and the rest: the cross pass is 132 units (3 launches), the band pass one unit per column
    block, 12 units of up to kBandPiece = 32 tiles, two to a launch of 64 tiles (6 launches)."""
    from fadtk_amd import hip
    distances()
    xv, yv = _gauss(N_A, M_A, d, dt)
    off = np.concatenate([[0], np.cumsum(SONG_LENGTHS), [M_A]]).astype(np.int64)
    songs = [yv[off[s]:off[s + 1]] for s in range(len(off) - 1)]
    x, y = _rows(xv, dt, ld), _rows(yv, dt, ld)
    uncut, cut, plan = _twice(monkeypatch, 1, lambda: hip.kad_individual(x, y, off))
    _tally_a(plan)
    assert plan["passes"] == 4                              # the median, XX, the cross pass, the band pass
    sigma = cut["bandwidth"]
    assert sigma == uncut["bandwidth"] == hip.kad_median_distance(x)
    kxx, _, want = KR.kad_individual(xv, songs, sigma, "gaussian")
    assert cut["kxx_mean"] == pytest.approx(kxx, rel=MEAN_RTOL) and abs(cut["kxx_mean"] - uncut["kxx_mean"]) <= CUT_RTOL * kxx
    worst64 = worst_cut = 0.0
    assert np.array_equal(cut["status"], uncut["status"])
    for s, song in enumerate(songs):
        if len(song) < 2:
            assert want[s] is None and cut["status"][s] == TI.TOO_FEW and np.isnan(cut["mmd2"][s]) and np.isnan(cut["kyy_mean"][s])
            continue
        assert cut["status"][s] == 0
        worst64 = max(worst64, TI._check_song(cut, s, want[s], f"cut {dt} song {s}"))
        scale = want[s]["kxx_mean"] + want[s]["kyy_mean"] + 2 * want[s]["kxy_mean"]
        for k in ("kyy_mean", "kxy_mean"):
            rel = abs(cut[k][s] - uncut[k][s]) / uncut[k][s]
            assert rel <= CUT_RTOL, (s, k, cut[k][s], uncut[k][s])
            worst_cut = max(worst_cut, rel)
        assert abs(cut["mmd2"][s] - uncut["mmd2"][s]) <= CUT_RTOL * scale, s
    _line("kad_individual", dt, 1, plan, worst64, worst_cut)


@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_kad_uncertainty(monkeypatch, distances, dt, d, ld):
    """Two evaluation sets.  The covariance is quadratic in the centred projections, each within CUT_RTOL of the kernel-mean scale of
    the uncut call's: it is held to the uncut call at 1e-9 of its largest entry (the centring takes at most three digits here), and to
    float64 at COV_RTOL."""
    from fadtk_amd import hip
    distances()
    xv, yv = _gauss(N_A, M_A, d, dt)
    _, y2v = _gauss(N_A, 700, d, dt)
    ysv = [yv, -y2v]                                        # a second set on the other side of the baseline (negation is exact)
    x, ys = _rows(xv, dt, ld), [_rows(v, dt, ld) for v in ysv]
    uncut, cut, plan = _twice(monkeypatch, 1, lambda: hip.kad_uncertainty(x, ys, rows=True))
    _tally_a(plan)
    assert plan["passes"] == 2                              # the median, the Z x Z pass
    assert cut["bandwidth"] == uncut["bandwidth"] and np.array_equal(cut["m"], [M_A, 700]) and cut["n"] == N_A
    want = KR.uncertainty(xv, ysv, cut["bandwidth"], "gaussian")
    TU._check(cut, want, f"cut {dt}")
    worst64 = worst_cut = 0.0
    for s, w in enumerate(want["sets"]):
        scale = w["kxx_mean"] + w["kyy_mean"] + 2 * w["kxy_mean"]
        worst64 = max([worst64, abs(cut["mmd2"][s] - w["mmd2"]) / scale] + [abs(cut[k][s] - w[k]) / w[k] for k in ("kyy_mean", "kxy_mean")])
        diffs = [abs(cut["mmd2"][s] - uncut["mmd2"][s]) / scale, float(np.max(np.abs(cut["proj_x"][s] - uncut["proj_x"][s]))) / scale,
                 float(np.max(np.abs(cut["proj_y"][s] - uncut["proj_y"][s]))) / scale]
        diffs += [abs(cut[k][s] - uncut[k][s]) / uncut[k][s] for k in ("kyy_mean", "kxy_mean")]
        assert max(diffs) <= CUT_RTOL, (s, diffs)
        worst_cut = max(worst_cut, max(diffs))
    assert abs(cut["kxx_mean"] - uncut["kxx_mean"]) <= CUT_RTOL * uncut["kxx_mean"]
    assert np.max(np.abs(cut["cov"] - uncut["cov"])) <= 1e-9 * np.max(np.abs(uncut["cov"]))
    _line("kad_uncertainty", dt, 1, plan, worst64, worst_cut)


def _perm_tau(xr, yr, sigma, null, rng):
    """TAU of the reference null's standard deviation, from 200 more labellings when the call's are fewer than 50 (test_gpu_kad_permutation.py)"""
    spread = null if len(null) >= 50 else PR.statistics(xr, yr, PR.random_labellings(len(xr), len(yr), 200, rng), sigma)
    return TAU * float(np.std(spread))


@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_kad_permutation_test(monkeypatch, distances, dt, d, ld):
    """P = 33.  Every |k - c0| is below 1, so a statistic (Sxx / n(n-1) + Syy / m(m-1) - 2 Sxy / nm of sums of k - c0) moves by less than
    4 CUT_RTOL between the cut and the uncut call."""
    from fadtk_amd import hip
    distances()
    xv, yv = _gauss(N_A, M_A, d, dt)
    x, y = _rows(xv, dt, ld), _rows(yv, dt, ld)
    u = _labels(N_A, M_A)
    words = hip.pack_labels(u)
    uncut, cut, plan = _twice(monkeypatch, 1, lambda: hip.kad_permutation_test(x, y, words))
    _tally_a(plan)
    assert plan["passes"] == 3                              # the pooled median, the r pass, the permutation pass (one word group)
    sigma = cut["bandwidth"]
    assert sigma == uncut["bandwidth"]
    xr, yr = xv.astype(np.float64), yv.astype(np.float64)
    t = PR.statistics(xr, yr, np.concatenate([PR.observed_labelling(N_A, M_A), u]), sigma)
    t0, null = t[0], t[1:]
    tau = _perm_tau(xr, yr, sigma, null, np.random.default_rng(9))
    err = max(abs(cut["mmd2"] - t0), float(np.max(np.abs(cut["null"] - null))))
    assert err <= tau, (dt, err, tau)
    if not np.any(np.abs(null - t0) <= 4 * tau):
        assert cut["p_value"] == uncut["p_value"] == PR.p_value(t0, null)
    err_cut = max(abs(cut["mmd2"] - uncut["mmd2"]), float(np.max(np.abs(cut["null"] - uncut["null"]))))
    assert err_cut <= 4 * CUT_RTOL, err_cut
    for k in MEANS:                                         # means of sums of values below 1 in magnitude
        assert abs(cut[k] - uncut[k]) <= CUT_RTOL, k
    _line("kad_permutation_test", dt, 1, plan, err / (tau / TAU), err_cut)


@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_kad_permutation_sweep(monkeypatch, distances, dt, d, ld):
    """Three bandwidths (the kernel of 4 with a row idle), P = 33."""
    from fadtk_amd import hip
    import test_gpu_kad_permutation_sweep as TPS
    distances()
    xv, yv = _gauss(N_A, M_A, d, dt)
    x, y = _rows(xv, dt, ld), _rows(yv, dt, ld)
    u = _labels(N_A, M_A)
    words = hip.pack_labels(u)
    factors = [0.5, 1.0, 2.0]
    uncut, cut, plan = _twice(monkeypatch, 1, lambda: hip.kad_permutation_sweep(x, y, words, factors=factors))
    _tally_a(plan)
    assert plan["passes"] == 3                              # the pooled median, one r pass and one walk for the three bandwidths
    assert cut["bandwidth"].tobytes() == uncut["bandwidth"].tobytes()
    TPS._assert_aggregate_is_the_reference_on_own_statistics(cut)
    xr, yr = xv.astype(np.float64), yv.astype(np.float64)
    t = AR.statistics(xr, yr, AR.with_observed(N_A, M_A, u), cut["bandwidth"])
    pv, pa = AR.aggregate(t)
    rng = np.random.default_rng(9)
    more = PR.random_labellings(N_A, M_A, 200, rng)
    worst, clear = 0.0, True
    for b, s in enumerate(cut["bandwidth"]):
        sd = float(np.std(PR.statistics(xr, yr, more, float(s))))
        err = max(abs(cut["mmd2"][b] - t[b, 0]), float(np.max(np.abs(cut["null"][b] - t[b, 1:]))))
        assert err <= TAU * sd, (b, err, TAU * sd)
        worst = max(worst, err / sd)
        if not np.any(np.abs(t[b, 1:] - t[b, 0]) <= 4 * TAU * sd):
            assert cut["p_values"][b] == uncut["p_values"][b] == pv[b], b
        else:
            clear = False
    if clear and all(pv == 1.0 / (P_LABELS + 1)):           # the observed statistic the largest at every bandwidth: min-p is its own
        assert cut["p_aggregated"] == pa
    err_cut = max(float(np.max(np.abs(cut["mmd2"] - uncut["mmd2"]))), float(np.max(np.abs(cut["null"] - uncut["null"]))))
    assert err_cut <= 4 * CUT_RTOL, err_cut
    for k in MEANS:
        assert np.max(np.abs(cut[k] - uncut[k])) <= CUT_RTOL, k
    _line("kad_permutation_sweep[B=3]", dt, 1, plan, worst, err_cut)


# ------------------------------------------------------------------------------------------------ integer-exact outputs
def _check_median(monkeypatch, regime, dt, d, ld, n, budget):
    from fadtk_amd import hip
    xi, _ = _ints(n, M_A if n == N_A else M_B, d)
    x = _rows(xi, dt, ld)
    uncut, cut, plan = _twice(monkeypatch, budget, lambda: hip.kad_median_distance(x))
    regime(plan)
    assert plan["passes"] == 1
    assert cut == uncut == KR.median_distance(xi), (cut, uncut)       # integer d^2: sqrt of the same float64 in both
    _line("kad_median_distance", dt, budget, plan, 0.0, 0.0)


@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_median_distance(monkeypatch, dt, d, ld):
    _check_median(monkeypatch, _tally_a, dt, d, ld, N_A, 1)


def _check_prdc(monkeypatch, regime, dt, d, ld, n, m, budget, k=5):
    from fadtk_amd import hip
    xi, yi = _ints(n, m, d)
    x, y = _rows(xi, dt, ld), _rows(yi, dt, ld)
    uncut, cut, plan = _twice(monkeypatch, budget, lambda: hip.prdc(x, y, k=k, details=True))
    regime(plan)
    assert plan["passes"] == 3                              # the radius passes of x and of y, the cross pass
    want = PRDC.prdc(xi, yi, k)
    for key in ("radius2_x", "radius2_y"):
        np.testing.assert_array_equal(cut[key].astype(np.float64), want[key])
    np.testing.assert_array_equal(cut["balls_y"], want["balls_y"])
    np.testing.assert_array_equal(cut["flags_x"], want["flags_x"])
    for key in ("precision", "recall", "density", "coverage"):
        assert cut[key] == want[key], (key, cut[key], want[key])
    _same_bits(cut, uncut)
    _line(f"prdc[k={k}]", dt, budget, plan, 0.0, 0.0)


@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_prdc(monkeypatch, distances, dt, d, ld):
    distances()
    _check_prdc(monkeypatch, _tally_a, dt, d, ld, N_A, M_A, 1)


def _check_nearest(monkeypatch, regime, dt, d, ld, n, m, budget, k):
    from fadtk_amd import hip
    xi, yi = _ints(n, m, d)
    x, y = _rows(xi, dt, ld), _rows(yi, dt, ld)
    uncut, cut, plan = _twice(monkeypatch, budget, lambda: hip.nearest(x, y, k=k, authenticity=True))
    regime(plan)
    assert plan["passes"] == 2                              # the radius pass of x (k = 1), the cross pass
    idx, d2 = NR.nearest(xi, yi, k)
    np.testing.assert_array_equal(cut["index"], idx)
    np.testing.assert_array_equal(cut["dist2"].astype(np.float64), d2)
    want = NR.authenticity(xi, yi)
    np.testing.assert_array_equal(cut["nn_radius2"].astype(np.float64), want["nn_radius2"])
    assert cut["copied"] == want["copied"] >= 1 and cut["authenticity"] == want["authenticity"]
    _same_bits(cut, uncut)
    _line(f"nearest[k={k}]", dt, budget, plan, 0.0, 0.0)


@pytest.mark.parametrize("k", [1, 5, 16])                   # three of the four key buckets (1, 8, 16)
@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_nearest(monkeypatch, distances, dt, d, ld, k):
    distances()
    _check_nearest(monkeypatch, _tally_a, dt, d, ld, N_A, M_A, 1, k)


def _check_nn_test(monkeypatch, regime, dt, d, ld, n, m, budget, k):
    from fadtk_amd import hip
    xi, yi = _ints(n, m, d)
    x, y = _rows(xi, dt, ld), _rows(yi, dt, ld)
    u = _labels(n, m)
    words = hip.pack_labels(u)
    uncut, cut, plan = _twice(monkeypatch, budget, lambda: hip.nn_test(x, y, words, k=k, return_graph=True))
    regime(plan)
    assert plan["passes"] == 1                              # Z x Z with the self pair masked
    want = NT.reference(xi, yi, u, k)
    np.testing.assert_array_equal(_np(cut["index"]), want["index"])
    np.testing.assert_array_equal(_np(cut["dist2"]).astype(np.float64), want["dist2"])
    TNN._same(cut, want, n, m)
    _same_bits(cut, uncut)
    _line(f"nn_test[k={k}]", dt, budget, plan, 0.0, 0.0)


@pytest.mark.parametrize("dt,d,ld", CASES_A, ids=IDS_A)
def test_regime_a_nn_test(monkeypatch, distances, dt, d, ld):
    distances()
    _check_nn_test(monkeypatch, _tally_a, dt, d, ld, N_A, M_A, 1, 5)


def _kid_rows(n, m, dt, ld):
    """rows in {-1, 0, 1} at D = 16 (kid_reference.exact_rows): every kernel value and every sum exact"""
    xv, yv = KID.exact_rows(n, m)
    return xv, yv, _rows(xv, dt, ld), _rows(yv, dt, ld)


def _check_kid(monkeypatch, regime, dt, ld, n, m, budget):
    from fadtk_amd import hip
    xv, yv, x, y = _kid_rows(n, m, dt, ld)
    uncut, cut, plan = _twice(monkeypatch, budget, lambda: hip.kid(x, y))
    regime(plan)
    assert plan["passes"] == 3
    want = KID.kid_full(xv, yv)
    for k in KID.MEANS:                                     # Sxx, Syy, Sxy over their exact counts
        assert cut[k] == want[k], (k, cut[k], want[k])
    assert abs(cut["mmd2"] - want["mmd2"]) <= 1e-14 * (want["abs_kxx_mean"] + want["abs_kyy_mean"] + 2 * want["abs_kxy_mean"])
    _same_bits(cut, uncut)
    _line("kid", dt, budget, plan, 0.0, 0.0)


@pytest.mark.parametrize("dt,ld", [("fp16", None), ("bf16", KID.EXACT_LD), ("fp32", None)], ids=IDS_A)
def test_regime_a_kid(monkeypatch, dt, ld):
    _check_kid(monkeypatch, _tally_a, dt, ld, N_A, M_A, 1)


@pytest.mark.parametrize("dt,ld", [("fp16", None), ("bf16", KID.EXACT_LD), ("fp32", None)], ids=IDS_A)
def test_regime_a_kid_subsets(monkeypatch, dt, ld):
    """17 subsets of 129 rows: 10 units each (3 + 3 triangle tiles, 4 rectangle tiles), 170 units in launches of 64."""
    from fadtk_amd import hip
    xv, yv, x, y = _kid_rows(N_A, M_A, dt, ld)
    ix, iy = KID.exact_indices(N_A, M_A, 17, 129, seed=17)
    uncut, cut, plan = _twice(monkeypatch, 1, lambda: hip.kid_subsets(x, y, ix, iy))
    _tally_a(plan)
    assert plan["passes"] == 1 and plan["launches"] == 3    # one group of 170 units
    terms, mmd2, mean, std = KID.subset_stats(KID.kid_subsets(xv, yv, ix, iy), 129)
    assert np.array_equal(cut["terms"], terms), np.abs(cut["terms"] - terms).max()
    tol = 1e-14 * TKID._scale(terms)
    assert np.abs(cut["mmd2"] - mmd2).max() <= tol and abs(cut["mean"] - mean) <= tol and abs(cut["std"] - std) <= tol
    _same_bits(cut, uncut)
    _line("kid_subsets[17x129]", dt, 1, plan, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------------ regime B
# A budget per case, chosen so that the largest pass is cut into launches of more than 512 tiles or units (the device's persistent
# grid: 2 workgroups per CU, 512 on an MI355X); the tally asserts fail on a device with another grid, they do not pass silently.
# Cost units per tile: D = 128 in 16 bit has depth 128; D = 17 in float32 has depth 32 at 16 units each, 512; D = 16 has depth 64 in 16
# bit.  Plus the epilogue: 128 sums (x bandwidths of a sweep), 2048 histogram, 1024 radius, 1536 k-NN keys (kad_tiles.h).
BUDGET_B = {   # (entry, dtype) -> budget                   tiles or units per launch -> launches of the largest pass
    ("median", "fp16"): 1 << 21,     # 2^21 / 2176 = 963    1081 -> 963 + 118
    ("median", "fp32"): 1 << 21,     # 2^21 / 2560 = 819    1081 -> 819 + 262
    ("kad", "fp16"): 1 << 18,        # 2^18 / 256 = 1024    1081 -> 1024 + 57 (the median's rounds: 120 tiles a launch)
    ("kad", "fp32"): 1 << 19,        # 2^19 / 640 = 819     1081 -> 819 + 262
    ("sweep", "fp16"): 1 << 19,      # 2^19 / 640 = 819     1081 -> 819 + 262
    ("sweep", "fp32"): 1 << 20,      # 2^20 / 1024 = 1024   1081 -> 1024 + 57
    ("prdc", "fp16"): 1 << 20,       # 2^20 / 1152 = 910    the radius pass of x, 2116 units -> 910 + 910 + 296
    ("prdc", "fp32"): 1 << 20,       # 2^20 / 1536 = 682    2116 -> 682 + 682 + 682 + 70
    ("nearest", "fp16"): 700000,     # radius 607 units a launch (2116 -> 4 launches); cross 420 (506 -> 420 + 86)
    ("nearest", "fp32"): 900000,     # radius 585 (2116 -> 4 launches); cross 439 (506 -> 439 + 67)
    ("nn_test", "fp16"): 1 << 20,    # 2^20 / 1664 = 630    3136 units of Z x Z -> 5 launches
    ("nn_test", "fp32"): 1 << 21,    # 2^21 / 2048 = 1024   3136 -> 4 launches
    ("kid", "fp16"): 1 << 17,        # 2^17 / 192 = 682     1081 -> 682 + 399
    ("kid", "fp32"): 1 << 19,        # 2^19 / 640 = 819     1081 -> 819 + 262
}


@pytest.mark.parametrize("dt,d", CASES_B, ids=[c[0] for c in CASES_B])
def test_regime_b_median_distance(monkeypatch, dt, d):
    _check_median(monkeypatch, _tally_b, dt, d, None, N_B, BUDGET_B["median", dt])


@pytest.mark.parametrize("kernel", ["gaussian", "imq"])
@pytest.mark.parametrize("dt,d", CASES_B, ids=[c[0] for c in CASES_B])
def test_regime_b_kad(monkeypatch, distances, dt, d, kernel):
    distances(gemm=True)
    _check_kad(monkeypatch, _tally_b, dt, d, None, N_B, M_B, BUDGET_B["kad", dt], kernel)


@pytest.mark.parametrize("dt,d", CASES_B, ids=[c[0] for c in CASES_B])
def test_regime_b_kad_sweep(monkeypatch, distances, dt, d):
    distances(gemm=True)
    _check_sweep(monkeypatch, _tally_b, dt, d, None, N_B, M_B, BUDGET_B["sweep", dt], 4)


@pytest.mark.parametrize("dt,d", CASES_B, ids=[c[0] for c in CASES_B])
def test_regime_b_prdc(monkeypatch, distances, dt, d):
    distances(gemm=True)
    _check_prdc(monkeypatch, _tally_b, dt, d, None, N_B, M_B, BUDGET_B["prdc", dt])


@pytest.mark.parametrize("dt,d", CASES_B, ids=[c[0] for c in CASES_B])
def test_regime_b_nearest(monkeypatch, distances, dt, d):
    """The cross pass has 46 x 11 = 506 units, fewer than the 513 a second slot needs: the budget cuts it in two launches, and it is
    the radius pass (2116 units) whose workgroups walk two slots."""
    distances(gemm=True)
    _check_nearest(monkeypatch, _tally_b, dt, d, None, N_B, M_B, BUDGET_B["nearest", dt], 5)


@pytest.mark.parametrize("dt,d", CASES_B, ids=[c[0] for c in CASES_B])
def test_regime_b_nn_test(monkeypatch, distances, dt, d):
    distances(gemm=True)
    _check_nn_test(monkeypatch, _tally_b, dt, d, None, N_B, M_B, BUDGET_B["nn_test", dt], 1)


@pytest.mark.parametrize("dt", [c[0] for c in CASES_B])
def test_regime_b_kid(monkeypatch, dt):
    _check_kid(monkeypatch, _tally_b, dt, None, N_B, M_B, BUDGET_B["kid", dt])


# ------------------------------------------------------------------------------------------------------------------ refusals
SENTINEL = -12345.5


def _raw_kad(x, y):
    from fadtk_amd import _capi
    res = _capi.FadKadResult()
    res.mmd2 = res.kxx_mean = res.bandwidth = SENTINEL
    st = _capi.load_library().fad_kad_k(x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, y.shape[0], y.shape[1], x.shape[1],
                                        _capi.FAD_F32, 0, 0.0, _capi.FAD_KAD_GAUSSIAN, C.byref(res), 0, None)
    return st, bool(res.mmd2 == SENTINEL and res.kxx_mean == SENTINEL and res.bandwidth == SENTINEL)


def _raw_prdc(x, y, k=5):
    from fadtk_amd import _capi
    res = _capi.FadPrdcResult()
    res.precision = res.coverage = SENTINEL
    arrays = [np.full(x.shape[0], SENTINEL, np.float32), np.full(y.shape[0], SENTINEL, np.float32), np.full(y.shape[0], -7, np.int32),
              np.full(x.shape[0], -7, np.int32)]
    det = _capi.FadPrdcDetail(*(a.ctypes.data for a in arrays))
    st = _capi.load_library().fad_prdc(x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, y.shape[0], y.shape[1], x.shape[1],
                                       _capi.FAD_F32, 0, k, C.byref(res), C.byref(det), 0, None)
    untouched = bool(res.precision == SENTINEL and res.coverage == SENTINEL and (arrays[0] == SENTINEL).all()
                     and (arrays[1] == SENTINEL).all() and (arrays[2] == -7).all() and (arrays[3] == -7).all())
    return st, untouched


def test_regime_a_refusals_leave_the_outputs_untouched_and_the_next_call_is_right(monkeypatch, distances):
    """One NaN row under the cut.  fad_kad, fad_prdc and fad_nn_test refuse on the norms, before they plan a pass (an empty tally);
    fad_kid_subsets learns of it from its sums, after its cut pass."""
    import torch
    from fadtk_amd import hip
    distances()
    d = 17
    xv, yv = _gauss(N_A, M_A, d, "fp32")
    bad = xv.copy()
    bad[777, 3] = np.nan
    u = hip.pack_labels(_labels(N_A, M_A))
    ix, iy = KID.exact_indices(N_A, M_A, 17, 129, seed=17)
    ix[5, 7] = 777
    monkeypatch.setenv(ENV, "1")
    assert _raw_kad(bad, yv) == (NOT_FINITE, True) and hip.kad_last_plan()["passes"] == 0
    assert _raw_kad(yv, bad) == (NOT_FINITE, True)
    assert _raw_prdc(bad, yv) == (NOT_FINITE, True) and hip.kad_last_plan()["passes"] == 0
    st, untouched, msg = TNN._raw(torch.from_numpy(bad).cuda(), torch.from_numpy(yv).cuda(), u, 5)
    assert st == NOT_FINITE and untouched and hip.kad_last_plan()["passes"] == 0, msg
    assert TKID._raw_subsets(bad, yv, ix, iy, 129, 17) == (NOT_FINITE, True)
    _tally_a(hip.kad_last_plan())
    cut = hip.kad(xv, yv)                                   # the call after the refusals, still cut
    _tally_a(hip.kad_last_plan())
    monkeypatch.delenv(ENV)
    got = hip.kad(xv, yv)                                   # and the next one with the variable unset: one launch per pass, and right
    plan = hip.kad_last_plan()
    assert plan["passes"] == 4 and plan["max_launches"] == 1, plan
    errs = TK._check(got, KR.kad(xv, yv, got["bandwidth"], "gaussian"), "after the refusals")
    _line("refusals, then kad", "fp32", "unset", plan, max(errs.values()), _means_near_uncut(cut, got))
    for bad_budget in ("", "0", "-3", "12x", "1e6", " "):   # unset, empty, unparsable or <= 0: the default
        monkeypatch.setenv(ENV, bad_budget)
        assert hip.kad(xv, yv) == got and hip.kad_last_plan() == plan, bad_budget


# ------------------------------------------------------------------------------------------- the production budget, no variable
def test_production_budget_cuts_the_triangle_of_32769_float32_rows_at_d_2048(monkeypatch):
    """fad_kad on float32 device rows, D = 2048, n = 32 769, m = 129, a given bandwidth (no median).  A tile costs 16 * 2048 + 128 units,
    so a launch holds 2^30 / 32 896 = 32 640 tiles and the baseline's triangle of 257 blocks (33 153 tiles) takes two.  If the constants
    of kad_tiles.h move, the tally assert says so and the shape moves with them.  Reference: torch float64 on the GPU, as the config-3
    tests.  On an MI355X the whole call (pack, four launches, read-back) takes 20 ms and the test 0.6 s (profiles/kad_cut_err.txt)."""
    import torch
    from fadtk_amd import hip
    monkeypatch.delenv(ENV, raising=False)
    n, m, d, sigma = 32769, 129, 2048, 64.0                 # |x - y|^2 is about 2 D = 64^2
    gen = torch.Generator(device="cuda").manual_seed(2048)
    x = torch.randn((n, d), generator=gen, device="cuda")
    y = torch.randn((m, d), generator=gen, device="cuda") * 1.05 + 0.02
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = hip.kad(x, y, bandwidth=sigma)
    t_call = time.perf_counter() - t0
    plan = hip.kad_last_plan()
    assert plan["passes"] == 3 and plan["max_launches"] == 2 and plan["min_launches"] == 1 and plan["launches"] == 4, plan
    assert plan["slots_per_workgroup"] >= 2, plan
    t0 = time.perf_counter()
    want, _ = TK._torch_means_f64(x.double(), y.double(), sigma, chunk=2048)
    t_ref = time.perf_counter() - t0
    errs = TK._check(got, want, "production budget f32 32769 x 2048")
    assert got["bandwidth"] == sigma and got["n"] == n and got["m"] == m
    _line("kad production budget", "fp32", "unset", plan, max(errs.values()), 0.0)
    print(f"[kad-cut] kad production budget: the call {t_call * 1e3:.0f} ms (pack, 4 launches, read-back), the float64 reference {t_ref:.2f} s")
