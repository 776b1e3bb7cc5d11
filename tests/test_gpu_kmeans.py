"""Lloyd's k-means on the GPU (fad_kmeans, csrc/kad.hip and csrc/kmeans_update.h) against the float64 reference of
tests/kmeans_reference.py on the same row values, upcast.  Three stages, each held on its own so that the reference follows the
device's trajectory and no near-tie can make a test vacuous:
  assignment (max_iter = 0): exact on integer rows with integer and dyadic centroids; on Gaussian rows with float32 centroids that the
      row dtype cannot hold, every label, distance and tie inside the bracket of tau = 1.3e-5;
  update (max_iter = 1): the returned centroids are the float64 means under the labels the device itself returned for the init;
  loop: max_iter = T equals the chain of T single-step calls bit for bit, on a second run, and under a launch cut.
"""
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
_spec = importlib.util.spec_from_file_location("kmeans_reference", Path(__file__).resolve().parent / "kmeans_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

# Margin of one float32 d^2 against float64, relative to |x|^2 + |c|^2: the project's bound for this main loop.
TAU = 1.3e-5


def _cast(a, dt):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"fp16": t.half(), "bf16": t.bfloat16(), "fp32": t}[dt]


def _host(t):
    return t.float().cpu().numpy().astype(np.float64)


def _wide(t, pad, device):
    """the rows of t inside a wider matrix (ld = D + pad), on the host (numpy where numpy has the dtype) or on the device"""
    import torch
    w = torch.zeros((t.shape[0], t.shape[1] + pad), dtype=t.dtype)
    w[:, : t.shape[1]] = t
    if device:
        return w.cuda()[:, : t.shape[1]]
    if t.dtype == torch.bfloat16:
        return w[:, : t.shape[1]]
    return w.numpy()[:, : t.shape[1]]


# ------------------------------------------------------------------------------------------------------------------ assignment
EXACT = [  # N, K, D
    (1, 1, 1), (2, 2, 3), (127, 127, 17), (127, 2, 1), (129, 128, 128), (1001, 129, 130), (1001, 300, 3), (3000, 300, 512),
    (300, 300, 17), (129, 127, 512), (1001, 1, 17), (3000, 128, 1),
]


def _exact_case(n, k, d, seed):
    """integer rows in [-3, 3]; centroids integer (rows among them) or dyadic (halves), with duplicates"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    c = (rng.integers(-6, 7, size=(k, d)) / 2.0).astype(np.float32)
    take = rng.choice(n, size=min(n, max(1, k // 2)), replace=False)
    c[: len(take)] = x[take]                                   # rows equal to centroids: d^2 = 0
    if k > 1:
        c[k - 1] = c[0]                                        # duplicate centroids: the smaller index wins
    if k > 3:
        c[k // 2] = c[1]
    if n > 2:
        x[n - 1] = x[0]                                        # duplicate rows
    return x, c


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,k,d", EXACT)
def test_assignment_exact_on_integer_rows(n, k, d, dt):
    from fadtk_amd import hip
    x, c = _exact_case(n, k, d, seed=n * 7 + k * 3 + d)
    xt = _cast(x, dt)
    rows = _wide(xt, 8 if (n + k) % 2 else 0, device=(n + d) % 2 == 1)                # host and device rows, ld > D and ld == D
    got = hip.kmeans(rows, c, iterations=0)
    labels, d2, _ = R.assign(_host(xt), c)
    np.testing.assert_array_equal(got["labels"], labels)
    np.testing.assert_array_equal(got["dist2"].astype(np.float64), d2)
    np.testing.assert_array_equal(got["counts"], np.bincount(labels, minlength=k))
    assert got["inertia"] == d2.sum() and list(got["inertia_trace"]) == [d2.sum()]
    np.testing.assert_array_equal(got["centroids"], c)                                # a pure assignment returns the init
    assert (got["iterations"], got["converged"], got["changed_last"], got["assignments"]) == (0, 0, -1, 1)
    assert got["empty_clusters"] == int((np.bincount(labels, minlength=k) == 0).sum())
    assert (got["n"], got["k"]) == (n, k)
    if k > 1:
        assert got["counts"][k - 1] == 0                                              # the duplicate of centroid 0 never wins
    plan = hip.kmeans_last_plan()
    assert plan["planes"] == {"fp16": 2, "bf16": 3, "fp32": 1}[dt] and plan["assign_launches"] >= 1 and plan["assignments"] == 1


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
def test_pooled_sets_equal_the_concatenated_set(dt):
    import torch
    from fadtk_amd import hip
    rng = np.random.default_rng(5)
    x = _cast(rng.standard_normal((700, 40)).astype(np.float32) * 2, dt)
    init = x[R.seed_rows(700, 33, 0, 0)].float().numpy()
    one = hip.kmeans(x.cuda(), init, iterations=2)
    for cuts in ((129,), (1, 400)):
        parts = [p.cuda() for p in torch.tensor_split(x, cuts)]
        parts[0] = _wide(parts[0].cpu(), 24, device=True)                              # sets of different row pitches
        got = hip.kmeans(parts, init, iterations=2)
        for key in ("labels", "dist2", "centroids", "counts", "inertia_trace"):
            np.testing.assert_array_equal(got[key], one[key], err_msg=key)
        assert got["inertia"] == one["inertia"]
    host = hip.kmeans([p if dt == "bf16" else p.numpy() for p in torch.tensor_split(x, (300,))], init, iterations=2)
    np.testing.assert_array_equal(host["labels"], one["labels"])
    np.testing.assert_array_equal(host["centroids"], one["centroids"])


def _blobs(n, k, d, seed, dt):
    """standard normal rows around blob centres of scale <= 6, in the row dtype; entries below 2^-7 are set to 0 so that a float16
    row times 2^-6 is still exact (float16's subnormal spacing is 2^-24)"""
    rng = np.random.default_rng(seed)
    scale = min(6.0, 12.0 / np.sqrt(d))
    centres = rng.standard_normal((max(2, k // 3), d)) * scale
    x = (rng.standard_normal((n, d)) + centres[rng.integers(0, len(centres), n)]).astype(np.float32)
    x[np.abs(x) < 2.0 ** -7] = 0.0
    return _cast(x, dt)


_GAUSS = {}


def _gauss_case(n, k, d, dt):
    """-> (rows, x64, float32 means that the row dtype cannot hold (one reference update from K rows), the reference's d^2 [N, K])"""
    key = (n, k, d, dt)
    if key not in _GAUSS:
        xt = _blobs(n, k, d, seed=n + k + d, dt=dt)
        x64 = _host(xt)
        init = x64[R.seed_rows(n, k, 1, 0)].astype(np.float32)
        labels0, _, _ = R.assign(x64, init)
        cent, _ = R.update(x64, labels0, init)
        d2 = R.dist2(x64, cent)
        d2.setflags(write=False)
        _GAUSS[key] = (xt, x64, cent, d2)
    return _GAUSS[key]


GAUSS = [(1001, 20, 17), (3000, 300, 128), (1001, 129, 512), (777, 40, 130)]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,k,d", GAUSS)
def test_assignment_gaussian_rows_inside_the_bracket(n, k, d, dt):
    from fadtk_amd import hip
    xt, x64, cent, d2 = _gauss_case(n, k, d, dt)
    if dt != "fp32":              # the test is about centroids the rows' dtype cannot hold: all but those of one-row clusters (and chance)
        assert (_host(_cast(cent, dt)) != cent.astype(np.float64)).mean() > 0.5
    got = hip.kmeans(_wide(xt, 8, device=True), cent, iterations=0)
    lab = got["labels"].astype(np.int64)
    sx, sc = (x64 ** 2).sum(1), (cent.astype(np.float64) ** 2).sum(1)
    marg = TAU * (sx[:, None] + sc[None, :])
    rows = np.arange(n)
    best = d2.min(1)
    err = np.abs(got["dist2"].astype(np.float64) - d2[rows, lab]) / (sx + sc[lab])
    print(f"[kmeans-err] {dt} N={n} K={k} D={d}: d2 {err.max():.2e}")
    assert err.max() <= TAU, float(err.max())
    assert (d2[rows, lab] <= best + marg[rows, lab]).all()
    inside = (d2 <= best[:, None] + 2 * marg).sum(1)
    sure = inside == 1
    print(f"[kmeans-err] {dt} N={n} K={k} D={d}: ambiguous rows {(~sure).mean():.4f}")
    assert (~sure).mean() <= 0.05
    np.testing.assert_array_equal(lab[sure], d2.argmin(1)[sure])
    # rows and centroids times 2^6 and 2^-6: every label kept
    import torch
    for s in (64.0, 1.0 / 64.0):
        scaled = (xt.float() * s).to(xt.dtype)
        assert torch.equal(scaled.float(), xt.float() * s)                            # the scaling itself is exact
        again = hip.kmeans(scaled.cuda(), cent * np.float32(s), iterations=0)
        np.testing.assert_array_equal(again["labels"], got["labels"], err_msg=f"scale {s}")


def test_a_centroid_rounded_to_float16_misses_the_bracket():
    """What the planes are for: with the centroids rounded to the rows' dtype, the exact d^2 itself leaves the bracket (4.7 TAU on
    this case, before any float32 accumulation error; the planes' largest error above is 0.05 TAU), so the bracket test does hold the
    planes to account.  Host arithmetic only."""
    xt, x64, cent, d2 = _gauss_case(1001, 129, 512, "fp16")
    rounded = _host(_cast(cent, "fp16"))
    sx, sc = (x64 ** 2).sum(1), (cent.astype(np.float64) ** 2).sum(1)
    err = np.abs(R.dist2(x64, rounded) - d2) / (sx[:, None] + sc[None, :])
    print(f"[kmeans-err] centroids rounded to fp16: d2 {err.max():.2e}")
    assert err.max() > TAU


# ---------------------------------------------------------------------------------------------------------------------- update
def _ulp32(a):
    a = np.abs(np.asarray(a, dtype=np.float32))
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def _check_update(got_first, got, x64, init):
    """got = the call with max_iter = 1 from init; got_first = the pure assignment against init: the device's own A_1"""
    labels = got_first["labels"].astype(np.int64)
    k = init.shape[0]
    counts = np.bincount(labels, minlength=k)
    want = np.array(init, dtype=np.float64)
    for j in np.flatnonzero(counts):
        want[j] = x64[labels == j].sum(0) / counts[j]
    tol = _ulp32(want.astype(np.float32)) + counts[:, None] * 2.0 ** -52 * np.abs(x64).max()
    assert (np.abs(got["centroids"].astype(np.float64) - want) <= tol).all()
    empty = counts == 0
    np.testing.assert_array_equal(got["centroids"][empty], init[empty])               # an empty cluster keeps its bits
    return counts


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,k,d", [(1001, 20, 17), (3000, 300, 128), (777, 40, 130), (500, 500, 3)])
def test_update_is_the_float64_mean_of_the_device_labels(n, k, d, dt):
    from fadtk_amd import hip
    xt = _blobs(n, k, d, seed=3 * n + d, dt=dt)
    x64 = _host(xt)
    init = x64[R.seed_rows(n, k, 2, 0)].astype(np.float32)
    first = hip.kmeans(xt.cuda(), init, iterations=0)
    got = hip.kmeans(xt.cuda(), init, iterations=1)
    _check_update(first, got, x64, init)
    assert got["iterations"] == 1 and got["assignments"] == 2 and got["inertia_trace"][0] == first["inertia"]
    again = hip.kmeans(xt.cuda(), got["centroids"], iterations=0)                     # the labels belong to the returned centroids
    np.testing.assert_array_equal(again["labels"], got["labels"])
    np.testing.assert_array_equal(again["dist2"], got["dist2"])


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
def test_update_cluster_shapes_and_exact_integer_means(dt):
    """Clusters of chunk - 1, chunk, chunk + 1 and several chunks of rows, single-row clusters and an init centroid far from every row:
    integer rows on separated integer sites, so every mean is exact."""
    from fadtk_amd import hip
    chunk = 64
    sizes = [chunk - 1, chunk, chunk + 1, 5 * chunk + 7, 1, 1, 1, 2 * chunk]
    rng = np.random.default_rng(11)
    d = 19
    sites = (np.arange(len(sizes))[:, None] * 40 + np.zeros((1, d))).astype(np.float32)             # 40 apart in every coordinate
    parts = [sites[j] + rng.integers(-3, 4, size=(s, d)) for j, s in enumerate(sizes)]
    order = rng.permutation(sum(sizes))
    x = np.concatenate(parts, 0).astype(np.float32)[order]
    truth = np.concatenate([np.full(s, j) for j, s in enumerate(sizes)])[order]
    far = np.full((1, d), -900.0, np.float32)                                        # cluster 3 stays empty
    init = np.concatenate([sites[:3], far, sites[3:]], 0)
    want_labels = np.where(truth >= 3, truth + 1, truth)
    xt = _cast(x, dt)
    got = hip.kmeans(xt.numpy() if dt != "bf16" else xt, init, iterations=1)
    plan = hip.kmeans_last_plan()
    assert plan["chunk_rows"] == chunk and plan["max_chunks"] == 6 and plan["iterations"] == 1
    np.testing.assert_array_equal(got["labels"], want_labels)
    want, counts = R.update(_host(xt), want_labels, init)
    np.testing.assert_array_equal(got["centroids"], want)                             # sums of integers: exact
    np.testing.assert_array_equal(got["counts"], counts)
    assert got["empty_clusters"] == 1 and got["counts"][3] == 0
    assert got["centroids"][3].tobytes() == far[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------------ loop
def _chain(rows, init, steps):
    """`steps` single-step calls that hand the float32 centroids back in -> what one call with max_iter = steps must return"""
    from fadtk_amd import hip
    first = hip.kmeans(rows, init, iterations=0)
    prev, cent, trace = first["labels"], init, [first["inertia"]]
    out = None
    for t in range(1, steps + 1):
        # iteration t: A_t = prev (the assignment against `cent`); stop if it repeats A_{t-1}
        if out is not None and np.array_equal(prev, before):
            return {"labels": prev, "centroids": cent, "dist2": out["dist2"], "inertia_trace": np.array(trace), "iterations": t,
                    "converged": 1}
        step = hip.kmeans(rows, cent, iterations=1)
        assert step["inertia_trace"][0] == trace[-1]
        before, prev, cent, out = prev, step["labels"], step["centroids"], step
        trace.append(step["inertia"])
    if out is None:
        out = first
    return {"labels": prev, "centroids": cent, "dist2": out["dist2"], "inertia_trace": np.array(trace), "iterations": steps, "converged": 0}


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,k,d,steps", [(600, 7, 5, 8), (1001, 40, 17, 3), (900, 12, 130, 8), (300, 300, 3, 2)])
def test_loop_equals_the_chain_of_single_steps(n, k, d, steps, dt):
    from fadtk_amd import hip
    xt = _blobs(n, k, d, seed=n + steps, dt=dt)
    rows = xt.cuda()
    x64 = _host(xt)
    init = x64[R.seed_rows(n, k, 3, 0)].astype(np.float32)
    got = hip.kmeans(rows, init, iterations=steps)
    want = _chain(rows, init, steps)
    for key in ("labels", "centroids", "dist2", "inertia_trace"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert (got["iterations"], got["converged"]) == (want["iterations"], want["converged"])
    assert got["inertia"] == got["inertia_trace"][-1] and got["assignments"] == len(got["inertia_trace"])
    np.testing.assert_array_equal(got["counts"], np.bincount(got["labels"], minlength=k))
    # each single step of the chain is held to the two stages above
    first = hip.kmeans(rows, init, iterations=0)
    _check_update(first, hip.kmeans(rows, init, iterations=1), x64, init)
    if got["converged"]:                                                              # the fixed point: the centroids are the means of the labels
        assert got["changed_last"] == 0
        _check_update(got, hip.kmeans(rows, got["centroids"], iterations=1), x64, got["centroids"])
        np.testing.assert_array_equal(hip.kmeans(rows, got["centroids"], iterations=1)["centroids"], got["centroids"])
    second = hip.kmeans(rows, init, iterations=steps)                                 # the same bits on a second run
    for key in ("labels", "centroids", "dist2", "inertia_trace", "counts"):
        np.testing.assert_array_equal(second[key], got[key], err_msg=key)


def test_a_long_run_converges_to_the_fixed_point():
    from fadtk_amd import hip
    xt = _blobs(1500, 9, 8, seed=77, dt="fp16")
    x64 = _host(xt)
    init = x64[R.seed_rows(1500, 9, 0, 0)].astype(np.float32)
    got = hip.kmeans(xt.numpy(), init, iterations=100)
    assert got["converged"] == 1 and got["changed_last"] == 0 and got["iterations"] < 100
    assert (np.diff(got["inertia_trace"]) <= 1e-6 * got["inertia_trace"][:-1]).all()  # Lloyd's steps do not raise the inertia
    step = hip.kmeans(xt.numpy(), got["centroids"], iterations=1)
    np.testing.assert_array_equal(step["centroids"], got["centroids"])
    np.testing.assert_array_equal(step["labels"], got["labels"])


_CUT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from fadtk_amd import hip
d = np.load(sys.argv[2])
got = hip.kmeans(d["x"], d["init"], iterations=4)
plan = hip.kmeans_last_plan()
np.savez(sys.argv[3], launches=plan["assign_launches"], **{k: got[k] for k in ("labels", "centroids", "dist2", "inertia_trace", "counts")})
"""


def test_same_bits_under_a_launch_cut(tmp_path):
    """FAD_KAD_LAUNCH_BUDGET cuts the assignment into several launches (the plan says so first); labels, centroids, dist2 and the
    inertia trace keep their bits.  The variable is read per call; a child process keeps this one's environment as it is."""
    xt = _blobs(6000, 300, 24, seed=9, dt="fp16")
    x = xt.numpy()
    init = x[R.seed_rows(6000, 300, 4, 0)].astype(np.float32)
    np.savez(tmp_path / "in.npz", x=x, init=init)
    outs = []
    for name, budget in (("whole", ""), ("cut", "1")):
        env = dict(os.environ, FAD_KAD_LAUNCH_BUDGET=budget)
        r = subprocess.run([sys.executable, "-c", _CUT_SCRIPT, str(ROOT), str(tmp_path / "in.npz"), str(tmp_path / f"{name}.npz")], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(tmp_path / f"{name}.npz"))
    whole, cut = outs
    assert int(whole["launches"]) == 1 and int(cut["launches"]) > 1, (int(whole["launches"]), int(cut["launches"]))
    for key in ("labels", "centroids", "dist2", "inertia_trace", "counts"):
        np.testing.assert_array_equal(cut[key], whole[key], err_msg=key)


# -------------------------------------------------------------------------------------------------------------------- refusals
def _raw(sets, k, init, max_iter=1, dtype=None, d=None, lds=None, outputs=None):
    from fadtk_amd import _capi
    lib = _capi.load_library()
    S = len(sets)
    ptrs = (C.c_void_p * S)(*[s.ctypes.data for s in sets])
    ns = (C.c_int64 * S)(*[s.shape[0] for s in sets])
    ld = (C.c_int64 * S)(*(lds or [s.shape[1] for s in sets]))
    d = sets[0].shape[1] if d is None else d
    N = sum(s.shape[0] for s in sets)
    cent, lab, cnt = outputs or (np.full((max(k, 1), d), 7, np.float32), np.full(N, 7, np.int32), np.full(max(k, 1), 7, np.int64))
    res = _capi.FadKmeansResult()
    st = lib.fad_kmeans(ptrs, ns, ld, S, d, _capi.FAD_F32 if dtype is None else dtype, 0, k, init.ctypes.data if init is not None else None,
                        max_iter, cent.ctypes.data, lab.ctypes.data, cnt.ctypes.data, None, None, C.byref(res), 0, None)
    return st, (cent, lab, cnt), res


def test_refusals_leave_the_outputs_untouched():
    from fadtk_amd import _capi, hip
    rng = np.random.default_rng(0)
    x = rng.standard_normal((200, 12)).astype(np.float32)
    init = x[:5].copy()
    st, outs, res = _raw([x], 5, init)
    assert st == _capi.FAD_OK and res.n == 200 and res.k == 5 and (outs[1] != 7).any()
    bad = x.copy()
    bad[77, 3] = np.nan
    binit = init.copy()
    binit[2, 2] = np.inf
    cases = [
        (dict(sets=[bad], k=5, init=init), _capi.FAD_ERR_NOT_FINITE),
        (dict(sets=[x, bad], k=5, init=init), _capi.FAD_ERR_NOT_FINITE),
        (dict(sets=[x], k=5, init=binit), _capi.FAD_ERR_NOT_FINITE),
        (dict(sets=[x], k=0, init=init), _capi.FAD_ERR_INVALID),
        (dict(sets=[x], k=201, init=np.zeros((201, 12), np.float32)), _capi.FAD_ERR_INVALID),
        (dict(sets=[x], k=5, init=None), _capi.FAD_ERR_INVALID),
        (dict(sets=[x], k=5, init=init, max_iter=-1), _capi.FAD_ERR_INVALID),
        (dict(sets=[x], k=5, init=init, lds=[11]), _capi.FAD_ERR_INVALID),
        (dict(sets=[x], k=5, init=init, dtype=_capi.FAD_F64), _capi.FAD_ERR_INVALID),
        (dict(sets=[x] * 9, k=5, init=init), _capi.FAD_ERR_INVALID),
        (dict(sets=[x, x[:0]], k=5, init=init), _capi.FAD_ERR_TOO_FEW_ROWS),
    ]
    for kw, want in cases:
        st, outs, _ = _raw(**kw)
        assert st == want, (kw.keys(), st, want)
        assert all((o == 7).all() for o in outs)
        assert hip.kmeans_last_plan()["planes"] == 0
    # float16 rows: an init entry far past the rows' range cannot be carried by float16 planes
    h = x.astype(np.float16)
    huge = init.copy()
    huge[0, 0] = 1e6
    st, outs, _ = _raw([h], 5, huge, dtype=_capi.FAD_F16)
    assert st == _capi.FAD_ERR_NOT_FINITE and all((o == 7).all() for o in outs)
