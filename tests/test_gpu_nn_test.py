"""Leave-one-out k-NN two-sample test on the GPU (fad_nn_test, csrc/kad.hip and csrc/nn_vote.h) against the float64 reference of
tests/nn_test_reference.py on the same 16-bit values, upcast: exact on integer rows (ties by index, duplicates inside and across the
sets, k up to N - 1), valid self-excluded k-NN lists inside nearest_reference's bracket on Gaussian rows with the votes recomputed
from the returned graph, consistency with fad_nearest, power and direction through the public function, determinism, refusals that
leave every output untouched, and the command line end to end."""
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


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NT = _load("nn_test_reference")
AR = _load("kad_aggregate_reference")
PR = NT.PR

# Margin of one float32 d^2 against float64, relative to |z_i|^2 + |z_j|^2: test_gpu_nearest.py's constant, for the same arithmetic.
TAU = 1.3e-5
P_WORDS = 70                                                   # three labelling words, the last partial (with the observed one: 71)


def _cast(a, dt):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"fp16": t.half(), "bf16": t.bfloat16(), "fp32": t}[dt]


def _host(t):
    return t.float().numpy().astype(np.float64)


def _arg(t, dt):
    """numpy on the host for fp16 / fp32, a torch device tensor for bf16 (numpy has no bfloat16)"""
    return t.cuda() if dt == "bf16" else t.numpy()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _int_rows(rng, n, d, dups):
    a = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    for i, j in dups:
        if i < n and j < n:
            a[j] = a[i]
    return a


def _same(got, want, n, m):
    """counts, accuracies and p-values of a hip.nn_test result against nn_test_reference.results, exactly"""
    np.testing.assert_array_equal(got["null_correct_x"], want["null_correct_x"])
    np.testing.assert_array_equal(got["null_correct_y"], want["null_correct_y"])
    for key in ("correct_x", "correct_y", "accuracy", "accuracy_x", "accuracy_y", "p_value", "p_value_low"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert (got["n"], got["m"]) == (n, m)


EXACT = [  # n, m, d, k
    (3, 2, 1, 3),            # k = N - 2
    (2, 2, 3, 3),            # k = N - 1
    (100, 29, 17, 1),        # N = 129: the set boundary inside a tile, two row ranges
    (128, 128, 128, 5),
    (257, 130, 130, 15),     # the list bucket of 16
    (640, 361, 128, 7),      # the bucket of 8; N = 1001
]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,m,d,k", EXACT)
def test_nn_test_exact_on_integer_rows(n, m, d, k, dt):
    from fadtk_amd import hip
    rng = np.random.default_rng(n * 5 + m * 3 + d + k)
    x = _int_rows(rng, n, d, [(0, 1), (3, n - 1), (2, n // 2)])               # duplicates inside x ...
    y = _int_rows(rng, m, d, [(1, 0)])                                         # ... inside y ...
    for j, i in ((0, 1), (2, n - 1), (m - 1, n // 2), (m // 2, 0)):            # ... and across them
        if j < m:
            y[j] = x[i]
    u = PR.random_labellings(n, m, P_WORDS, rng)
    xt, yt = _cast(x, dt), _cast(y, dt)
    got = hip.nn_test(_arg(xt, dt), _arg(yt, dt), hip.pack_labels(u), k=k, return_graph=True)
    want = NT.reference(_host(xt), _host(yt), u, k)
    np.testing.assert_array_equal(_np(got["index"]), want["index"])
    np.testing.assert_array_equal(_np(got["dist2"]).astype(np.float64), want["dist2"])
    _same(got, want, n, m)
    assert got["k"] == k


def test_nn_test_hand_written_line():
    from fadtk_amd import hip
    for k in (1, 3):
        got = hip.nn_test(NT.LINE_X, NT.LINE_Y, NT.LINE_U, k=k, return_graph=True)
        assert got["index"].tolist() == NT.LINE_GRAPH[k] and got["dist2"].tolist() == NT.LINE_DIST2[k]
        assert (got["correct_x"], got["correct_y"]) == NT.LINE_COUNTS[k][0]
        assert (int(got["null_correct_x"][0]), int(got["null_correct_y"][0])) == NT.LINE_COUNTS[k][1]


def _gauss(n, m, d, seed, noise=0.5):
    """x standard normal; a third of y near copies of x rows, the rest fresh rows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * 1.05 + 0.03).astype(np.float32)
    near = rng.choice(n, size=m // 3, replace=False) if m // 3 <= n else rng.integers(0, n, m // 3)
    y[: m // 3] = x[near] + noise * rng.standard_normal((m // 3, d)).astype(np.float32)
    return x, y


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,m,d,k", [(1100, 900, 128, 5), (777, 1301, 512, 3), (641, 1029, 1024, 1), (1500, 500, 768, 15)])
def test_nn_test_gaussian_rows_inside_the_bracket(n, m, d, k, dt):
    import torch
    from fadtk_amd import hip
    x, y = _gauss(n, m, d, seed=n + d)
    xt, yt = _cast(x, dt), _cast(y, dt)
    wide_x = torch.zeros((n, d + 24), dtype=xt.dtype, device="cuda")           # ld > D on one side
    wide_x[:, :d] = xt.cuda()
    u = PR.random_labellings(n, m, P_WORDS, np.random.default_rng(n + m))
    got = hip.nn_test(wide_x[:, :d], yt.cuda(), hip.pack_labels(u), k=k, return_graph=True)
    idx, d2 = _np(got["index"]).astype(np.int64), _np(got["dist2"])
    label = f"{dt} n={n} m={m} D={d} k={k}"
    br = NT.bracket(_host(xt), _host(yt), TAU)
    assert ((idx >= 0) & (idx < n + m)).all() and (idx != np.arange(n + m)[:, None]).all(), label      # no row its own neighbour
    err = np.abs(d2.astype(np.float64) - np.take_along_axis(br["d2"], idx, 1)) / (br["norms"][:, None] + br["norms"][idx])
    print(f"[nn-test-err] {label}: d2 {err.max():.2e}")
    assert err.max() <= TAU, (label, float(err.max()))
    ok = NT.valid_graph(idx, d2, br, k)
    assert ok.all(), (label, np.flatnonzero(~ok)[:10])                         # a valid self-excluded k-NN of every row
    _same(got, NT.results(idx, n, m, u), n, m)                                 # the votes on the RETURNED graph, exactly


def test_nn_test_is_consistent_with_fad_nearest():
    from fadtk_amd import hip
    n, m, k = 300, 200, 5
    x, y = _gauss(n, m, 64, seed=3)
    x16, y16 = x.astype(np.float16), y.astype(np.float16)
    u = hip.pack_labels(PR.random_labellings(n, m, 5, np.random.default_rng(0)))
    mine = hip.nn_test(x16, y16, u, k=k, return_graph=True)
    near = hip.nearest(x16, y16, k=k, authenticity=False)
    seen = 0
    for j in range(m):                                                         # y_j's baseline neighbours: a prefix of fad_nearest's list
        keep = mine["index"][n + j] < n
        sub, sd = mine["index"][n + j][keep], mine["dist2"][n + j][keep]
        assert sub.tolist() == near["index"][j][: len(sub)].tolist(), j
        assert sd.tobytes() == near["dist2"][j][: len(sub)].tobytes(), j
        seen += len(sub)
    assert 0 < seen < m * k                                                    # both kinds of neighbour occur
    # every evaluation row's nearest pooled row is a baseline row: the very index and bits of fad_nearest
    rng = np.random.default_rng(5)
    yc = (x[rng.choice(n, size=m, replace=False)] + 0.01 * rng.standard_normal((m, 64))).astype(np.float16)
    one = hip.nn_test(x16, yc, u, k=1, return_graph=True)
    ref = hip.nearest(x16, yc, k=1, authenticity=False)
    assert (one["index"][n:, 0] < n).all()
    assert one["index"][n:, 0].tobytes() == ref["index"][:, 0].tobytes()
    assert one["dist2"][n:, 0].tobytes() == ref["dist2"][:, 0].tobytes()


def test_nn_test_power_and_direction_through_the_public_function():
    from fadtk_amd import calc_nearest_neighbour_test as calc
    x, y, u = AR.blobs_case()
    given = calc(x, y, k=5, labels=u)
    assert given["p_value"] <= 0.05 and given["accuracy"] > 0.55 and given["seed"] is None and given["permutations"] == 199
    drawn = calc(x, y, k=5, permutations=199, seed=5, return_labels=True)
    assert drawn["p_value"] <= 0.05 and drawn["seed"] == 5 and tuple(drawn["labels"].shape) == (199, 25)
    for key in ("accuracy", "accuracy_baseline", "accuracy_eval"):             # the observed labelling does not depend on the draws
        assert drawn[key] == given[key]
    assert drawn["null"].dtype == np.float64 and drawn["null"].shape == (199,)
    np.testing.assert_array_equal(drawn["null"], (drawn["null_correct_baseline"] + drawn["null_correct_eval"]) / 800.0)
    xc, yc, uc = NT.near_copies_case()
    low = calc(xc, yc, k=1, labels=uc, return_graph=True)
    assert low["p_value_low"] <= 0.05 and low["accuracy_eval"] == 0.0 and low["accuracy"] < 0.25 and low["p_value"] == 1.0
    assert low["index"].shape == (500, 1) and low["dist2"].dtype == np.float32
    assert (low["n"], low["m"], low["k"]) == (300, 200, 1)


def test_nn_test_deterministic_numpy_equals_torch_and_host_labels_equal_device_labels():
    import torch
    from fadtk_amd import hip
    n, m, k = 1500, 1100, 5
    x, y = _gauss(n, m, 256, seed=4)
    x16, y16 = x.astype(np.float16), y.astype(np.float16)
    u = hip.pack_labels(PR.random_labellings(n, m, 100, np.random.default_rng(1)))
    a = hip.nn_test(x16, y16, u, k=k, return_graph=True)
    b = hip.nn_test(x16, y16, u, k=k, return_graph=True)
    c = hip.nn_test(torch.from_numpy(x16).cuda(), torch.from_numpy(y16).cuda(), u, k=k, return_graph=True)
    d = hip.nn_test(x16, y16, torch.from_numpy(u.view(np.int32)).cuda(), k=k, return_graph=True)
    assert hip.K._is_torch(c["index"]) and c["index"].is_cuda and c["dist2"].is_cuda
    for other in (b, c, d):
        for key in ("index", "dist2", "null_correct_x", "null_correct_y"):
            assert _np(a[key]).tobytes() == _np(other[key]).tobytes(), key
        for key in ("accuracy", "accuracy_x", "accuracy_y", "p_value", "p_value_low", "correct_x", "correct_y"):
            assert a[key] == other[key], key
    plain = hip.nn_test(x16, y16, u, k=k)                                      # without the graph: the same counts
    assert "index" not in plain and plain["null_correct_x"].tobytes() == a["null_correct_x"].tobytes()


def _raw(x, y, labels, k, labels_on_device=0):
    """the C call on torch device rows with sentinel outputs -> (status, outputs untouched, message)"""
    import torch
    from fadtk_amd import _capi
    lib = _capi.load_library()
    P, N = labels.shape[0], x.shape[0] + y.shape[0]
    res = _capi.FadNnTestResult()
    res.accuracy, res.k = -7.0, -7
    nx, ny = np.full(P, -7, np.int64), np.full(P, -7, np.int64)
    idx = torch.full((N * 16,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((N * 16,), -7.0, dtype=torch.float32, device="cuda")
    lp = labels.data_ptr() if labels_on_device else labels.ctypes.data
    st = lib.fad_nn_test(x.data_ptr(), x.shape[0], x.stride(0), y.data_ptr(), y.shape[0], y.stride(0), x.shape[1], _capi.FAD_F32, 1, k,
                         lp, P, labels_on_device, C.byref(res), nx.ctypes.data, ny.ctypes.data, idx.data_ptr(), d2.data_ptr(), 0,
                         _capi.current_stream_ptr(0))
    untouched = bool(res.accuracy == -7.0 and res.k == -7 and (nx == -7).all() and (ny == -7).all() and bool((idx == -7).all())
                     and bool((d2 == -7.0).all()))
    return st, untouched, lib.fad_last_error()


def test_nn_test_refusals_leave_the_outputs_untouched():
    import torch
    from fadtk_amd import _capi, hip
    n, m = 12, 9
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.standard_normal((m, 8)).astype(np.float32)).cuda()
    labels = hip.pack_labels(PR.random_labellings(n, m, 6, rng))
    for k in (2, 17, n + m):                                                   # even, past 15, and k = N
        st, untouched, msg = _raw(x, y, labels, k)
        assert st == _capi.FAD_ERR_INVALID and untouched, (k, msg)
    wrong = labels.copy()
    wrong[3, 0] ^= 1 << 20                                                     # row 20 flips: n + 1 or n - 1 ones
    st, untouched, msg = _raw(x, y, wrong, 3)
    assert st == _capi.FAD_ERR_INVALID and untouched and b"labelling 3" in msg, msg
    st, untouched, msg = _raw(x, y, torch.from_numpy(wrong.view(np.int32)).cuda(), 3, labels_on_device=1)      # counted on the device
    assert st == _capi.FAD_ERR_INVALID and untouched, msg
    bad = x.clone()
    bad[5, 2] = float("nan")
    st, untouched, msg = _raw(bad, y, labels, 3)
    assert st == _capi.FAD_ERR_NOT_FINITE and untouched, msg
    st, untouched, msg = _raw(x[:1], y, hip.pack_labels(PR.random_labellings(1, m, 6, rng)), 1)
    assert st == _capi.FAD_ERR_TOO_FEW_ROWS and untouched, msg
    st, untouched, _ = _raw(x, y, labels, 3)                                   # the call after the refusals
    assert st == _capi.FAD_OK and not untouched
    assert _raw(x, y, labels, 15)[0] == _capi.FAD_OK                           # the largest k


def _caches(tmp_path):
    """two directories whose every file has its embedding cache: a baseline of 6 songs and an eval set drawn somewhere else"""
    rng = np.random.default_rng(21)
    base, evl = tmp_path / "base", tmp_path / "evl"
    rows = {}
    for d, shift, count in ((base, 0.0, 6), (evl, 1.5, 5)):
        (d / "embeddings" / "vggish").mkdir(parents=True)
        rows[d] = 0
        for i in range(count):
            e = (shift + rng.standard_normal((20 + 3 * i, 128))).astype(np.float32)
            (d / f"s{i}.wav").write_bytes(b"")                     # the audio itself is never read
            np.save(d / "embeddings" / "vggish" / f"s{i}.npy", e)
            rows[d] += e.shape[0]
    return base, evl, rows[base], rows[evl]


def test_nn_test_cli_end_to_end(tmp_path):
    from fadtk_amd.nn_test import CSV_HEADER
    base, evl, n, m = _caches(tmp_path)
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    csv = tmp_path / "out" / "nn.csv"
    for k, seed in ((3, 1), (1, 2)):
        r = subprocess.run([sys.executable, "-m", "fadtk_amd.nn_test", "vggish", str(base), str(evl), str(csv), "-k", str(k), "-p", "99",
                            "--seed", str(seed), "-w", "2"], capture_output=True, text=True, cwd=tmp_path, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    lines = csv.read_text().splitlines()
    assert lines[0] + "\n" == CSV_HEADER and len(lines) == 3
    for line, (k, seed) in zip(lines[1:], ((3, 1), (1, 2))):
        row = dict(zip(CSV_HEADER.strip().split(","), line.split(",")))
        assert len(line.split(",")) == 13 and row["model"] == "vggish" and row["baseline"] == str(base) and row["eval"] == str(evl)
        assert (int(row["k"]), int(row["n"]), int(row["m"]), int(row["permutations"]), int(row["seed"])) == (k, n, m, 99, seed)
        acc, ab, ae = float(row["accuracy"]), float(row["accuracy_baseline"]), float(row["accuracy_eval"])
        assert round(acc * (n + m)) == round(ab * n) + round(ae * m)
        assert acc > 0.9 and float(row["p_value"]) == 0.01 and float(row["p_value_low"]) == 1.0      # a shift of 1.5 in 128 dimensions
