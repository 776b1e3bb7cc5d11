"""KAD permutation test over several bandwidths, aggregated, on the GPU (fad_kad_permutation_sweep, csrc/kad.hip).

Every entry of a sweep carries the bits of kad_permutation_test(bandwidth = sigma_b) on the same labellings (both calls
run the permutation pass as one launch at these sizes) over D, dtypes, kernels, bandwidth counts and labelling counts around the word
and walk edges; the statistics against the float64 reference within tau = 1e-2 of the reference null's spread; the aggregate against
tests/kad_aggregate_reference.py on the library's own statistics, exactly; the factor 1 against the pooled median; calibration and
power (the blobs pair); refusals that leave the outputs untouched; the config-3 size once."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


AR = _load("kad_aggregate_reference")
PR = AR.PR
TAU = 1e-2           # of the reference null's standard deviation, as tests/test_gpu_kad_permutation.py
N_ROWS, M_ROWS = 255, 257       # 512 pooled rows: 4 row blocks, 10 triangle tiles; n = 255 ends inside a label word and a tile


def _sets(n, m, d, dtype, seed, shift=0.1):
    import torch
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (rng.standard_normal((m, d)) * 1.05 + shift).astype(np.float32)
    if dtype == "bf16":
        xt, yt = torch.from_numpy(x).cuda().bfloat16(), torch.from_numpy(y).cuda().bfloat16()
        return xt, yt, xt.double().cpu().numpy(), yt.double().cpu().numpy()
    x, y = x.astype(np.float16 if dtype == "f16" else np.float32), y.astype(np.float16 if dtype == "f16" else np.float32)
    return x, y, x.astype(np.float64), y.astype(np.float64)


def _pooled_median(x, y):
    from fadtk_amd import hip
    if isinstance(x, np.ndarray):
        return hip.kad_median_distance(np.concatenate([x, y]))
    import torch
    return hip.kad_median_distance(torch.cat([x, y]))


def _ladder(med, B):
    """B distinct sigmas around the pooled median, 1/4 .. 4 of it"""
    return [float(med * 2.0 ** e) for e in (np.linspace(-2.0, 2.0, B) if B > 1 else [0.0])]


FIELDS = ("mmd2", "kxx_mean", "kyy_mean", "kxy_mean", "bandwidth")


def _assert_entries_are_the_single_calls(got, x, y, labels, kernel="gaussian", label=""):
    from fadtk_amd import hip
    for b, s in enumerate(got["bandwidth"]):
        one = hip.kad_permutation_test(x, y, labels, bandwidth=float(s), kernel=kernel)
        for k in FIELDS:
            assert got[k][b] == one[k], (label, b, k, got[k][b], one[k])
        assert got["null"][b].tobytes() == one["null"].tobytes(), (label, b, float(np.max(np.abs(got["null"][b] - one["null"]))))
        assert got["p_values"][b] == one["p_value"], (label, b)
    assert got["n"] == one["n"] and got["m"] == one["m"]


def _assert_aggregate_is_the_reference_on_own_statistics(got):
    t = np.concatenate([got["mmd2"][:, None], got["null"]], axis=1)
    pv, pa = AR.aggregate(t)
    assert got["p_values"].tolist() == pv.tolist() and got["p_aggregated"] == pa, (got["p_values"], pv, got["p_aggregated"], pa)


EQUAL_CASES = [  # (dtype, d, kernel, B, P)
    ("f16", 17, "gaussian", 4, 199), ("f16", 128, "gaussian", 4, 199), ("f16", 512, "gaussian", 4, 199),
    ("bf16", 128, "gaussian", 4, 199), ("f32", 128, "gaussian", 4, 199), ("f32", 17, "iq", 3, 300), ("bf16", 512, "imq", 2, 32),
    ("f16", 128, "iq", 4, 199), ("f16", 128, "imq", 4, 199),
    ("f16", 128, "gaussian", 1, 199), ("f16", 128, "gaussian", 2, 199), ("f16", 128, "gaussian", 3, 199), ("f16", 128, "gaussian", 5, 199),
    ("f16", 128, "gaussian", 9, 199), ("f16", 128, "gaussian", 16, 199),
    ("f16", 128, "gaussian", 4, 31), ("f16", 128, "gaussian", 4, 32), ("f16", 128, "gaussian", 4, 300), ("f16", 128, "gaussian", 16, 300),
    ("f32", 512, "gaussian", 5, 31),
]


@pytest.mark.parametrize("dtype,d,kernel,B,P", EQUAL_CASES)
def test_sweep_entries_carry_the_bits_of_the_single_test(dtype, d, kernel, B, P):
    from fadtk_amd import hip
    x, y, _, _ = _sets(N_ROWS, M_ROWS, d, dtype, seed=d + B + P)
    labels = hip.pack_labels(PR.random_labellings(N_ROWS, M_ROWS, P, np.random.default_rng(P + B)))
    got = hip.kad_permutation_sweep(x, y, labels, bandwidths=_ladder(_pooled_median(x, y), B), kernel=kernel)
    assert got["null"].shape == (B, P) and got["p_values"].shape == (B,)
    _assert_entries_are_the_single_calls(got, x, y, labels, kernel, f"{dtype} D={d} {kernel} B={B} P={P}")
    _assert_aggregate_is_the_reference_on_own_statistics(got)
    if B == 1:
        assert got["p_aggregated"] == got["p_values"][0]


def test_sweep_two_rows_each_and_one_column():
    from fadtk_amd import hip
    x = np.array([[0.5], [-1.25]], np.float16)
    y = np.array([[2.0], [0.25]], np.float16)
    u = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [0, 0, 1, 1], [1, 0, 0, 1], [0, 1, 0, 1]], bool)
    got = hip.kad_permutation_sweep(x, y, hip.pack_labels(u), bandwidths=[0.5, 1.0, 3.0])
    _assert_entries_are_the_single_calls(got, x, y, hip.pack_labels(u), label="n = m = 2, D = 1")
    _assert_aggregate_is_the_reference_on_own_statistics(got)
    t = AR.statistics(x.astype(np.float64), y.astype(np.float64), AR.with_observed(2, 2, u), got["bandwidth"])
    assert np.allclose(np.concatenate([got["mmd2"][:, None], got["null"]], axis=1), t, rtol=0, atol=5e-3)      # f16(k - c0) of 6 pairs


def test_sweep_row_pitch_device_rows_and_device_labels():
    import torch
    from fadtk_amd import hip
    rng = np.random.default_rng(4)
    xw = rng.standard_normal((150, 200)).astype(np.float16)
    yw = (rng.standard_normal((90, 200)) + 0.2).astype(np.float16)
    x, y = torch.from_numpy(xw).cuda()[:, :130], torch.from_numpy(yw).cuda()[:, :130]          # ld = 200 > D = 130
    words = hip.pack_labels(PR.random_labellings(150, 90, 129, rng))
    dev_words = torch.from_numpy(words.view(np.int32)).cuda()
    sig = _ladder(_pooled_median(x.contiguous(), y.contiguous()), 4)
    got = hip.kad_permutation_sweep(x, y, dev_words, bandwidths=sig)
    _assert_entries_are_the_single_calls(got, x, y, dev_words, label="ld > D, device rows, device labels")
    host = hip.kad_permutation_sweep(np.ascontiguousarray(xw[:, :130]), np.ascontiguousarray(yw[:, :130]), words, bandwidths=sig)
    for k in FIELDS + ("null", "p_values"):
        assert np.asarray(got[k]).tobytes() == np.asarray(host[k]).tobytes(), k
    assert got["p_aggregated"] == host["p_aggregated"]


def test_sweep_factors_are_the_pooled_median_times_the_factor_and_runs_repeat():
    from fadtk_amd import hip
    x, y, _, _ = _sets(N_ROWS, M_ROWS, 64, "f16", seed=21)
    labels = hip.pack_labels(PR.random_labellings(N_ROWS, M_ROWS, 199, np.random.default_rng(3)))
    factors = [0.25, 0.5, 1.0, 2.0, 1.0]
    med = _pooled_median(x, y)
    rel = hip.kad_permutation_sweep(x, y, labels, factors=factors)
    assert rel["bandwidth"][2] == med and rel["bandwidth"][4] == med                            # the factor 1: the pooled median, bit for bit
    assert rel["bandwidth"].tolist() == [f * med for f in factors]
    assert med != hip.kad_median_distance(x)                                                    # not the baseline's
    absolute = hip.kad_permutation_sweep(x, y, labels, bandwidths=rel["bandwidth"])
    again = hip.kad_permutation_sweep(x, y, labels, factors=factors)
    for other in (absolute, again):
        for k in FIELDS + ("null", "p_values"):
            assert np.asarray(rel[k]).tobytes() == np.asarray(other[k]).tobytes(), k
        assert rel["p_aggregated"] == other["p_aggregated"]
    # a bandwidth given twice, once in the walk of four and once in the single kernel's walk: the same bits, the aggregate unchanged
    for k in FIELDS:
        assert rel[k][2] == rel[k][4], k
    assert rel["null"][2].tobytes() == rel["null"][4].tobytes()
    four = hip.kad_permutation_sweep(x, y, labels, factors=factors[:4])
    assert four["p_aggregated"] == rel["p_aggregated"] and four["p_values"].tolist() == rel["p_values"][:4].tolist()


REF_CASES = [("f16", 128, 255, 257, 199), ("f32", 17, 127, 129, 31), ("bf16", 512, 96, 161, 300), ("f16", 3, 300, 212, 32)]


@pytest.mark.parametrize("dtype,d,n,m,P", REF_CASES)
def test_sweep_statistics_against_float64_reference(dtype, d, n, m, P):
    from fadtk_amd import hip
    x, y, xr, yr = _sets(n, m, d, dtype, seed=d + n + P)
    rng = np.random.default_rng(P)
    u = PR.random_labellings(n, m, P, rng)
    got = hip.kad_permutation_sweep(x, y, hip.pack_labels(u), factors=[0.5, 1.0, 2.0])
    _assert_aggregate_is_the_reference_on_own_statistics(got)
    t = AR.statistics(xr, yr, AR.with_observed(n, m, u), got["bandwidth"])
    more = None if P >= 50 else PR.random_labellings(n, m, 200, rng)
    for b, s in enumerate(got["bandwidth"]):
        spread = t[b, 1:] if more is None else PR.statistics(xr, yr, more, float(s))
        sd = float(np.std(spread))
        err = max(abs(got["mmd2"][b] - t[b, 0]), float(np.max(np.abs(got["null"][b] - t[b, 1:]))))
        print(f"[kad-perm-sweep-err] {dtype} D={d} n={n} m={m} P={P} factor {[0.5, 1.0, 2.0][b]}: max |dt| / sd = {err / sd:.2e}")
        assert err <= TAU * sd, (b, err, TAU * sd)
    pv, pa = AR.aggregate(t)
    print(f"[kad-agg] {dtype} D={d} n={n} m={m} P={P}: library p_aggregated {got['p_aggregated']} p_values {got['p_values'].tolist()}; "
          f"float64 reference {pa} {pv.tolist()}")


def test_sweep_calibration_over_100_null_draws():
    from fadtk_amd import hip
    hits = 0
    for s in range(100):
        x, y, u = AR.null_draw(s)
        hits += hip.kad_permutation_sweep(x, y, hip.pack_labels(u), factors=AR.CALIBRATION_FACTORS)["p_aggregated"] <= 0.05
    print(f"[kad-agg] calibration: {hits} of 100 aggregates <= 0.05 (cap {AR.CALIBRATION_CAP})")
    assert hits <= AR.CALIBRATION_CAP, hits


def test_sweep_power_on_the_blobs_pair():
    from fadtk_amd import calc_kernel_audio_distance_aggregated_test as agg, hip
    x, y, u = AR.blobs_case()
    got = agg(x, y, labels=hip.pack_labels(u), factors=AR.BLOBS_LADDER)
    at_median = float(got["p_values"][AR.BLOBS_LADDER.index(1.0)])
    print(f"[kad-agg] blobs fp32: p_values = {got['p_values'].tolist()}, p_aggregated = {got['p_aggregated']}")
    assert got["permutations"] == 199 and got["seed"] is None and got["kad"].shape == (len(AR.BLOBS_LADDER),)
    assert at_median > 0.2 and got["p_aggregated"] <= 0.05
    assert at_median == hip.kad_permutation_test(x, y, hip.pack_labels(u), bandwidth=float(got["bandwidths"][5]))["p_value"]
    seeded = agg(x, y, permutations=199, seed=5, factors=AR.BLOBS_LADDER, return_labels=True)     # labellings drawn on the device
    assert seeded["seed"] == 5 and seeded["labels"].shape[0] == 199 and seeded["p_aggregated"] <= 0.05


def _raw(x, y, labels, bw, relative):
    """the C call on torch device rows with host labels and sentinel outputs -> (status, outputs untouched)"""
    from fadtk_amd import _capi
    lib = _capi.load_library()
    bw = np.asarray(bw, dtype=np.float64)
    B, P = len(bw), labels.shape[0]
    res = (_capi.FadKadResult * B)()
    for r in res:
        r.mmd2 = -7.0
    null, pv, pa = np.full((B, P), -7.0), np.full(B, -7.0), C.c_double(-7.0)
    st = lib.fad_kad_permutation_sweep(x.data_ptr(), x.shape[0], x.stride(0), y.data_ptr(), y.shape[0], y.stride(0), x.shape[1],
                                       _capi.FAD_F32, 1, bw.ctypes.data_as(C.POINTER(C.c_double)), B, relative, 0, labels.ctypes.data, P, 0,
                                       res, null.ctypes.data, pv.ctypes.data, C.byref(pa), 0, _capi.current_stream_ptr(0))
    untouched = bool(np.all(null == -7.0) and np.all(pv == -7.0) and pa.value == -7.0 and all(r.mmd2 == -7.0 for r in res))
    return st, untouched, lib.fad_last_error()


def test_sweep_refusals_on_device_rows_leave_the_outputs_untouched():
    import torch
    from fadtk_amd import _capi, hip
    xn, yn, _, _ = _sets(40, 30, 8, "f32", seed=3)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    labels = hip.pack_labels(PR.random_labellings(40, 30, 6, np.random.default_rng(0)))
    st, untouched, msg = _raw(x, y, labels, [1.0, 2.0, 1e-30], 0)                               # c_2 = log2(e) / sigma^2 leaves float32
    assert st == _capi.FAD_ERR_INVALID and untouched and b"bandwidth 2 " in msg, msg
    st, untouched, msg = _raw(x, y, labels, [1e25, 1.0], 1)                                     # ... and underflows to 0
    assert st == _capi.FAD_ERR_INVALID and untouched and b"bandwidth 0 " in msg, msg
    same = torch.ones((40, 8), device="cuda")
    st, untouched, msg = _raw(same, same[:30].clone(), labels, [0.5, 1.0], 1)                   # a median of 0
    assert st == _capi.FAD_ERR_INVALID and untouched and b"median" in msg, msg
    bad = x.clone()
    bad[5, 2] = float("nan")
    st, untouched, msg = _raw(bad, y, labels, [0.5, 1.0], 0)
    assert st == _capi.FAD_ERR_NOT_FINITE and untouched, msg
    wrong = labels.copy()
    wrong[3, 0] ^= 1
    with pytest.raises(RuntimeError, match=r"status -1"):                                       # counted on the device
        hip.kad_permutation_sweep(x, y, torch.from_numpy(wrong.view(np.int32)).cuda(), bandwidths=[1.0, 2.0])
    st, untouched, _ = _raw(x, y, labels, [1.0, 2.0], 0)                                        # the call after the refusals
    assert st == _capi.FAD_OK and not untouched


def test_sweep_config3_size_against_the_single_calls():
    """2 x [100 000 x 512] fp16, B = 4, P = 199.  At this size the sweep's walk of 4 x 7 words is cut into more launches than a single
    call's walk of 7 words, so the float64 order of adding the per-tile sums differs: sigma is bit-equal, every
    statistic is held to tau of the null's spread."""
    import torch
    from fadtk_amd import hip
    from fadtk_amd.kad import random_labellings
    gen = torch.Generator(device="cuda").manual_seed(2026)
    n = 100_000
    x = torch.randn((n, 512), generator=gen, device="cuda").half()
    y = (torch.randn((n, 512), generator=gen, device="cuda") * 1.05 + 0.02).half()
    labels = random_labellings(n, n, 199, seed=1)
    got = hip.kad_permutation_sweep(x, y, labels, factors=[0.25, 0.5, 1.0, 2.0])
    _assert_aggregate_is_the_reference_on_own_statistics(got)
    for b, s in enumerate(got["bandwidth"]):
        one = hip.kad_permutation_test(x, y, labels, bandwidth=float(s))
        assert one["bandwidth"] == got["bandwidth"][b]
        sd = float(np.std(one["null"]))
        err = max(abs(got["mmd2"][b] - one["mmd2"]), float(np.max(np.abs(got["null"][b] - one["null"]))))
        print(f"[kad-perm-sweep-err] config-3 sigma {s:.4g}: max |sweep - single| / sd = {err / sd:.2e}, p {got['p_values'][b]} / {one['p_value']}")
        assert err <= TAU * sd, (b, err, sd)
