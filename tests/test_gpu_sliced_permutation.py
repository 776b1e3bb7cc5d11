"""The sliced Wasserstein permutation test on the GPU (fad_sliced_permutation_test; csrc/kad.hip and csrc/sliced_split.h).

(a) stage: index_z is a permutation per direction; sorted_z is non-decreasing, equal keys in ascending row order.
(b) the observed labelling against the plain call: `observed` and values[0] have the bits of hip.sliced_wasserstein(x, y).
(c) every labelling against the plain call: values[p] has the bits of hip.sliced_wasserstein(Z[u_p], Z[~u_p]).
(d) against the float64 reference of tests/sliced_permutation_reference.py: every values[p][l] within value_bound(w_ref, q, dz, dz),
    dz = projection_bound of the pooled rows (both groups' projections are pooled projections): derived, no measured figure.
(e) null, null_max and both p-values follow from values exactly; each p-value lies between the reference's counts at the threshold
    moved up and down by beta = the two bounds involved.
(f) exact rows (every projection exact in float32): values equal the ordered reference bit for bit, the p-values equal the reference's.
(g) repeated rows within and across the sets and a zero row; chunking forced by FAD_SLICED_WORKSPACE, read back from the plan.
(h) the same bits again, for swapped arguments with complemented labellings, 0 for identical sets, powers of two scale exactly.
(i) the sort's and the split's edges (2047, 2048, 2049, 4100 pooled rows; 100 rows x 20 directions), read from the plan.
(j) refusals leave every output untouched.
(k) the public function and the command line.

Measured on an MI355X over this file's cases (the [sliced-perm-err] lines, profiles/sliced_permutation_gpu_tail.txt): the worst value
error is 0.063 of its bound (2 x 3 float32 rows), under 0.03 elsewhere.  No bound here comes from those figures."""
import ctypes as C
import functools

import numpy as np
import pytest

import sliced_permutation_reference as PR
import sliced_reference as SR

pytestmark = pytest.mark.gpu
TOO_FEW, NOT_FINITE, INVALID = -6, -7, -1
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16", "fp32": "float32"}
SHAPES = ((1, 1, 5, 1), (1, 300, 37, 3), (300, 1, 37, 3), (2, 3, 1, 2), (255, 257, 128, 33), (257, 130, 64, 5), (129, 127, 2047, 2),
          (1300, 900, 64, 5))
PITCHED = ((255, 257), (1, 300), (2, 3), (1300, 900))       # x at a row pitch of D + 3


def _perms(n, m):
    return 31 if (n, m) == (257, 130) else 37              # NL = 32: one full word; NL = 38: two words, the last with six labellings


def _dev(a, dt, ld=None):
    """float32 values -> a torch CUDA tensor of dtype dt; with ld, a view of a wider buffer (row pitch ld > D) whose pitch entries are 7"""
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, TORCH_DT[dt]))
    if ld is None:
        return t
    wide = torch.full((t.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _run(x, y, t, dt, u, ldx=None, host=False, stages=False):
    from fadtk_amd import hip
    if host:
        npdt = {"fp16": np.float16, "fp32": np.float32}[dt]
        xs, ys = x.astype(npdt), y.astype(npdt)
    else:
        xs, ys = _dev(x, dt, ldx), _dev(y, dt)
    return hip.sliced_permutation_test(xs, ys, u, t, per_labelling=True, stages=stages)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _case(n, m, d, L, dt):
    """rows, directions, labellings and the device's answer, computed once and left unchanged"""
    x, y = SR.rows(n, m, d, dt)
    t = SR.directions(L, d)
    u = PR.labellings(n, m, _perms(n, m))
    got = _run(x, y, t, dt, u, ldx=d + 3 if (n, m) in PITCHED else None, stages=True)
    return x, y, t, u, got


@functools.lru_cache(maxsize=None)
def _reference(n, m, d, L, dt):
    x, y, t, u, _ = _case(n, m, d, L, dt)
    return PR.permutation_test(x, y, t, dt, u)


def _check_stage(got, N):
    iz, sz = got["index_z"], got["sorted_z"]
    assert iz.dtype == np.int32 and sz.dtype == np.float32 and iz.shape == sz.shape and iz.shape[1] == N
    assert np.array_equal(np.sort(iz, axis=1), np.broadcast_to(np.arange(N, dtype=np.int32), iz.shape))
    assert np.all(np.isfinite(sz)) and np.all(np.diff(sz, axis=1) >= 0)
    tie = np.diff(sz, axis=1) == 0
    assert np.all(np.diff(iz, axis=1)[tie] > 0)


def _check_statistics(got):
    """(e), first half: everything but values follows from values exactly"""
    stats = [SR.statistics(v) for v in got["values"]]
    T, M = np.array([s[0] for s in stats]), np.array([s[2] for s in stats])
    mean, se, mx, k = stats[0]
    assert got["sw2_squared"] == mean and got["max_sliced"] == mx and got["max_index"] == k
    assert (np.isnan(se) and np.isnan(got["std_error"])) if got["values"].shape[1] == 1 else got["std_error"] == se
    assert _same_bits(got["null"], T[1:]) and _same_bits(got["null_max"], M[1:])
    assert (got["p_value"], got["p_value_max"]) == PR.p_values(T, M) and got["permutations"] == len(T) - 1


# ----------------------------------------------------------------------------------------------------- (a), (b), (c)
@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("n,m,d,L", SHAPES)
def test_every_labelling_has_the_plain_calls_bits(n, m, d, L, dt):
    import torch
    from fadtk_amd import hip
    x, y, t, u, got = _case(n, m, d, L, dt)
    assert got["values"].shape == (len(u) + 1, L) and (got["n"], got["m"], got["projections"]) == (n, m, L)
    _check_stage(got, n + m)
    xs, ys = _dev(x, dt), _dev(y, dt)
    plain = hip.sliced_wasserstein(xs, ys, t, values=True)
    assert _same_bits(got["values"][0], plain["values"])
    for k in ("sw2_squared", "max_sliced", "max_index", "n", "m", "projections"):
        assert got[k] == plain[k], k
    assert got["std_error"] == plain["std_error"] or (L == 1 and np.isnan(got["std_error"]) and np.isnan(plain["std_error"]))
    z = torch.cat([xs, ys])
    for p, row in enumerate(u):
        mask = torch.from_numpy(row).cuda()
        one = hip.sliced_wasserstein(z[mask], z[~mask], t, values=True)                # rows in ascending pooled order
        assert _same_bits(got["values"][p + 1], one["values"]), (p, got["values"][p + 1], one["values"])
    _check_statistics(got)


def test_host_rows_and_device_labels():
    import torch
    x, y, t, u, got = _case(257, 130, 64, 5, "fp16")
    host = _run(x, y, t, "fp16", u, host=True, stages=True)
    for k in ("values", "null", "null_max", "sorted_z", "index_z"):
        assert _same_bits(host[k], got[k]), k
    for labels in (torch.from_numpy(u).cuda(), torch.from_numpy(u.astype(np.uint8)), __import__("fadtk_amd").hip.pack_labels(u)):
        again = _run(x, y, t, "fp16", labels)
        assert _same_bits(again["values"], got["values"]) and again["p_value"] == got["p_value"]


# ----------------------------------------------------------------------------------------------------- (d), (e)
@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("n,m,d,L", SHAPES)
def test_against_reference(n, m, d, L, dt):
    x, y, t, u, got = _case(n, m, d, L, dt)
    want = _reference(n, m, d, L, dt)
    tr = SR.round_to_dtype(t, dt)
    dz = SR.projection_bound(np.concatenate([x, y]), tr, dt)
    bound = SR.value_bound(want["values"], want["q"][None, :], dz[None, :], dz[None, :])
    err = np.abs(got["values"] - want["values"])
    print(f"[sliced-perm-err] {n}x{m}x{d} L={L} {dt} values: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), (got["values"], want["values"], bound)
    _check_statistics(got)
    # the p-values: |T_dev - T_ref| <= mean_l bound (and the mean's own rounding), |M_dev - M_ref| <= max_l bound
    P = len(u)
    for key, ref, b in (("p_value", want["T"], bound.mean(axis=1) + L * 2.0 ** -52 * want["T"]), ("p_value_max", want["M"], bound.max(axis=1))):
        beta = b[1:] + b[0]
        low = (1 + int(np.sum(ref[1:] >= ref[0] + beta))) / (P + 1)
        high = (1 + int(np.sum(ref[1:] >= ref[0] - beta))) / (P + 1)
        assert low <= got[key] <= high, (key, low, got[key], high)


# ----------------------------------------------------------------------------------------------------- (f) exact rows
def _exact_check(got, x, y, t, u, tag):
    want = PR.permutation_test(x, y, t, "fp32", u, ordered=True)
    assert np.array_equal(want["pz"], want["pz"].astype(np.float32).astype(np.float64))                    # the projections are exact
    assert _same_bits(got["values"], want["values"]), (tag, got["values"], want["values"])
    assert (got["p_value"], got["p_value_max"]) == (want["p_value"], want["p_value_max"]), tag
    if "sorted_z" in got:
        assert _same_bits(got["sorted_z"], np.sort(want["pz"], axis=0).T.astype(np.float32)), tag
        _check_stage(got, len(x) + len(y))
    _check_statistics(got)


@pytest.mark.parametrize("n,m,d,L,P,dt", ((257, 130, 64, 5, 37, "fp16"), (257, 130, 64, 5, 37, "bf16"), (2049, 2047, 16, 3, 33, "fp32"),
                                          (20001, 13333, 16, 4, 33, "fp16")))
def test_exact_rows_bit_for_bit(n, m, d, L, P, dt):
    from fadtk_amd import hip
    x, y = SR.exact_rows(n, m, d)
    t = SR.exact_directions(L, d)
    u = PR.labellings(n, m, P)
    got = _run(x, y, t, dt, u, stages=True)
    _exact_check(got, x, y, t, u, f"exact {n}x{m}x{d} L={L} {dt}")
    if n == 20001:
        plan = hip.sliced_permutation_last_plan()
        assert plan["share"] == 17 and plan["sort_chunks"] == 1 and plan["rounds"] == 1     # 17 workgroups per segment, 79 match blocks a pair


# ----------------------------------------------------------------------------------------------------- (g) repeated rows, chunking
def test_repeated_rows_within_and_across_the_sets():
    from fadtk_amd import hip
    import torch
    x, y = SR.exact_rows(300, 257, 16, seed=4)
    x[40:80] = x[7]                        # inside x
    y[100:150] = y[3]                      # inside y
    y[200:230] = x[7]                      # across the sets
    y[10:20] = x[250:260]
    x[17] = 0
    y[5] = 0
    t = SR.exact_directions(4, 16)
    u = PR.labellings(300, 257, 37, seed=2)
    got = _run(x, y, t, "fp16", u, stages=True)
    _exact_check(got, x, y, t, u, "repeated rows")
    z = torch.cat([_dev(x, "fp16"), _dev(y, "fp16")])
    for p in (0, 5, 36):
        mask = torch.from_numpy(u[p]).cuda()
        assert _same_bits(got["values"][p + 1], hip.sliced_wasserstein(z[mask], z[~mask], t, values=True)["values"])


def test_same_bits_in_chunks(monkeypatch):
    from fadtk_amd import hip
    n, m, d, L, P = 255, 257, 128, 33, 70
    x, y = SR.rows(n, m, d, "bf16")
    t = SR.directions(L, d)
    u = PR.labellings(n, m, P, seed=3)
    one = _run(x, y, t, "bf16", u, stages=True)
    plan = hip.sliced_permutation_last_plan()
    assert plan == {"sort_chunks": 1, "directions_per_sort_chunk": 33, "rounds": 1, "directions_per_round": 33, "words_per_round": 3,
                    "share": 1}
    keys = ("values", "null", "null_max", "sorted_z", "index_z")
    # here a direction of a sort chunk takes 10 240 bytes and a labelling word of a round 82 816
    for budget, check in (("250000", lambda q: q["sort_chunks"] >= 3 and q["words_per_round"] == 2 and q["directions_per_round"] == 1),
                          ("2000000", lambda q: q["sort_chunks"] == 1 and q["words_per_round"] == 3 and 1 < q["directions_per_round"] < 33),
                          ("1", lambda q: q["sort_chunks"] == 33 and q["directions_per_sort_chunk"] == 1 and q["directions_per_round"] == 1
                           and q["words_per_round"] == 1 and q["rounds"] == 99)):
        monkeypatch.setenv("FAD_SLICED_WORKSPACE", budget)
        cut = _run(x, y, t, "bf16", u, stages=True)
        plan = hip.sliced_permutation_last_plan()
        assert check(plan), (budget, plan)
        assert plan["sort_chunks"] * plan["directions_per_sort_chunk"] >= L > (plan["sort_chunks"] - 1) * plan["directions_per_sort_chunk"]
        for k in keys:
            assert _same_bits(one[k], cut[k]), (budget, k)
        assert (cut["p_value"], cut["p_value_max"], cut["max_index"]) == (one["p_value"], one["p_value_max"], one["max_index"])


# ----------------------------------------------------------------------------------------------------- (h) invariants
@pytest.mark.parametrize("n,m,d,L,dt", ((255, 257, 128, 33, "fp16"), (257, 130, 64, 5, "fp32"), (130, 130, 37, 4, "bf16")))
def test_same_bits_again_and_swapped(n, m, d, L, dt):
    x, y = SR.rows(n, m, d, dt)
    t = SR.directions(L, d)
    u = PR.labellings(n, m, 37, seed=5)
    one, two = _run(x, y, t, dt, u, stages=True), _run(x, y, t, dt, u, stages=True)
    for k in ("values", "null", "null_max", "sorted_z", "index_z"):
        assert _same_bits(one[k], two[k]), k
    swapped = _run(y, x, t, dt, ~np.concatenate([u[:, n:], u[:, :n]], axis=1))         # Z' = [y; x], every label complemented
    for k in ("values", "null", "null_max"):
        assert _same_bits(one[k], swapped[k]), k
    assert (swapped["p_value"], swapped["p_value_max"], swapped["sw2_squared"]) == (one["p_value"], one["p_value_max"], one["sw2_squared"])


def test_identical_sets_give_zero():
    x, _ = SR.rows(255, 257, 128, "fp16")
    got = _run(x, x.copy(), SR.directions(33, 128), "fp16", PR.labellings(255, 255, 37))
    assert got["sw2_squared"] == 0 and got["max_sliced"] == 0 and np.all(got["values"][0] == 0)
    assert got["p_value"] == 1.0 and got["p_value_max"] == 1.0                         # nothing is below 0


@pytest.mark.parametrize("dt,e", (("fp16", 3), ("bf16", -20), ("fp32", 40)))
def test_scaling_by_a_power_of_two(dt, e):
    x, y = SR.rows(257, 130, 64, dt)
    x, y = SR.round_to_dtype(x * np.float32(0.25), dt), SR.round_to_dtype(y * np.float32(0.25), dt)       # away from float16's limits
    t = SR.directions(5, 64)
    u = PR.labellings(257, 130, 37)
    one = _run(x, y, t, dt, u)
    s = np.float32(2.0 ** e)
    two = _run(x * s, y * s, t, dt, u)
    assert _same_bits(two["values"], one["values"] * 4.0 ** e)
    assert (two["p_value"], two["p_value_max"]) == (one["p_value"], one["p_value_max"])


# ----------------------------------------------------------------------------------------------------- (i) the sort's edges
@pytest.mark.parametrize("n,m,L,share", ((1747, 300, 2, 1), (1748, 300, 2, 1), (1749, 300, 2, 2), (2100, 2000, 3, 3), (60, 40, 20, -8)))
def test_sort_and_split_edges(n, m, L, share):
    from fadtk_amd import hip
    x, y = SR.exact_rows(n, m, 8, seed=1)
    t = SR.exact_directions(L, 8, seed=1)
    u = PR.labellings(n, m, 33, seed=1)
    got = _run(x, y, t, "fp16", u, stages=True)
    plan = hip.sliced_permutation_last_plan()
    assert plan["share"] == share and plan["sort_chunks"] == 1 and plan["directions_per_sort_chunk"] == L and plan["rounds"] == 1
    _exact_check(got, x, y, t, u, f"edge N={n + m} L={L}")


# ----------------------------------------------------------------------------------------------------- (j) refusals
def test_refusals_leave_the_outputs_untouched():
    import torch
    from fadtk_amd import _capi, hip
    lib = _capi.load_library()
    x, y = SR.rows(130, 70, 37, "fp32")
    t = SR.directions(4, 37)
    lab = hip.pack_labels(PR.labellings(130, 70, 5))
    res = _capi.FadSlicedPermutationResult()
    res.observed.sw2_squared, res.observed.max_index, res.p_value, res.p_value_max, res.permutations = -7.0, 99, -7.0, -7.0, 99
    null, null_max, vals = np.full(5, -7.0), np.full(5, -7.0), np.full((6, 4), -7.0)
    sz, iz = np.full((4, 200), -7.0, np.float32), np.full((4, 200), -7, np.int32)
    det = _capi.FadSlicedPermutationDetail(vals.ctypes.data, sz.ctypes.data, iz.ctypes.data)

    def call(xa=x, ya=y, n=130, m=70, d=37, dt=_capi.FAD_F32, th=t, L=4, out=C.byref(res), ld=37, lb=lab.ctypes.data, P=5, dev_l=0):
        return lib.fad_sliced_permutation_test(xa.ctypes.data, n, ld, ya.ctypes.data, m, ld, d, dt, 0, th.ctypes.data if th is not None else None,
                                               L, lb, P, dev_l, out, null.ctypes.data, null_max.ctypes.data, C.byref(det), 0, None)
    assert call(dt=_capi.FAD_F64) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID and call(ld=36) == INVALID
    assert call(L=0) == INVALID and call(L=65537) == INVALID and call(P=0) == INVALID and call(P=65537) == INVALID
    assert call(out=None) == INVALID and call(th=None) == INVALID and call(lb=None) == INVALID
    assert call(n=0) == TOO_FEW and call(m=0) == TOO_FEW
    assert call(n=2 ** 27, m=2 ** 26) == INVALID and call(n=2 ** 30, m=2 ** 30) == INVALID
    tz = t.copy()
    tz[2] = 0
    assert call(th=tz) == INVALID
    wrong = lab.copy()
    wrong[2, 3] ^= np.uint32(1 << 9)                                                   # labelling 2 with one label flipped: n +- 1 ones
    assert call(lb=wrong.ctypes.data) == INVALID
    wrong_d = torch.from_numpy(wrong.view(np.int32)).cuda()
    assert call(lb=wrong_d.data_ptr(), dev_l=1) == INVALID                             # counted on the device
    assert "fad_sliced_permutation_test" in _capi.last_error()
    bad_rows = y.copy()
    bad_rows[69, 36] = np.inf
    assert call(ya=bad_rows) == NOT_FINITE
    bad_rows[69, 36] = np.nan
    assert call(xa=np.concatenate([bad_rows, bad_rows]), n=130) == NOT_FINITE
    big = np.full((130, 37), 1e18, np.float32)                                         # finite norms, projections beyond float32
    tb = t.copy()
    tb[3] = 1e25
    assert call(xa=big, th=tb) == NOT_FINITE
    assert (res.observed.sw2_squared, res.observed.max_index, res.p_value, res.p_value_max, res.permutations) == (-7.0, 99, -7.0, -7.0, 99)
    for a in (null, null_max, vals, sz):
        assert np.all(a == -7.0)
    assert np.all(iz == -7)
    good_d = torch.from_numpy(lab.view(np.int32)).cuda()
    assert call(lb=good_d.data_ptr(), dev_l=1) == 0 and res.observed.sw2_squared > 0 and res.permutations == 5
    assert np.all(vals > 0) and np.all(null > 0) and np.all(null_max >= null) and np.all(sz != -7.0) and np.all(iz >= 0)
    first = vals.copy()
    assert call() == 0 and _same_bits(first, vals)


# ----------------------------------------------------------------------------------------------------- (k) the public function
def test_public_function_has_power_and_takes_labels():
    from fadtk_amd import calc_sliced_wasserstein, calc_sliced_wasserstein_permutation_test, sliced_directions
    rng = np.random.default_rng([2000, 0])
    x, y = rng.standard_normal((60, 8)).astype(np.float32), (rng.standard_normal((45, 8)) + 0.5).astype(np.float32)
    res = calc_sliced_wasserstein_permutation_test(x, y, permutations=199, projections=16, seed=1, return_labels=True, per_labelling=True)
    assert res["p_value"] <= 0.05 and res["permutations"] == 199 and res["seed"] == 1 and res["values"].shape == (200, 16)
    assert res["null"].shape == res["null_max"].shape == (199,) and (res["n"], res["m"], res["projections"]) == (60, 45, 16)
    plain = calc_sliced_wasserstein(x, y, projections=16, seed=1)
    for k in ("sw2_squared", "sliced_w2", "std_error", "max_sliced", "max_index", "fad_scale"):
        assert res[k] == plain[k], k
    again = calc_sliced_wasserstein_permutation_test(x, y, directions=sliced_directions(8, 16, 1), labels=res["labels"])
    assert again["seed"] is None and again["permutations"] == 199
    assert _same_bits(again["null"], res["null"]) and (again["p_value"], again["p_value_max"]) == (res["p_value"], res["p_value_max"])
    rng = np.random.default_rng([2000, 2])
    centre = np.zeros(8)
    centre[0] = 3.0
    base = np.concatenate([rng.standard_normal((100, 8)) + centre, rng.standard_normal((100, 8)) - centre]).astype(np.float16)
    dropped = (rng.standard_normal((150, 8)) + centre).astype(np.float32)              # mixed dtypes go to float32
    res = calc_sliced_wasserstein_permutation_test(base, dropped, permutations=199, projections=16, seed=1)
    assert res["p_value"] <= 0.05


def test_command_line_on_two_cached_directories(tmp_path, capsys):
    from fadtk_amd import SlicedWasserstein, sliced_permutation
    from fadtk_amd.model_loader import get_all_models
    rng = np.random.default_rng(3)
    base, evl = tmp_path / "base", tmp_path / "evl"
    for d, sizes, shift in ((base, (40, 41, 42), 0.0), (evl, (25, 31, 1), 0.5)):
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i, rows in enumerate(sizes):
            (d / f"f{i}.wav").write_bytes(b"")                  # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"f{i}.npy", (rng.standard_normal((rows, 128)) + shift).astype(np.float32))
    csv = tmp_path / "out" / "perm.csv"
    for _ in range(2):
        sliced_permutation.main(["vggish", str(base), str(evl), str(csv), "-p", "99", "--projections", "16", "--seed", "2", "-w", "2"])
    printed = capsys.readouterr().out.split()
    lines = csv.read_text().splitlines()
    assert lines[0] + "\n" == sliced_permutation.CSV_HEADER and len(lines) == 3 and lines[1] == lines[2]
    cells = dict(zip(sliced_permutation.CSV_HEADER.strip().split(","), lines[1].split(",")))
    assert (cells["model"], cells["n"], cells["m"], cells["permutations"], cells["projections"], cells["seed"]) == ("vggish", "123", "57", "99",
                                                                                                                 "16", "2")
    assert printed[-3:] == [cells["sw2_squared"], cells["p_value"], cells["p_value_max"]] and float(cells["p_value"]) == 0.01
    ml = {m.name: m for m in get_all_models()}["vggish"]
    sw = SlicedWasserstein(ml, audio_load_worker=2, projections=16, seed=2)
    res = sw.score_permutation_test(base, evl, permutations=99)
    assert repr(res["sw2_squared"]) == cells["sw2_squared"] and repr(res["p_value"]) == cells["p_value"]
    assert res["sw2_squared"] == sw.score(base, evl)["sw2_squared"]
