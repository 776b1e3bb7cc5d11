"""The sliced Wasserstein bootstrap on the GPU (fad_sliced_bootstrap; csrc/kad.hip and csrc/sliced_expand.h).

(1) the contract by equality: every replicate's values row has the bits of the plain call on np.repeat of the rows by its counts; row 0
    and `observed` those of the plain call on (x, y); boot / boot_max that call's sw2_squared / max_sliced.
(2) explicit counts: totals that differ per replicate (x leads in some replicates, y in others), a total of 1, a 255 on one row with
    zeros elsewhere; 1, 3, 4 and 5 replicates.
(3) chunking forced by FAD_SLICED_WORKSPACE, read back from the plan: the bits of the uncut call.
(4) the same bits again, for swapped arguments with swapped counts, exactly 0 for x against itself with equal counts.
(5) files as units through x_offsets / y_offsets (unequal lengths, an empty file), against the same equality.
(6) compare: two evaluation sets meet the same baseline counts; diff is the difference of the two boot arrays.
(7) sanity: two samples of one Gaussian give bias > 0 and a basic interval below the percentile one.
(8) the float64 reference of tests/sliced_bootstrap_reference.py within the bound tests/test_gpu_sliced.py derives for the plain call,
    per replicate on the repeated rows: a projection of a repeated row is the row's projection, so delta_x and delta_y =
    SR.projection_bound of the sets as given bound every replicate's sorted projections (sorting is 1-Lipschitz in the sup norm), and
    |W - W_ref| <= (2 sqrt(W_ref q) (delta_x + delta_y) + (delta_x + delta_y)^2) / q = SR.value_bound.  No measured figure.
(9) the command line on two small cached directories, files as units; a second evaluation directory adds the pair row; --rows.
(10) a non-finite row refuses with FAD_ERR_NOT_FINITE and leaves the outputs untouched.

Measured on an MI355X over (8)'s cases (the [sliced-boot-err] lines): the worst value error is 0.001 of its bound.  No bound here comes
from that figure."""
import ctypes as C

import numpy as np
import pytest

import sliced_bootstrap_reference as BR
import sliced_reference as SR

pytestmark = pytest.mark.gpu
NOT_FINITE = -7
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16", "fp32": "float32"}
SHAPES = ((1, 1, 37, 2, 3), (1, 300, 37, 3, 5), (65, 64, 128, 8, 9), (257, 256, 37, 4, 4), (2049, 700, 128, 3, 5), (4500, 4100, 37, 2, 3))
PITCHED = ((1, 300), (257, 256), (4500, 4100))              # x at a row pitch of D + 3


def _dev(a, dt, ld=None):
    """float32 values -> a torch CUDA tensor of dtype dt; with ld, a view of a wider buffer (row pitch ld > D) whose pitch entries are 7"""
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, TORCH_DT[dt]))
    if ld is None:
        return t
    wide = torch.full((t.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _run(x, y, t, dt, cx, cy, ldx=None, stages=False):
    from fadtk_amd import hip
    return hip.sliced_bootstrap(_dev(x, dt, ldx), _dev(y, dt), cx, cy, t, per_replicate=True, stages=stages)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_against_plain_calls(got, x, y, t, dt, cx, cy, tag):
    """(1): replicate by replicate against hip.sliced_wasserstein on the repeated rows"""
    import torch
    from fadtk_amd import hip
    xs, ys = _dev(x, dt), _dev(y, dt)
    B, L = len(cx), len(t)
    assert got["values"].shape == (B + 1, L) and got["replicates"] == B and (got["n"], got["m"], got["projections"]) == (len(x), len(y), L)
    plain = hip.sliced_wasserstein(xs, ys, t, values=True)
    assert _same_bits(got["values"][0], plain["values"]), tag
    for k in ("sw2_squared", "max_sliced", "max_index", "n", "m", "projections"):
        assert got[k] == plain[k], (tag, k)
    assert got["std_error"] == plain["std_error"] or (L == 1 and np.isnan(got["std_error"]) and np.isnan(plain["std_error"]))
    assert got["totals"][0].tolist() == [len(x), len(y)]
    for b in range(B):
        rx = torch.repeat_interleave(xs, torch.from_numpy(cx[b].astype(np.int64)).cuda(), dim=0)       # np.repeat along the rows
        ry = torch.repeat_interleave(ys, torch.from_numpy(cy[b].astype(np.int64)).cuda(), dim=0)
        one = hip.sliced_wasserstein(rx, ry, t, values=True)
        assert got["totals"][b + 1].tolist() == [len(rx), len(ry)] == [int(cx[b].sum()), int(cy[b].sum())], (tag, b)
        assert _same_bits(got["values"][b + 1], one["values"]), (tag, b, got["values"][b + 1], one["values"])
        assert got["boot"][b] == one["sw2_squared"] and got["boot_max"][b] == one["max_sliced"], (tag, b)


def _drawn(n, m, B, seed=0):
    from fadtk_amd.sliced import bootstrap_counts
    return bootstrap_counts(np.ones(n, dtype=int), B, seed, 0), bootstrap_counts(np.ones(m, dtype=int), B, seed, 1)


# ----------------------------------------------------------------------------------------------------- (1)
@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("n,m,d,L,B", SHAPES)
def test_every_replicate_has_the_plain_calls_bits(n, m, d, L, B, dt):
    x, y = SR.rows(n, m, d, dt)
    t = SR.directions(L, d)
    cx, cy = _drawn(n, m, B)
    got = _run(x, y, t, dt, cx, cy, ldx=d + 3 if (n, m) in PITCHED else None, stages=True)
    for k, rows in (("x", n), ("y", m)):
        ix, sx = got["index_" + k], got["sorted_" + k]
        assert np.array_equal(np.sort(ix, axis=1), np.broadcast_to(np.arange(rows, dtype=np.int32), ix.shape))
        assert np.all(np.diff(sx, axis=1) >= 0) and np.all(np.diff(ix, axis=1)[np.diff(sx, axis=1) == 0] > 0)
    _check_against_plain_calls(got, x, y, t, dt, cx, cy, f"{n}x{m}x{d} L={L} B={B} {dt}")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_integer_rows_with_ties_and_duplicated_rows(dt):
    rng = np.random.default_rng(21)
    x = rng.integers(-2, 3, (300, 8)).astype(np.float32)                               # 5 values a coordinate: many equal projections
    y = rng.integers(-2, 3, (257, 8)).astype(np.float32)
    x[40:80] = x[7]
    y[100:150] = y[3]
    y[200:230] = x[7]                                                                  # across the sets
    t = SR.exact_directions(4, 8)
    cx, cy = _drawn(300, 257, 5, seed=2)
    got = _run(x, y, t, dt, cx, cy)
    _check_against_plain_calls(got, x, y, t, dt, cx, cy, f"ties {dt}")
    want = BR.bootstrap(x, y, t, dt, cx, cy, ordered=True)                             # every projection exact: the ordered reference's bits
    assert _same_bits(got["values"], want["values"]) and _same_bits(got["boot"], want["boot"])
    assert np.array_equal(got["totals"], want["totals"])


# ----------------------------------------------------------------------------------------------------- (2)
@pytest.mark.parametrize("B", (1, 3, 4, 5))
def test_explicit_counts(B):
    n, m, d, L = 70, 90, 37, 3
    x, y = SR.rows(n, m, d, "fp16")
    t = SR.directions(L, d)
    cx, cy = BR.row_counts(n, B, seed=B), BR.row_counts(m, B, seed=10 + B)
    cx[0], cy[0] = 0, 0
    cx[0, 33], cy[0, 5] = 255, 1                                                       # 255 on one row and zeros elsewhere; a total of 1
    if B >= 3:
        cx[1], cy[1] = 3, 0
        cy[1, :40] = 2                                                                 # 210 rows of x against 80 of y: x leads
        cx[2], cy[2] = 0, 4
        cx[2, 10:35] = 1                                                               # 25 against 360: y leads
    if B >= 4:
        cx[3], cy[3] = 0, 0
        cx[3, :60], cy[3, 30:] = 3, 3                                                  # 180 against 180: a tie, x leads
    got = _run(x, y, t, "fp16", cx, cy)
    _check_against_plain_calls(got, x, y, t, "fp16", cx, cy, f"explicit B={B}")
    assert got["totals"][1].tolist() == [255, 1]
    if B >= 4:
        assert got["totals"][2:5].tolist() == [[210, 80], [25, 360], [180, 180]]


# ----------------------------------------------------------------------------------------------------- (3)
def test_same_bits_in_chunks(monkeypatch):
    from fadtk_amd import hip
    n, m, d, L, B = 257, 256, 64, 7, 9
    x, y = SR.rows(n, m, d, "bf16")
    t = SR.directions(L, d)
    cx, cy = _drawn(n, m, B, seed=3)
    one = _run(x, y, t, "bf16", cx, cy, stages=True)
    plan = hip.sliced_bootstrap_last_plan()
    assert plan == {"sort_chunks": 1, "directions_per_sort_chunk": 7, "rounds": 1, "directions_per_round": 7, "words_per_round": 3,
                    "replicates_per_word": 4}
    keys = ("values", "totals", "boot", "boot_max", "sorted_x", "index_x", "sorted_y", "index_y")
    # here a direction of a sort chunk takes 10 240 bytes and a replicate word of a round 10 352
    for budget, check in (("60000", lambda q: q["sort_chunks"] == 7 and q["words_per_round"] == 3 and q["rounds"] == 7),
                          ("30000", lambda q: q["sort_chunks"] == 7 and q["words_per_round"] == 2 and q["rounds"] == 14),
                          ("160000", lambda q: q["sort_chunks"] == 3 and q["directions_per_sort_chunk"] == 3 and q["words_per_round"] == 3
                           and q["directions_per_round"] == 3 and q["rounds"] == 3),
                          ("1", lambda q: q["sort_chunks"] == 7 and q["directions_per_sort_chunk"] == 1 and q["directions_per_round"] == 1
                           and q["words_per_round"] == 1 and q["rounds"] == 21)):
        monkeypatch.setenv("FAD_SLICED_WORKSPACE", budget)
        cut = _run(x, y, t, "bf16", cx, cy, stages=True)
        plan = hip.sliced_bootstrap_last_plan()
        assert check(plan) and plan["rounds"] > 1, (budget, plan)
        assert plan["sort_chunks"] * plan["directions_per_sort_chunk"] >= L > (plan["sort_chunks"] - 1) * plan["directions_per_sort_chunk"]
        for k in keys:
            assert _same_bits(one[k], cut[k]), (budget, k)
        assert (cut["sw2_squared"], cut["max_index"]) == (one["sw2_squared"], one["max_index"])


# ----------------------------------------------------------------------------------------------------- (4)
@pytest.mark.parametrize("n,m,d,L,dt", ((255, 257, 128, 8, "fp16"), (257, 130, 64, 5, "fp32"), (130, 130, 37, 4, "bf16")))
def test_same_bits_again_and_swapped(n, m, d, L, dt):
    x, y = SR.rows(n, m, d, dt)
    t = SR.directions(L, d)
    cx, cy = _drawn(n, m, 6, seed=5)
    one, two = _run(x, y, t, dt, cx, cy, stages=True), _run(x, y, t, dt, cx, cy, stages=True)
    for k in ("values", "boot", "boot_max", "totals", "sorted_x", "index_x", "sorted_y", "index_y"):
        assert _same_bits(one[k], two[k]), k
    swapped = _run(y, x, t, dt, cy, cx)
    for k in ("values", "boot", "boot_max"):
        assert _same_bits(one[k], swapped[k]), k
    assert np.array_equal(swapped["totals"], one["totals"][:, ::-1]) and swapped["sw2_squared"] == one["sw2_squared"]


def test_a_set_against_itself_gives_exactly_zero():
    from fadtk_amd import hip
    x, _ = SR.rows(255, 257, 128, "fp16")
    cx, _ = _drawn(255, 1, 7)
    xs = _dev(x, "fp16")
    got = hip.sliced_bootstrap(xs, xs, cx, cx, SR.directions(8, 128), per_replicate=True)
    assert got["sw2_squared"] == 0 and got["max_sliced"] == 0 and np.all(got["values"] == 0) and np.all(got["boot"] == 0)


# ----------------------------------------------------------------------------------------------------- (5)
def test_files_as_units():
    from fadtk_amd import calc_sliced_wasserstein_bootstrap, sliced_directions
    from fadtk_amd.sliced import bootstrap_counts
    xo, yo = np.array([0, 40, 40, 47, 130, 131, 200]), np.array([0, 3, 90, 90, 150])   # unequal lengths, an empty file on both sides
    x, y = SR.rows(200, 150, 37, "fp32")
    res = calc_sliced_wasserstein_bootstrap(x, y, replicates=8, projections=6, seed=3, x_offsets=xo, y_offsets=yo, per_replicate=True)
    assert (res["unit"], res["unit_x"], res["unit_y"], res["seed"], res["replicates"]) == ("file", "file", "file", 3, 8)
    cx, cy = res["counts_x"], res["counts_y"]
    assert np.array_equal(cx, bootstrap_counts(np.diff(xo), 8, 3, 0)) and np.array_equal(cy, bootstrap_counts(np.diff(yo), 8, 3, 1))
    assert len({int(v) for v in cx.sum(axis=1)}) > 1                                   # the totals differ from replicate to replicate
    raw = {k: res[k] for k in ("values", "totals", "boot", "boot_max", "sw2_squared", "max_sliced", "max_index", "std_error", "n", "m",
                               "projections", "replicates")}
    _check_against_plain_calls(raw, x, y, sliced_directions(37, 6, 3), "fp32", cx, cy, "files")
    half = calc_sliced_wasserstein_bootstrap(x, y, replicates=8, projections=6, seed=3, x_offsets=xo)
    assert (half["unit"], half["unit_x"], half["unit_y"]) == ("file", "file", "row")
    given = calc_sliced_wasserstein_bootstrap(x, y, projections=6, seed=3, counts_x=cx, counts_y=cy)
    assert given["seed"] is None and given["unit"] == "row" and _same_bits(given["boot"], res["boot"])


# ----------------------------------------------------------------------------------------------------- (6)
def test_compare_two_sets_on_one_baseline():
    from fadtk_amd import calc_sliced_wasserstein_bootstrap, calc_sliced_wasserstein_bootstrap_compare
    rng = np.random.default_rng(31)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    ya, yb = (rng.standard_normal((280, 16)) + 0.1).astype(np.float32), (rng.standard_normal((310, 16)) + 0.6).astype(np.float32)
    res = calc_sliced_wasserstein_bootstrap_compare(x, [ya, yb], replicates=9, projections=8, seed=2, per_replicate=True)
    a, b = res["sets"]
    assert np.array_equal(a["counts_x"], b["counts_x"]) and not np.array_equal(a["counts_y"][:, :280], b["counts_y"][:, :280])
    pair = res["pairs"][(0, 1)]
    assert _same_bits(pair["diff"], a["boot"] - b["boot"]) and pair["diff_observed"] == a["sw2_squared"] - b["sw2_squared"]
    assert pair["prob_closer"] == 1.0 and pair["ci_diff"][1] < 0                       # a shift of 0.1 against one of 0.6
    alone = calc_sliced_wasserstein_bootstrap(x, ya, replicates=9, projections=8, seed=2)
    assert _same_bits(alone["boot"], a["boot"]) and alone["sw2_squared"] == a["sw2_squared"]      # set 0 is the single call's stream 1


# ----------------------------------------------------------------------------------------------------- (7)
def test_plug_in_bias_on_two_samples_of_one_gaussian():
    from fadtk_amd import calc_sliced_wasserstein_bootstrap
    rng = np.random.default_rng(41)
    x, y = rng.standard_normal((400, 16)).astype(np.float32), rng.standard_normal((350, 16)).astype(np.float32)
    res = calc_sliced_wasserstein_bootstrap(x, y, replicates=9, projections=8, seed=1)
    assert res["sw2_squared"] > 0 and res["bias"] > 0 and res["bias"] == res["boot_mean"] - res["sw2_squared"]
    assert res["ci_basic"][0] < res["ci_percentile"][0] and res["ci_basic"][1] < res["ci_percentile"][1]
    assert res["ci_basic"] == (2 * res["sw2_squared"] - res["ci_percentile"][1], 2 * res["sw2_squared"] - res["ci_percentile"][0])
    assert res["boot_std"] == np.std(res["boot"], ddof=1) and res["confidence"] == 0.95 and res["unit"] == "row"


# ----------------------------------------------------------------------------------------------------- (8)
@pytest.mark.parametrize("n,m,d,L,dt", ((257, 130, 64, 5, "fp16"), (300, 301, 37, 4, "fp32")))
def test_against_reference(n, m, d, L, dt):
    x, y = SR.rows(n, m, d, dt)
    t = SR.directions(L, d)
    cx, cy = _drawn(n, m, 6, seed=7)
    got = _run(x, y, t, dt, cx, cy)
    want = BR.bootstrap(x, y, t, dt, cx, cy)
    tr = SR.round_to_dtype(t, dt)
    dx, dy = SR.projection_bound(x, tr, dt), SR.projection_bound(y, tr, dt)
    bound = SR.value_bound(want["values"], want["q"][None, :], dx[None, :], dy[None, :])
    err = np.abs(got["values"] - want["values"])
    print(f"[sliced-boot-err] {n}x{m}x{d} L={L} {dt} values: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), (got["values"], want["values"], bound)
    assert np.array_equal(got["totals"], want["totals"])
    for b in range(7):                                                                 # everything but values follows from values exactly
        mean, _, mx, k = SR.statistics(got["values"][b])
        assert (got["sw2_squared"], got["max_sliced"], got["max_index"]) == (mean, mx, k) if b == 0 else \
            (got["boot"][b - 1], got["boot_max"][b - 1]) == (mean, mx)
    stats = BR.intervals(got["boot"], got["sw2_squared"])
    from fadtk_amd.sliced import bootstrap_statistics
    mine = bootstrap_statistics(got["boot"], got["sw2_squared"])
    assert mine["bias"] == stats["bias"] and mine["ci_percentile"] == tuple(stats["ci_percentile"]) and mine["ci_basic"] == tuple(stats["ci_basic"])


# ----------------------------------------------------------------------------------------------------- (9)
def test_command_line_on_cached_directories(tmp_path, capsys):
    from fadtk_amd import SlicedWasserstein, sliced_bootstrap
    from fadtk_amd.model_loader import get_all_models
    rng = np.random.default_rng(3)
    base, eva, evb = tmp_path / "base", tmp_path / "eva", tmp_path / "evb"
    for d, sizes, shift in ((base, (40, 41, 42, 9), 0.0), (eva, (25, 31, 1, 12), 0.2), (evb, (30, 28, 17), 0.7)):
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i, rows in enumerate(sizes):
            (d / f"f{i}.wav").write_bytes(b"")                  # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"f{i}.npy", (rng.standard_normal((rows, 128)) + shift).astype(np.float32))
    csv = tmp_path / "out" / "boot.csv"
    common = ["-b", "9", "--projections", "8", "--seed", "2", "-w", "2", "--confidence", "0.8"]
    sliced_bootstrap.main(["vggish", str(base), str(eva), "--csv", str(csv), *common])
    printed = capsys.readouterr().out.split()
    header = sliced_bootstrap.CSV_HEADER.strip().split(",")
    lines = csv.read_text().splitlines()
    assert lines[0] + "\n" == sliced_bootstrap.CSV_HEADER and len(lines) == 2
    one = dict(zip(header, lines[1].split(",")))
    assert (one["kind"], one["model"], one["unit"], one["n"], one["m"], one["replicates"], one["confidence"], one["projections"], one["seed"]) == \
        ("set", "vggish", "file", "132", "69", "9", "0.8", "8", "2")
    assert printed[-3:] == [one["sw2_squared"], one["ci_basic_lo"], one["ci_basic_hi"]]
    sliced_bootstrap.main(["vggish", str(base), str(eva), str(evb), "--csv", str(csv), *common])
    lines = csv.read_text().splitlines()
    assert len(lines) == 5 and lines[2] == lines[1]                                    # set A again, set B, the pair
    two, pair = dict(zip(header, lines[3].split(","))), dict(zip(header, lines[4].split(",")))
    assert (two["kind"], two["eval"], two["m"]) == ("set", str(evb), "75")
    assert (pair["kind"], pair["eval"], pair["other"], pair["unit"]) == ("pair", str(eva), str(evb), "file")
    assert float(pair["sw2_squared"]) == float(one["sw2_squared"]) - float(two["sw2_squared"]) and 0.0 <= float(pair["prob_closer"]) <= 1.0
    sliced_bootstrap.main(["vggish", str(base), str(eva), "--csv", str(csv), "--rows", *common])
    rows = dict(zip(header, csv.read_text().splitlines()[5].split(",")))
    assert rows["unit"] == "row" and rows["sw2_squared"] == one["sw2_squared"] and rows["boot_mean"] != one["boot_mean"]
    ml = {m.name: m for m in get_all_models()}["vggish"]
    sw = SlicedWasserstein(ml, audio_load_worker=2, projections=8, seed=2)
    res = sw.score_bootstrap(base, [eva], replicates=9, confidence=0.8)
    assert repr(res["sets"][0]["sw2_squared"]) == one["sw2_squared"] and repr(res["sets"][0]["boot_mean"]) == one["boot_mean"]
    assert res["sets"][0]["sw2_squared"] == sw.score(base, eva)["sw2_squared"] and len(res["x_files"]) == 4


# ----------------------------------------------------------------------------------------------------- (10)
def test_a_non_finite_row_refuses_and_leaves_the_outputs_untouched():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, y = SR.rows(130, 70, 37, "fp32")
    t = SR.directions(4, 37)
    cx, cy = _drawn(130, 70, 5)
    res = _capi.FadSlicedBootstrapResult()
    res.observed.sw2_squared, res.observed.max_index, res.replicates = -7.0, 99, 99
    boot, boot_max, vals, tot = np.full(5, -7.0), np.full(5, -7.0), np.full((6, 4), -7.0), np.full((6, 2), -7, np.int64)
    sx, ix = np.full((4, 130), -7.0, np.float32), np.full((4, 130), -7, np.int32)
    sy, iy = np.full((4, 70), -7.0, np.float32), np.full((4, 70), -7, np.int32)
    det = _capi.FadSlicedBootstrapDetail(vals.ctypes.data, sx.ctypes.data, ix.ctypes.data, sy.ctypes.data, iy.ctypes.data, tot.ctypes.data)

    def call(xa=x, ya=y, th=t):
        return lib.fad_sliced_bootstrap(xa.ctypes.data, 130, 37, ya.ctypes.data, 70, 37, 37, _capi.FAD_F32, 0, th.ctypes.data, 4, cx.ctypes.data,
                                        cy.ctypes.data, 5, C.byref(res), boot.ctypes.data, boot_max.ctypes.data, C.byref(det), 0, None)
    bad = y.copy()
    bad[69, 36] = np.inf
    assert call(ya=bad) == NOT_FINITE
    bad = x.copy()
    bad[0, 0] = np.nan
    assert call(xa=bad) == NOT_FINITE
    big = np.full((130, 37), 1e18, np.float32)                                         # finite norms, projections beyond float32
    tb = t.copy()
    tb[3] = 1e25
    assert call(xa=big, th=tb) == NOT_FINITE and "fad_sliced_bootstrap" in _capi.last_error()
    assert (res.observed.sw2_squared, res.observed.max_index, res.replicates) == (-7.0, 99, 99)
    for a in (boot, boot_max, vals, sx, sy):
        assert np.all(a == -7.0)
    assert np.all(ix == -7) and np.all(iy == -7) and np.all(tot == -7)
    assert call() == 0 and res.observed.sw2_squared > 0 and res.replicates == 5
    assert np.all(vals > 0) and np.all(boot > 0) and np.all(boot_max >= boot) and np.all(sx != -7.0) and np.all(iy >= 0)
    assert tot[0].tolist() == [130, 70] and np.array_equal(tot[1:, 0], cx.sum(axis=1)) and np.array_equal(tot[1:, 1], cy.sum(axis=1))
