"""The per-song sliced Wasserstein distance on the GPU (fad_sliced_individual; csrc/kad.hip and csrc/sliced_song_sort.h).

The contract is equality: song s gets, bit for bit, what fad_sliced_wasserstein(x, song_s) returns with the same directions -- values,
the three statistics, max_index, and the sorted projections behind them.  The whole-set entry holds to its float64 reference in
tests/test_gpu_sliced.py, so equality carries those bounds over and no new tolerance appears here; the reference is checked per song all
the same (bound (c) of that file, computed here per song from the inputs; exact rows to the last bit).  Then the invariances the header
promises -- the same bits again, for any chunking of the directions, wherever a song sits and whatever its neighbours are -- and the
per-song statuses.  The resident capacity C and the unit table's edges are read from fad_sliced_individual_last_plan, so a test asserts
that it hit the edges it claims.  numpy has no bfloat16, so host rows run in float16 and float32 only."""
import ctypes as C
import functools

import numpy as np
import pytest

import sliced_reference as SR

pytestmark = pytest.mark.gpu
TOO_FEW, NOT_FINITE = -6, -7
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16", "fp32": "float32"}
# (n; song lengths; D; L)
SHAPES = {
    "roles-swap": (130, (1, 2, 3, 255, 256, 257, 300), 37, 3),
    "600-songs": (300, (1,) * 600, 5, 2),
    "empty-song": (257, (130, 130, 0, 257), 64, 5),
    "one-row": (1, (1, 7), 1, 1),
    "deep": (129, (127, 40), 2047, 2),
}
MODES = [(dt, mode) for dt in SR.DTYPES for mode in ("device", "pitch", "host") if not (dt == "bf16" and mode == "host")]
PITCH_ON_ROWS = ("600-songs", "deep")          # mode "pitch": a row pitch of D + 3 on the song rows there, on the baseline elsewhere


def _dev(a, dt, ld=None):
    """float32 values -> a torch CUDA tensor of dtype dt; with ld, a view of a wider buffer (row pitch ld > D) whose pitch entries are 7"""
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, TORCH_DT[dt]))
    if ld is None:
        return t
    wide = torch.full((t.shape[0], ld), 7.0, dtype=t.dtype, device="cuda")
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _name(p):
    return str(p).replace("\\", "/").rsplit("/", 1)[-1]


def _indiv(x, rows, lens, t, dt, mode="device", sorted=True):
    """mode: "device" tensors, "host" numpy rows, "pitch-x" / "pitch-rows": device tensors, that operand at a row pitch of D + 3"""
    from fadtk_amd import hip
    d = x.shape[1]
    if mode == "host":
        npdt = {"fp16": np.float16, "fp32": np.float32}[dt]
        xs, rs = x.astype(npdt), rows.astype(npdt)
    else:
        xs, rs = _dev(x, dt, d + 3 if mode == "pitch-x" else None), _dev(rows, dt, d + 3 if mode == "pitch-rows" else None)
    return hip.sliced_individual(xs, rs, _offsets(lens), t, values=True, sorted=sorted)


def _whole(x, y, t, dt):
    from fadtk_amd import hip
    return hip.sliced_wasserstein(_dev(x, dt), _dev(y, dt), t, values=True, sorted_projections=True)


@functools.lru_cache(maxsize=None)
def _case(name, dt):
    n, lens, d, L = SHAPES[name]
    x, rows = SR.rows(n, int(sum(lens)), d, dt)
    return x, rows, SR.directions(L, d)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _whole_songs(name, dt):
    """fad_sliced_wasserstein(x, song_s) for every song with rows of a case, computed once for all modes"""
    x, rows, t = _case(name, dt)
    lens = SHAPES[name][1]
    off = _offsets(lens)
    return tuple(_whole(x, rows[off[s]:off[s + 1]], t, dt) if m else None for s, m in enumerate(lens))


def _equal_to_whole_set(got, x, lens, t, ones, tag):
    """every song of `got` against ones[s] = fad_sliced_wasserstein(x, song_s): the same bits everywhere"""
    off = _offsets(lens)
    L = len(t)
    assert got["n"] == len(x) and got["projections"] == L and got["values"].shape == (len(lens), L)
    first = True
    for s, m in enumerate(lens):
        if m == 0:
            assert got["status"][s] == TOO_FEW and got["max_index"][s] == -1 and np.all(np.isnan(got["values"][s])), (tag, s)
            assert np.isnan(got["sw2_squared"][s]) and np.isnan(got["std_error"][s]) and np.isnan(got["max_sliced"][s]), (tag, s)
            continue
        one = ones[s]
        assert got["status"][s] == 0, (tag, s)
        assert _same_bits(got["values"][s], one["values"]), (tag, s, got["values"][s], one["values"])
        for k in ("sw2_squared", "max_sliced"):
            assert got[k][s] == one[k] and np.float64(got[k][s]).tobytes() == np.float64(one[k]).tobytes(), (tag, s, k)
        if L == 1:
            assert np.isnan(got["std_error"][s]) and np.isnan(one["std_error"]), (tag, s)
        else:
            assert np.float64(got["std_error"][s]).tobytes() == np.float64(one["std_error"]).tobytes(), (tag, s)
        assert got["max_index"][s] == one["max_index"], (tag, s)
        if "sorted_rows" in got:
            assert _same_bits(got["sorted_rows"][:, off[s]:off[s + 1]], one["sorted_y"]), (tag, s)
            if first:
                assert _same_bits(got["sorted_x"], one["sorted_x"]), tag
                first = False


# ----------------------------------------------------------------------------------------------------- 1. equality with the whole-set entry
@pytest.mark.parametrize("dt,mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_whole_set_entry(name, dt, mode):
    from fadtk_amd import hip
    x, rows, t = _case(name, dt)
    lens = SHAPES[name][1]
    if mode == "pitch":
        mode = "pitch-rows" if name in PITCH_ON_ROWS else "pitch-x"
    got = _indiv(x, rows, lens, t, dt, mode)
    plan = hip.sliced_individual_last_plan()
    cap = plan["capacity"]
    assert plan["chunks"] == 1 and plan["directions_per_chunk"] == len(t) and plan["long_songs"] == 0 and cap >= 2250
    if name == "600-songs":
        assert plan["units"] == 3 and plan["most_songs"] == 256            # more songs than one unit may hold
    else:
        assert plan["units"] == 1 and plan["most_songs"] == sum(m > 0 for m in lens)
    _equal_to_whole_set(got, x, lens, t, _whole_songs(name, dt), f"{name} {dt} {mode}")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_one_song_holding_all_rows(dt):
    x, rows, t = _case("empty-song", dt)
    got = _indiv(x, rows, (len(rows),), t, dt)
    one = _whole(x, rows, t, dt)
    assert _same_bits(got["values"][0], one["values"]) and _same_bits(got["sorted_rows"], one["sorted_y"])
    assert got["sw2_squared"][0] == one["sw2_squared"] and got["std_error"][0] == one["std_error"]
    assert got["max_sliced"][0] == one["max_sliced"] and got["max_index"][0] == one["max_index"]


# ----------------------------------------------------------------------------------------------------- 2. the float64 reference, per song
@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_float64_reference(name, dt):
    """bound (c) of DESIGN 4.17 per song: |W_l - reference| <= (2 sqrt(W_ref q_l) delta' + delta'^2) / q_l, delta' = delta_x + delta_s,
    each delta the projection bound of its own rows"""
    x, rows, t = _case(name, dt)
    lens = SHAPES[name][1]
    off = _offsets(lens)
    got = _indiv(x, rows, lens, t, dt, sorted=False)
    tr = SR.round_to_dtype(t, dt)
    dx = SR.projection_bound(x, tr, dt)
    worst = 0.0
    for s, m in enumerate(lens):
        if m == 0:
            continue
        y = rows[off[s]:off[s + 1]]
        want = SR.sliced(x, y, t, dt)
        bound = SR.value_bound(want["values"], want["q"], dx, SR.projection_bound(y, tr, dt))
        err = np.abs(got["values"][s] - want["values"])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (name, dt, s, got["values"][s], want["values"], bound)
        mean, se, mx, k = SR.statistics(got["values"][s])
        assert got["sw2_squared"][s] == mean and got["max_sliced"][s] == mx and got["max_index"][s] == k
        assert np.isnan(got["std_error"][s]) if len(t) == 1 else got["std_error"][s] == se
    print(f"[sliced-indiv-err] {name} {dt}: worst error / bound {worst:.3f}")


def _exact_songs(got, x, rows, lens, t, tag):
    """exact rows x exact directions: every song's values equal the reference summed in the documented order to the last bit, and the
    plain-order reference wherever S stays below 2^52 units of 2^-16 (every term and partial sum is then an exact integer)"""
    off = _offsets(lens)
    for s, m in enumerate(lens):
        y = rows[off[s]:off[s + 1]]
        want = SR.sliced(x, y, t, "fp32", ordered=True)
        assert _same_bits(got["sorted_rows"][:, off[s]:off[s + 1]], want["sorted_y"].astype(np.float32)), (tag, s)
        assert _same_bits(got["values"][s], want["values"]), (tag, s, got["values"][s], want["values"])
        plain = SR.sliced(x, y, t, "fp32")["values"]
        small = plain * want["q"] * float(len(x) * m) * 2.0 ** 16 < 2.0 ** 52
        assert np.array_equal(got["values"][s][small], plain[small]), (tag, s)
    assert _same_bits(got["sorted_x"], want["sorted_x"].astype(np.float32)), tag


@pytest.mark.parametrize("dt", SR.DTYPES)
@pytest.mark.parametrize("name", ("roles-swap", "600-songs", "one-row", "deep"))
def test_exact_rows_bit_for_bit(name, dt):
    n, lens, d, L = SHAPES[name]
    x, rows = SR.exact_rows(n, int(sum(lens)), d)
    t = SR.exact_directions(L, d)
    _exact_songs(_indiv(x, rows, lens, t, dt), x, rows, lens, t, f"exact {name} {dt}")


def test_capacity_edges_and_the_long_path():
    """(4000; C - 1, C, C + 1, 2 C + 5; 16; 4): two songs on each side of the resident capacity; the songs of the resident path have the
    bits they have without the long ones"""
    from fadtk_amd import hip
    _indiv(*SR.exact_rows(3, 2, 4), (2,), SR.exact_directions(1, 4), "fp32")
    cap = hip.sliced_individual_last_plan()["capacity"]
    lens = (cap - 1, cap, cap + 1, 2 * cap + 5)
    x, rows = SR.exact_rows(4000, int(sum(lens)), 16)
    t = SR.exact_directions(4, 16)
    got = _indiv(x, rows, lens, t, "fp16")
    plan = hip.sliced_individual_last_plan()
    assert plan["long_songs"] == 2 and plan["units"] == 2 and plan["most_songs"] == 1 and plan["chunks"] == 1
    assert np.all(got["status"] == 0)
    _exact_songs(got, x, rows, lens, t, "capacity edges")
    alone = _indiv(x, rows[:2 * cap - 1], lens[:2], t, "fp16")
    assert hip.sliced_individual_last_plan()["long_songs"] == 0
    for k in ("values", "sw2_squared", "std_error", "max_sliced", "max_index"):
        assert _same_bits(alone[k], got[k][:2]), k
    assert _same_bits(alone["sorted_rows"], got["sorted_rows"][:, :2 * cap - 1])


# ----------------------------------------------------------------------------------------------------- 3. invariances, bit for bit
KEYS = ("values", "sw2_squared", "std_error", "max_sliced", "max_index", "status")


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_same_bits_again_and_in_chunks(dt, monkeypatch):
    from fadtk_amd import hip
    n, lens, d, L = 130, (1, 2, 3, 255, 256, 257, 300), 37, 33
    x, rows = SR.rows(n, int(sum(lens)), d, dt)
    t = SR.directions(L, d)
    one = _indiv(x, rows, lens, t, dt)
    assert hip.sliced_individual_last_plan()["chunks"] == 1
    two = _indiv(x, rows, lens, t, dt)
    for k in KEYS + ("sorted_x", "sorted_rows"):
        assert _same_bits(one[k], two[k]), k
    # per direction (include/fad_hip.h): 4 (256 + 1152 + 256) + 4 (256 + 256) + 8 * 7 = 8760 bytes
    monkeypatch.setenv("FAD_SLICED_WORKSPACE", str(11 * 8760))
    cut = _indiv(x, rows, lens, t, dt)
    plan = hip.sliced_individual_last_plan()
    assert plan["chunks"] == 3 and plan["directions_per_chunk"] == 11
    for k in KEYS + ("sorted_x", "sorted_rows"):
        assert _same_bits(one[k], cut[k]), k
    monkeypatch.setenv("FAD_SLICED_WORKSPACE", "1")                                    # never less than one direction per chunk
    cut = _indiv(x, rows, lens, t, dt)
    plan = hip.sliced_individual_last_plan()
    assert plan["chunks"] == L and plan["directions_per_chunk"] == 1
    for k in KEYS + ("sorted_x", "sorted_rows"):
        assert _same_bits(one[k], cut[k]), k


def test_permuting_the_songs_permutes_the_outputs():
    x, rows, t = _case("roles-swap", "fp32")
    lens = SHAPES["roles-swap"][1]
    off = _offsets(lens)
    one = _indiv(x, rows, lens, t, "fp32")
    perm = [4, 0, 6, 2, 5, 1, 3]
    rows_p = np.concatenate([rows[off[s]:off[s + 1]] for s in perm])
    two = _indiv(x, rows_p, [lens[s] for s in perm], t, "fp32")
    for k in KEYS:
        assert _same_bits(two[k], one[k][perm]), k


@pytest.mark.parametrize("dt", SR.DTYPES)
def test_a_song_equal_to_the_baseline_gives_zero(dt):
    x, rows, t = _case("empty-song", dt)
    lens = (130, 257, 127)
    got = _indiv(x, np.concatenate([rows[:130], x, rows[130:257]]), lens, t, dt)
    assert np.all(got["values"][1] == 0) and got["sw2_squared"][1] == 0 and got["std_error"][1] == 0 and got["max_index"][1] == 0
    assert np.all(got["values"][[0, 2]] > 0)


@pytest.mark.parametrize("dt,e", (("fp16", 3), ("bf16", -20), ("fp32", 40)))
def test_scaling_by_a_power_of_two(dt, e):
    x, rows, t = _case("roles-swap", dt)
    lens = SHAPES["roles-swap"][1]
    x, rows = SR.round_to_dtype(x * np.float32(0.25), dt), SR.round_to_dtype(rows * np.float32(0.25), dt)   # away from float16's limits
    one = _indiv(x, rows, lens, t, dt)
    s = np.float32(2.0 ** e)
    two = _indiv(x * s, rows * s, lens, t, dt)
    assert _same_bits(two["values"], one["values"] * 4.0 ** e) and _same_bits(two["sorted_rows"], one["sorted_rows"] * s)
    assert _same_bits(two["max_index"], one["max_index"])


# ----------------------------------------------------------------------------------------------------- 4. statuses
@pytest.mark.parametrize("dt", SR.DTYPES)
def test_bad_songs_among_good_ones(dt):
    x, rows, t = _case("roles-swap", dt)
    lens = SHAPES["roles-swap"][1]
    off = _offsets(lens)
    good = _indiv(x, rows, lens, t, dt)
    nan_song = rows[off[3]:off[4]].copy()
    nan_song[17, 5] = np.nan
    parts, lens_b = [], []
    for s in range(7):
        parts.append(rows[off[s]:off[s + 1]])
        lens_b.append(lens[s])
        if s == 1:
            parts.append(rows[:0]); lens_b.append(0)                                   # an empty song
        if s == 4:
            parts.append(nan_song); lens_b.append(len(nan_song))                       # a song with one NaN row
    got = _indiv(x, np.concatenate(parts), lens_b, t, dt)
    keep = [0, 1, 3, 4, 5, 7, 8]
    assert got["status"][2] == TOO_FEW and got["status"][6] == NOT_FINITE and np.all(got["status"][keep] == 0)
    for s in (2, 6):
        assert np.all(np.isnan(got["values"][s])) and got["max_index"][s] == -1
        assert np.isnan(got["sw2_squared"][s]) and np.isnan(got["std_error"][s]) and np.isnan(got["max_sliced"][s])
    for k in KEYS:
        assert _same_bits(got[k][keep], good[k]), k


def test_projections_beyond_float32_in_one_song():
    """float32 rows of 1e18 (finite norms) against a direction of 1e25: that song's projections overflow, nothing else does"""
    x, rows, t = _case("roles-swap", "fp32")
    lens = SHAPES["roles-swap"][1]
    off = _offsets(lens)
    t = t.copy()
    t[2] = 0
    t[2, 3] = 1e25
    x, rows = x * np.float32(1e-12), rows * np.float32(1e-12)                          # the other projections stay finite
    good = _indiv(x, rows, lens, t, "fp32")
    assert np.all(good["status"] == 0)
    big = rows.copy()
    big[off[4]:off[5]] = 1e18
    got = _indiv(x, big, lens, t, "fp32")
    assert got["status"][4] == NOT_FINITE and np.all(np.isnan(got["values"][4])) and got["max_index"][4] == -1
    keep = [0, 1, 2, 3, 5, 6]
    assert np.all(got["status"][keep] == 0)
    for k in KEYS:
        assert _same_bits(got[k][keep], good[k][keep]), k


def test_a_bad_baseline_refuses_the_call_and_leaves_the_outputs():
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x, rows, t = _case("roles-swap", "fp32")
    lens = SHAPES["roles-swap"][1]
    off, S, L, n, m = _offsets(lens), 7, len(t), len(x), len(rows)
    outs = [np.full(S, -7.0) for _ in range(3)]
    idx, status = np.full(S, 99, np.int64), np.full(S, 55, np.int32)
    vals, sx, sr = np.full((S, L), -7.0), np.full((L, n), -7.0, np.float32), np.full((L, m), -7.0, np.float32)
    det = _capi.FadSlicedIndividualDetail(vals.ctypes.data, sx.ctypes.data, sr.ctypes.data)

    def call(xa, th=t):
        return lib.fad_sliced_individual(xa.ctypes.data, n, 37, rows.ctypes.data, m, 37, off.ctypes.data_as(C.POINTER(C.c_int64)), S, 37,
                                         _capi.FAD_F32, 0, th.ctypes.data, L, outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data,
                                         idx.ctypes.data, status.ctypes.data, C.byref(det), 0, None)
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[129, 36] = bad
        assert call(xb) == NOT_FINITE
    tb = t.copy()
    tb[2] = 1e25
    assert call(np.full((n, 37), 1e18, np.float32), tb) == NOT_FINITE                  # finite norms, baseline projections beyond float32
    assert all(np.all(o == -7.0) for o in outs) and np.all(idx == 99) and np.all(status == 55)
    assert np.all(vals == -7.0) and np.all(sx == -7.0) and np.all(sr == -7.0)
    assert call(x) == 0 and np.all(status == 0) and np.all(vals > 0) and np.all(sx != -7.0) and np.all(sr != -7.0)


# ----------------------------------------------------------------------------------------------------- the Python layer, the command line
def test_python_layer_and_split_calls():
    from fadtk_amd import calc_sliced_wasserstein, calc_sliced_wasserstein_individual, sliced_directions
    x, rows, _ = _case("empty-song", "fp32")
    lens = SHAPES["empty-song"][1]
    off = _offsets(lens)
    songs = [rows[off[s]:off[s + 1]] for s in range(len(lens))]
    res = calc_sliced_wasserstein_individual(x, songs, projections=16, seed=4, per_direction=True)
    assert res["values"].shape == (4, 16) and (res["n"], res["projections"], res["seed"]) == (257, 16, 4)
    assert np.array_equal(res["rows"], np.array(lens, dtype=np.float64)) and list(res["status"]) == [0, 0, TOO_FEW, 0]
    for s in (0, 1, 3):
        one = calc_sliced_wasserstein(x, songs[s], projections=16, seed=4, per_direction=True)
        assert _same_bits(res["values"][s], one["values"])
        for k in ("sw2_squared", "sliced_w2", "std_error", "max_sliced", "max_index", "fad_scale"):
            assert res[k][s] == one[k], (s, k)
    assert np.isnan(res["sw2_squared"][2]) and np.isnan(res["fad_scale"][2]) and res["max_index"][2] == -1
    split = calc_sliced_wasserstein_individual(x, songs, projections=16, seed=4, per_direction=True, max_bytes=1)   # a call per song
    for k in ("values", "sw2_squared", "std_error", "max_sliced", "max_index", "status"):
        assert _same_bits(split[k], res[k]), k
    mixed = calc_sliced_wasserstein_individual(x.astype(np.float16), songs, projections=16, seed=4)      # mixed dtypes go to float32
    want = calc_sliced_wasserstein_individual(x.astype(np.float16).astype(np.float32), songs, projections=16, seed=4)
    assert _same_bits(mixed["sw2_squared"], want["sw2_squared"])
    own = calc_sliced_wasserstein_individual(_dev(x, "fp32"), [_dev(y, "fp32") for y in songs], directions=sliced_directions(64, 16, 4))
    assert _same_bits(own["sw2_squared"], res["sw2_squared"]) and own["seed"] is None


def test_command_line_indiv_on_two_cached_directories(tmp_path):
    from fadtk_amd import calc_sliced_wasserstein_individual, sliced
    rng = np.random.default_rng(3)
    base, evl = tmp_path / "base", tmp_path / "evl"
    for d, sizes, shift in ((base, (40, 41, 42), 0.0), (evl, (25, 31, 1, 12), 0.5)):
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i, rows in enumerate(sizes):
            (d / f"f{i}.wav").write_bytes(b"")                  # the audio itself is never read: every file has its cache
            e = (rng.standard_normal((rows, 128)) + shift * (i + 1)).astype(np.float32)
            if d is evl and i == 3:
                e[5, 7] = np.inf                                # a file that is not finite: logged and dropped
            np.save(d / "embeddings" / "vggish" / f"f{i}.npy", e)
    csv = tmp_path / "out" / "indiv.csv"
    sliced.main(["vggish", str(base), str(evl), str(csv), "--projections", "16", "--seed", "2", "-w", "2", "--indiv"])
    lines = csv.read_text().splitlines()
    assert lines[0] + "\n" == sliced.INDIV_CSV_HEADER and len(lines) == 4
    cells = [dict(zip(sliced.INDIV_CSV_HEADER.strip().split(","), ln.split(","))) for ln in lines[1:]]
    assert sorted(_name(c["file"]) for c in cells) == ["f0.wav", "f1.wav", "f2.wav"]
    sw = [float(c["sw2_squared"]) for c in cells]
    assert sw == sorted(sw, reverse=True)
    x = np.concatenate([np.load(base / "embeddings" / "vggish" / (f.stem + ".npy")) for f in base.glob("*.*")])
    songs = {f"f{i}.wav": np.load(evl / "embeddings" / "vggish" / f"f{i}.npy") for i in range(3)}
    names = list(songs)
    want = calc_sliced_wasserstein_individual(x, [songs[k] for k in names], projections=16, seed=2)
    for c in cells:
        s = names.index(_name(c["file"]))
        assert c["rows"] == str(len(songs[names[s]]))
        for k in ("sw2_squared", "sliced_w2", "std_error", "fad_scale"):
            assert c[k] == repr(float(want[k][s])), (c["file"], k)
