"""KAD at several bandwidths in one fused pass (fad_kad_sweep, csrc/kad.hip) on the GPU: every entry against the single-bandwidth entry
fad_kad_k bit for bit (dtypes, D, kernels, the smallest sets, a row pitch), the group edges (a padded group, a second and a fourth
group, duplicates, a shuffled ladder, a second run), float64 accuracy at the factors 0.5, 1 and 2 at the tolerances of DESIGN 4.6, the
absolute mode and torch rows, the refusals (which leave `out` as it was), the Python layer and the command line.

n = 255 and m = 257 are the smallest sets with a diagonal tile's mask, ragged last tiles and several tiles in every pass; both entries
make one launch per pass there, so their float64 sums are added in the same order and equality is exact."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kad_conditioning_reference as CR
import kad_kernels_reference as KR
from test_gpu_kad import MEAN_RTOL, MMD_TOL

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
N, M = 255, 257
FACTORS = (0.25, 0.5, 1, 2, 4)
ACCURACY_FACTORS = (0.5, 1, 2)
DTYPES = ("fp16", "bf16", "fp32")
DIMS = (17, 128, 512)
FIELDS = ("mmd2", "kxx_mean", "kyy_mean", "kxy_mean", "bandwidth")
INVALID, TOO_FEW, NOT_FINITE = -1, -6, -7
assert MEAN_RTOL == 4e-7 and MMD_TOL == 1.5e-7
WORST = {}                                                # kernel -> [worst mean error, worst mmd2 error] over the accuracy cases


def _rows(a, dt):
    """float32 values that are exact in dt -> fp16 and fp32 numpy on the host, bf16 a torch tensor on the device"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == "bf16":
        return torch.from_numpy(a).cuda().bfloat16()
    return a.astype(np.float16) if dt == "fp16" else a


@functools.lru_cache(maxsize=None)
def _values(d, dt):
    """the sets of a case as float32 values of dtype dt"""
    x, y = CR.offset_gauss(N, M, d, 0, seed=d, shift=1)
    return CR.round_to(x, dt), CR.round_to(y, dt)


@functools.lru_cache(maxsize=None)
def _case(d, dt, kernel):
    """One sweep over FACTORS and what it is compared with, computed once: the median, the sweep's arrays and the float64 rows."""
    from fadtk_amd import hip
    xv, yv = _values(d, dt)
    x, y = _rows(xv, dt), _rows(yv, dt)
    return {"x": x, "y": y, "xv": xv, "yv": yv, "median": hip.kad_median_distance(x),
            "sweep": hip.kad_sweep(x, y, factors=FACTORS, kernel=kernel)}


def _same_as_single(sweep, b, single):
    for k in FIELDS:
        assert np.float64(sweep[k][b]).tobytes() == np.float64(single[k]).tobytes(), (b, k, sweep[k][b], single[k])
    assert sweep["n"] == single["n"] and sweep["m"] == single["m"]


# ------------------------------------------------------------------------------------------ 1. equality with the single entry
@pytest.mark.parametrize("kernel", KR.KERNELS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_every_entry_carries_the_bits_of_the_single_call(d, dt, kernel):
    from fadtk_amd import hip
    c = _case(d, dt, kernel)
    sw = c["sweep"]
    assert sw["n"] == N and sw["m"] == M and all(sw[k].shape == (len(FACTORS),) and sw[k].dtype == np.float64 for k in FIELDS)
    for b, f in enumerate(FACTORS):
        assert sw["bandwidth"][b] == f * c["median"]
        _same_as_single(sw, b, hip.kad(c["x"], c["y"], bandwidth=f * c["median"], kernel=kernel))
    _same_as_single(sw, FACTORS.index(1), hip.kad(c["x"], c["y"], kernel=kernel))              # the factor 1 is the default call
    assert np.all(np.diff(sw["kxx_mean"]) > 0) and np.all(np.diff(sw["kxy_mean"]) > 0)           # a wider kernel, larger means


@pytest.mark.parametrize("kernel", KR.KERNELS)
def test_smallest_sets(kernel):
    from fadtk_amd import hip
    x = np.array([[0.5], [-1.25]], dtype=np.float16)
    y = np.array([[0.25], [2.0], [-0.75]], dtype=np.float16)
    sw = hip.kad_sweep(x, y, factors=FACTORS, kernel=kernel)
    assert sw["n"] == 2 and sw["m"] == 3
    med = hip.kad_median_distance(x)
    assert med == 1.75
    for b, f in enumerate(FACTORS):
        _same_as_single(sw, b, hip.kad(x, y, bandwidth=f * med, kernel=kernel))


@pytest.mark.parametrize("dt", ["float16", "bfloat16", "float32"])
def test_row_pitch_on_device_rows(dt):
    import torch
    from fadtk_amd import hip
    d, ld = 17, 24
    xv, yv = _values(d, "fp32")
    tdt = getattr(torch, dt)
    xw = torch.zeros((N, ld), dtype=tdt, device="cuda")
    yw = torch.full((M, ld + 8), 7.0, dtype=tdt, device="cuda")              # what lies past D is not read
    xw[:, :d] = torch.from_numpy(xv).to(tdt)
    yw[:, :d] = torch.from_numpy(yv).to(tdt)
    x, y = xw[:, :d], yw[:, :d]
    sw = hip.kad_sweep(x, y, factors=FACTORS, kernel="iq")
    med = hip.kad_median_distance(x)
    for b, f in enumerate(FACTORS):
        _same_as_single(sw, b, hip.kad(x, y, bandwidth=f * med, kernel="iq"))
    packed = hip.kad_sweep(x.contiguous(), y.contiguous(), factors=FACTORS, kernel="iq")
    assert all(np.array_equal(sw[k], packed[k]) for k in FIELDS)


# -------------------------------------------------------------------------------------------------------------- 2. group edges
@functools.lru_cache(maxsize=None)
def _singles(kernel, sigmas):
    from fadtk_amd import hip
    c = _case(128, "fp16", kernel)
    return {s: hip.kad(c["x"], c["y"], bandwidth=s, kernel=kernel) for s in set(sigmas)}


@pytest.mark.parametrize("n_bw", [1, 2, 3, 8, 9, 17, 32])
def test_group_edges(n_bw):
    """Groups of at most 8: a group of one runs the single kernel, 2 and 3 a padded group of 4, 9 = 8 + 1, 17 = 8 + 8 + 1, 32 four
    full groups.  A geometric ladder inside [0.25, 4] in shuffled order, a duplicate pair at 0 and 8 (two groups)."""
    from fadtk_amd import hip
    c = _case(128, "fp16", "gaussian")
    ladder = 0.25 * 16.0 ** (np.arange(32) / 31.0)
    factors = np.random.default_rng(n_bw).permutation(ladder)[:n_bw]
    if n_bw > 8:
        factors[8] = factors[0]
    assert factors.min() >= 0.25 and factors.max() <= 4.0 and len(set(factors)) == n_bw - (n_bw > 8)
    sw = hip.kad_sweep(c["x"], c["y"], factors=factors)
    sigmas = tuple(float(f) * c["median"] for f in factors)
    assert sw["bandwidth"].tolist() == list(sigmas)
    singles = _singles("gaussian", sigmas)
    for b, s in enumerate(sigmas):
        _same_as_single(sw, b, singles[s])
    if n_bw > 8:
        assert all(sw[k][0].tobytes() == sw[k][8].tobytes() for k in FIELDS)
    again = hip.kad_sweep(c["x"], c["y"], factors=factors)
    assert all(sw[k].tobytes() == again[k].tobytes() for k in FIELDS)               # no float atomics: the same bits on every run


# ------------------------------------------------------------------------------------------------------- 3. float64 accuracy
@pytest.mark.parametrize("kernel", KR.KERNELS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_float64_accuracy_at_half_one_and_two(d, dt, kernel):
    """Each mean within MEAN_RTOL + 4 A kappa_b of the float64 reference at sigma_b, MMD^2 within MMD_TOL of Kxx + Kyy + 2 Kxy (DESIGN
    4.6's rule; the tolerances of a mean run from 4.0e-7 to 6.5e-7 here).  The float32 chain emulation (KR.chain32_means) over the 81
    combinations of dtype, D, kernel and factor leaves 4.1e-8 on a mean and 1.9e-9 on MMD^2 at worst, the smallest mean 0.087; the
    MI355X 1.1e-7 and 9.7e-9 (profiles/kad_sweep_err.txt).  The factor 0.25 is held by the equality test alone: the emulation has no
    float32 rounding of c S' and no v_exp_f32, so no tolerance there has been measured."""
    c = _case(d, dt, kernel)
    sw = c["sweep"]
    A = CR.conditioning_constant(dt)
    worst = WORST.setdefault(kernel, [0.0, 0.0])
    for f in ACCURACY_FACTORS:
        b = FACTORS.index(f)
        sigma = sw["bandwidth"][b]
        want = KR.kad(c["xv"], c["yv"], sigma, kernel)
        tol = MEAN_RTOL + 4 * A * CR.kappa(c["xv"], c["yv"], sigma)
        got = {k: sw[k][b] for k in FIELDS}
        err = CR.mean_errors(got, want)
        worst[0] = max(worst[0], *(err[k] for k in CR.MEANS))
        worst[1] = max(worst[1], err["mmd2"])
        print(f"[kad-sweep] {kernel} {dt} d={d} factor={f}: tol {tol:.2e}; " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
        for k in CR.MEANS:
            assert err[k] <= tol, (k, f, err[k], tol)
        assert err["mmd2"] <= MMD_TOL, (f, err["mmd2"])
    print(f"[kad-sweep] worst so far, {kernel}: mean {worst[0]:.2e} mmd2/scale {worst[1]:.2e}")


# ------------------------------------------------------------------------------------------ 4. absolute mode and torch input
@pytest.mark.parametrize("kernel", KR.KERNELS)
def test_absolute_mode_and_torch_rows(kernel):
    import torch
    from fadtk_amd import hip
    c = _case(128, "fp16", kernel)
    sigmas = [f * c["median"] for f in FACTORS]
    absolute = hip.kad_sweep(c["x"], c["y"], bandwidths=sigmas, kernel=kernel)
    assert all(absolute[k].tobytes() == c["sweep"][k].tobytes() for k in FIELDS)
    xd, yd = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["y"]).cuda()
    before = (xd.clone(), yd.clone())
    for a, b in ((xd, yd), (c["x"], yd), (xd, c["y"])):                             # in place; a numpy set next to a CUDA set
        got = hip.kad_sweep(a, b, factors=FACTORS, kernel=kernel)
        assert all(got[k].tobytes() == c["sweep"][k].tobytes() for k in FIELDS)
    assert torch.equal(xd, before[0]) and torch.equal(yd, before[1])


# ------------------------------------------------------------------------------------------------------------------ 5. errors
def _raw(x, y, values, relative, kernel=0, n=None, n_bw=None):
    """fad_kad_sweep through ctypes on float32 host rows with `out` filled by the caller -> (status, message, out untouched?)"""
    from fadtk_amd import _capi
    lib = _capi.load_library()
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = (_capi.FadKadResult * 32)()
    for r in out:
        r.mmd2, r.kxx_mean, r.kyy_mean, r.kxy_mean, r.bandwidth, r.n, r.m = 1.5, 2.5, 3.5, 4.5, 5.5, -6, -7
    st = lib.fad_kad_sweep(x.ctypes.data, len(x) if n is None else n, x.shape[1], y.ctypes.data, len(y), y.shape[1], x.shape[1], _capi.FAD_F32, 0,
                           v.ctypes.data_as(C.POINTER(C.c_double)), len(v) if n_bw is None else n_bw, relative, kernel, out, 0, None)
    untouched = all((r.mmd2, r.kxx_mean, r.kyy_mean, r.kxy_mean, r.bandwidth, r.n, r.m) == (1.5, 2.5, 3.5, 4.5, 5.5, -6, -7) for r in out)
    return st, _capi.last_error() if st else "", untouched


def test_errors_leave_out_untouched():
    from fadtk_amd import hip
    x = np.random.default_rng(0).standard_normal((50, 16)).astype(np.float32)
    same = np.repeat(np.round(x[:1] * 4), 10, axis=0)                              # every baseline distance is exactly 0
    st, msg, untouched = _raw(same, x, [0.5, 1, 2], 1)
    assert st == INVALID and "must be > 0" in msg and untouched, msg
    st, msg, untouched = _raw(same, x, [3.0, 4.0], 0)                              # absolute bandwidths need no median
    assert st == 0 and not untouched
    for kernel in (0, 1, 2):
        st, msg, untouched = _raw(x, x, [4.0, 5.0, 1e-30, 6.0], 0, kernel)         # c past float32 between valid entries
        assert st == INVALID and "float32 range" in msg and "bandwidth 2 " in msg and untouched, msg
    st, msg, untouched = _raw(x, x, [1.0, 1e30], 1)
    assert st == INVALID and "bandwidth 1 " in msg and untouched, msg
    bad = x.copy()
    bad[7, 3] = np.inf
    for a, b in ((bad, x), (x, bad)):
        st, msg, untouched = _raw(a, b, [0.5, 1, 2], 1)
        assert st == NOT_FINITE and untouched, msg
    st, msg, untouched = _raw(x, x, [1.0], 1, n=1)
    assert st == TOO_FEW and untouched, msg
    for values, n_bw in (([1.0], 0), ([1.0] * 32, 33), ([1.0, 0.0], None), ([1.0, -1.0], None), ([np.nan], None), ([np.inf, 1.0], None)):
        for relative in (0, 1):
            st, msg, untouched = _raw(x, x, values, relative, n_bw=n_bw)
            assert st == INVALID and "fad_kad_sweep" in msg and untouched, (values, msg)
    st, msg, untouched = _raw(x, x, [1.0], 1, kernel=3)
    assert st == INVALID and "kernel 3" in msg and untouched, msg
    with pytest.raises(RuntimeError, match="must be > 0"):
        hip.kad_sweep(same, x, factors=[1.0])
    with pytest.raises(ValueError):
        hip.kad_sweep(bad, x, factors=[1.0])
    with pytest.raises(AssertionError):
        hip.kad_sweep(x[:1], x, factors=[1.0])
    assert np.all(np.isfinite(hip.kad_sweep(x, x[:20], factors=[1.0, 2.0])["mmd2"]))           # the call after errors


# ------------------------------------------------------------------------------------------------------ 6. Python and CLI
@pytest.mark.parametrize("kernel", ["gaussian", "imq"])
def test_python_layer_matches_the_single_function(kernel):
    import fadtk_amd
    c = _case(128, "fp16", kernel)
    r = fadtk_amd.calc_kernel_audio_distance_sweep(c["x"], c["y"], scale=100.0, kernel=kernel)
    assert isinstance(r, fadtk_amd.KadSweep) and r.kernel == kernel and r.scale == 100.0
    assert r.bandwidths.tolist() == [f * c["median"] for f in FACTORS]
    for b, s in enumerate(r.bandwidths):
        assert r.values[b] == fadtk_amd.calc_kernel_audio_distance(c["x"], c["y"], bandwidth=s, scale=100.0, kernel=kernel)
    assert r.mixture == float(np.mean(r.values)) and r.details["n"] == N
    given = fadtk_amd.calc_kernel_audio_distance_sweep(c["x"], c["y"], bandwidths=r.bandwidths[::-1], scale=100.0, kernel=kernel)
    assert np.array_equal(given.values, r.values[::-1]) and np.array_equal(given.bandwidths, r.bandwidths[::-1])


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """Six tiny cached files per directory (the fixture of test_gpu_kad_kernels.py) -> (run, tmp, base dir, eval dir, x rows, y rows)"""
    from fadtk_amd import FrechetAudioDistance
    from fadtk_amd.model_loader import get_all_models
    tmp = tmp_path_factory.mktemp("kad_sweep_cli")
    rng = np.random.default_rng(5)
    for name, shift in (("base", 0.0), ("evl", 0.4)):
        d = tmp / name
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i in range(6):
            (d / f"s{i}.wav").write_bytes(b"")             # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"s{i}.npy", (rng.standard_normal((40 + 7 * i, 128)) + shift).astype(np.float32))
    env = dict(os.environ, PYTHONPATH=str(ROOT))

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "fadtk_amd.kad", "vggish", *args, "-w", "2"], capture_output=True, text=True, cwd=tmp,
                           env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return r
    ml = {m.name: m for m in get_all_models()}["vggish"]
    fad = FrechetAudioDistance(ml, load_model=False)
    return run, tmp, str(tmp / "base"), str(tmp / "evl"), fad.load_embeddings(tmp / "base"), fad.load_embeddings(tmp / "evl")


@pytest.mark.parametrize("kernel", ["gaussian", "iq"])
def test_command_line_writes_one_row_per_bandwidth(cli, kernel):
    from fadtk_amd import calc_kernel_audio_distance, hip
    run, tmp, base, evl, x, y = cli
    csv = tmp / f"sweep_{kernel}.csv"
    r = run(base, evl, str(csv), "--scale", "10", "--bandwidth-factors", "0.5,1,2", *(["--kernel", kernel] if kernel != "gaussian" else []))
    lines = csv.read_text().splitlines()
    tail = "" if kernel == "gaussian" else ",kernel"
    assert lines[0] == "model,baseline,eval,kad,bandwidth,scale,time" + tail and len(lines) == 4
    med = hip.kad_median_distance(x)
    printed = [float(v) for v in r.stdout.split()]
    for b, f in enumerate((0.5, 1.0, 2.0)):
        row = lines[1 + b].split(",")
        value, res = calc_kernel_audio_distance(x, y, bandwidth=f * med, scale=10.0, details=True, kernel=kernel)
        assert float(row[3]) == value and float(row[4]) == res["bandwidth"] == f * med and float(row[5]) == 10.0
        assert len(row) == (7 if kernel == "gaussian" else 8) and (kernel == "gaussian" or row[7] == kernel)
        assert printed[b] == value
    assert len(printed) == 3 and "mixture" in r.stderr + r.stdout


def test_command_line_takes_absolute_bandwidths(cli):
    from fadtk_amd import calc_kernel_audio_distance, hip
    run, tmp, base, evl, x, y = cli
    csv = tmp / "absolute.csv"
    med = hip.kad_median_distance(x)
    r = run(base, evl, str(csv), "--bandwidths", f"{2 * med!r},{med!r}")
    lines = csv.read_text().splitlines()
    assert lines[0] == "model,baseline,eval,kad,bandwidth,scale,time" and len(lines) == 3
    assert [float(line.split(",")[4]) for line in lines[1:]] == [2 * med, med]                  # the caller's order
    assert float(lines[2].split(",")[3]) == calc_kernel_audio_distance(x, y) == float(r.stdout.split()[1])


def test_command_line_refusals_write_nothing(cli, capsys):
    from fadtk_amd import kad
    run, tmp, base, evl, x, y = cli
    csv = tmp / "refused.csv"
    for flags in (("--bandwidths", "1,2", "--bandwidth-factors", "1,2"), ("--bandwidth-factors", "1,2", "--bandwidth", "3"),
                  ("--bandwidths", "1,2", "--indiv"), ("--bandwidth-factors", "1,0")):
        with pytest.raises(SystemExit) as e:
            kad.main(["vggish", base, evl, str(csv), *flags])
        assert e.value.code == 2 and not csv.exists()
    capsys.readouterr()
