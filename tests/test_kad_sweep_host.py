"""KAD at several bandwidths (fad_kad_sweep), the parts that need no GPU: the argument checks of hip.kad_sweep,
calc_kernel_audio_distance_sweep and KernelAudioDistance.score_sweep come before the native library is touched; the command line refuses
its flag conflicts before any file is read; the mixture value is MMD^2 under the averaged kernel; header and ctypes agree."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import kad_kernels_reference as KR

ROOT = Path(__file__).resolve().parent.parent
X = np.zeros((4, 3), dtype=np.float32)


@pytest.fixture
def no_library(monkeypatch):
    from fadtk_amd import _capi

    def refuse(*a, **k):
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(_capi, "load_library", refuse)


def _entries():
    import fadtk_amd
    from fadtk_amd import hip, kad
    obj = kad.KernelAudioDistance.__new__(kad.KernelAudioDistance)              # no model, no files: the checks come first
    return [lambda **k: hip.kad_sweep(X, X, **k), lambda **k: fadtk_amd.calc_kernel_audio_distance_sweep(X, X, **k),
            lambda **k: obj.score_sweep("a", "b", **k)]


BAD_LISTS = {"empty": [], "33 entries": [1.0] * 33, "zero": [1.0, 0.0, 2.0], "negative": [1.0, -2.0], "nan": [float("nan")],
             "inf": [1.0, float("inf")]}


@pytest.mark.parametrize("what", ["bandwidths", "factors"])
@pytest.mark.parametrize("bad", list(BAD_LISTS))
def test_a_bad_list_is_a_value_error_before_the_library_loads(no_library, what, bad):
    for call in _entries():
        with pytest.raises(ValueError, match="KAD sweep"):
            call(**{what: BAD_LISTS[bad]}, **({"factors": None} if what == "bandwidths" else {}))


def test_both_or_neither_is_a_value_error_before_the_library_loads(no_library):
    from fadtk_amd import hip
    for call in _entries():
        with pytest.raises(ValueError, match="KAD sweep"):
            call(bandwidths=[1.0], factors=[1.0])
        with pytest.raises(ValueError, match="KAD sweep"):
            call(bandwidths=None, factors=None)
    with pytest.raises(ValueError, match="KAD sweep"):
        hip.kad_sweep(X, X)                                                     # hip.kad_sweep has no default ladder


def test_unknown_kernel_is_a_value_error_before_the_library_loads(no_library):
    for call in _entries():
        for bad in ("laplace", "IQ", "", None, 1):
            with pytest.raises(ValueError, match="kernel"):
                call(factors=[1.0], kernel=bad)


def test_signatures():
    import fadtk_amd
    from fadtk_amd import hip, kad
    assert fadtk_amd.calc_kernel_audio_distance_sweep is kad.calc_kernel_audio_distance_sweep and fadtk_amd.KadSweep is kad.KadSweep
    for fn in (hip.kad_sweep, kad.calc_kernel_audio_distance_sweep, kad.KernelAudioDistance.score_sweep):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "kernel" and params["kernel"].default == "gaussian", fn
    assert inspect.signature(hip.kad_sweep).parameters["factors"].default is None
    assert tuple(inspect.signature(kad.calc_kernel_audio_distance_sweep).parameters["factors"].default) == (0.25, 0.5, 1, 2, 4)
    v, rel = hip.kad_sweep_bandwidths(factors=(0.25, 4, 1))
    assert v.dtype == np.float64 and v.tolist() == [0.25, 4.0, 1.0] and rel == 1                    # the caller's order
    v, rel = hip.kad_sweep_bandwidths(bandwidths=np.arange(1, 33))
    assert v.size == 32 and rel == 0


@pytest.mark.parametrize("kernel", KR.KERNELS)
def test_mixture_is_mmd2_under_the_averaged_kernel(monkeypatch, kernel):
    """values[b] from the float64 reference at each bandwidth; their mean against MMD^2 computed from the AVERAGED kernel matrices:
    equal by linearity, up to the order of the float64 sums (1e-13)."""
    from fadtk_amd import hip, kad
    rng = np.random.default_rng(7)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    y = (rng.standard_normal((40, 16)) * 1.1 + 0.3).astype(np.float32)
    med = KR.median_distance(x)
    factors = (0.25, 0.5, 1, 2, 4)
    sigmas = [f * med for f in factors]
    seen = {}

    def fake(xa, ya, bandwidths=None, factors=None, device=0, kernel="gaussian"):
        seen.update(bandwidths=bandwidths, factors=factors, kernel=kernel)
        sig = [f * med for f in factors] if bandwidths is None else list(bandwidths)
        rows = [KR.kad(xa, ya, s, kernel) for s in sig]
        out = {k: np.array([r[k] for r in rows]) for k in ("mmd2", "kxx_mean", "kyy_mean", "kxy_mean", "bandwidth")}
        out.update(n=len(xa), m=len(ya))
        return out
    monkeypatch.setattr(hip, "kad_sweep", fake)

    def mean_k(a, b, same):
        return KR._mean(sum(KR.kmat(a, b, s, kernel) for s in sigmas) / len(sigmas), same)
    want = mean_k(x, x, True) + mean_k(y, y, True) - 2.0 * mean_k(x, y, False)
    scale = mean_k(x, x, True) + mean_k(y, y, True) + 2.0 * mean_k(x, y, False)

    r = kad.calc_kernel_audio_distance_sweep(x, y, kernel=kernel)                # the default ladder
    assert seen == {"bandwidths": None, "factors": kad.SWEEP_FACTORS, "kernel": kernel}
    assert isinstance(r, kad.KadSweep) and r.kernel == kernel and r.scale == 1.0 and r.values.shape == (5,)
    assert np.array_equal(r.bandwidths, np.array(sigmas)) and r.details["n"] == 40
    assert abs(r.mixture - want) <= 1e-13 * scale, (r.mixture, want)
    assert r.mixture == float(np.mean(r.values))
    r10 = kad.calc_kernel_audio_distance_sweep(x, y, bandwidths=sigmas, scale=10.0, kernel=kernel)  # bandwidths override the default
    assert seen["bandwidths"] == sigmas and seen["factors"] is None
    assert np.array_equal(r10.values, 10.0 * r.values) and abs(r10.mixture - 10.0 * want) <= 1e-12 * scale and r10.scale == 10.0


def test_shape_rules_are_those_of_the_single_entry(no_library):
    from fadtk_amd import kad
    for a, b in ((np.zeros(4), X), (X, np.zeros((4, 5), dtype=np.float32)), (X[:1], X)):
        with pytest.raises(ValueError, match="KAD"):
            kad.calc_kernel_audio_distance_sweep(a, b)


# ---------------------------------------------------------------------------------------------------------- command line
CONFLICTS = [("--bandwidths", "1,2", "--bandwidth-factors", "1,2"), ("--bandwidths", "1,2", "--bandwidth", "3"),
             ("--bandwidth-factors", "1,2", "--bandwidth", "3"), ("--bandwidths", "1,2", "--indiv"), ("--bandwidth-factors", "1", "--indiv"),
             ("--bandwidths", "1,,2"), ("--bandwidths", "1,0"), ("--bandwidth-factors", "-1"), ("--bandwidth-factors", "nan"),
             ("--bandwidths", ",".join(["1"] * 33))]


@pytest.mark.parametrize("flags", CONFLICTS, ids=[" ".join(f) for f in CONFLICTS])
def test_command_line_refuses_flag_conflicts_before_any_file_is_read(flags, tmp_path, monkeypatch, capsys):
    from fadtk_amd import kad

    def no_files(*a, **k):
        raise AssertionError("the command line went on to read files")
    monkeypatch.setattr(kad.KernelAudioDistance, "__init__", no_files)
    monkeypatch.chdir(tmp_path)
    csv = tmp_path / "out.csv"
    with pytest.raises(SystemExit) as e:
        kad.main(["vggish", str(tmp_path / "none"), str(tmp_path / "none"), str(csv), *flags])
    assert e.value.code == 2                                                    # argparse's error
    assert "usage:" in capsys.readouterr().err
    assert not csv.exists() and not list(tmp_path.iterdir())


# ------------------------------------------------------------------------------------------------------ header and ctypes
def test_header_declares_and_capi_binds_the_entry():
    from fadtk_amd import _capi
    C = _capi.C
    text = (ROOT / "include" / "fad_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+FAD_KAD_MAX_BANDWIDTHS\s+32\b", code)
    m = re.search(r"\bint\s+fad_kad_sweep\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["const void* x", "int64_t n", "int64_t ldx", "const void* y", "int64_t m", "int64_t ldy", "int64_t d", "int dtype",
                    "int on_device", "const double* bandwidths", "int n_bw", "int relative", "int kernel", "fad_kad_result_t* out", "int device",
                    "void* stream"]
    res, sig = _capi.SIGNATURES["fad_kad_sweep"]
    k = _capi.SIGNATURES["fad_kad_k"][1]
    at = k.index(C.c_double)                                                    # fad_kad_k's `double bandwidth, int kernel` becomes the list
    assert res is C.c_int and sig == k[:at] + [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int] + k[at + 2:]
    from fadtk_amd import hip
    assert hip.KAD_MAX_BANDWIDTHS == 32
    if _capi.LIB_PATH.exists():
        assert hasattr(_capi.load_library(), "fad_kad_sweep")
