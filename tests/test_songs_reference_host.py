"""The per-song reference of the GPU tests (songs_reference.py) held to the oracle of score_individual (fad.py:373-387), and the
argument checks of fad_frechet_batched_vs_baseline, which return before any device call.  No GPU needed."""
import ctypes as C
import logging

import numpy as np
import pytest

import songs_reference as SR
from oracle import fad_oracle as O

logging.getLogger("fad_oracle").setLevel(logging.CRITICAL)


def _baseline(seed, d):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((4 * d + 8, d)) * (0.6 + rng.random(d)) + 0.2 * rng.standard_normal(d)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def _song(rng, n, d, dtype):
    return (rng.standard_normal((n, d)) * (0.5 + rng.random(d)) + 0.5).astype(dtype)


@pytest.mark.parametrize("d", [1, 5, 17, 64, 96])
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_reference_matches_the_oracle(d, dtype):
    rng = np.random.default_rng(d)
    mu_b, cov_b = _baseline(100 + d, d)
    full = [_song(rng, n, d, dtype) for n in (d + 1, 2 * d + 3, 8 * d + 1)]
    deficient = [_song(rng, n, d, dtype) for n in (2, 3, max(2, d // 2))]
    rep = _song(rng, max(4, d // 3), d, dtype)
    rep[2:] = rep[1]                                              # repeated frames
    flat = np.tile(_song(rng, 1, d, dtype), (d + 3, 1))           # Sigma_s = 0
    bad = _song(rng, d + 4, d, dtype)
    bad[-1, d // 2] = np.nan
    one = _song(rng, 1, d, dtype)
    songs = full + deficient + [rep, flat, bad, one]
    want = O.individual_scores(mu_b, cov_b, songs, run_sqrtm=False)
    got = SR.individual_scores(mu_b, cov_b, songs, mean_mode=1)
    for k, (g, w) in enumerate(zip(got, want)):
        if k >= len(songs) - 2:
            assert g is None and w is None, (k, g, w)
            continue
        # full rank: both are float64 to the last digits; rank deficient: the oracle's eig returns the zero eigenvalues as
        # +-1e-16 and takes their roots, so it is only good to ~sqrt(eps) of the trace
        rtol = 1e-9 if k < len(full) else 2e-7
        assert abs(g - w) <= rtol * abs(w), (k, g, w)


def test_reference_mean_modes_and_bfloat16():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    d = 24
    x = rng.standard_normal((300, d)) * 0.3 + 3.0
    for dtype in (np.float16, np.float32):
        a = x.astype(dtype)
        assert np.array_equal(SR.song_mean(a, 1), np.mean(a, axis=0).astype(np.float64))
        assert np.array_equal(SR.song_mean(a, 0), a.astype(np.float64).mean(axis=0))
    b = torch.from_numpy(x).to(torch.bfloat16)
    m1 = SR.song_mean(b, 1)
    assert np.array_equal(m1, torch.from_numpy(m1).to(torch.bfloat16).double().numpy())        # a bfloat16 value
    exact32 = np.mean(b.float().numpy(), axis=0)
    assert np.abs(m1 - exact32).max() <= 2.0 ** -8 * np.abs(exact32).max()
    mu_b, cov_b = _baseline(4, d)
    base = SR.Baseline(mu_b, cov_b)
    assert base.score(b, 1) != base.score(b, 0)
    nan_cov = cov_b.copy()
    nan_cov[1, 2] = np.nan
    assert SR.Baseline(mu_b, nan_cov).score(x[:10], 1) is None


# --------------------------------------------------------------------------------- argument checks (C ABI, no device call)
def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def _call(lib, d, rows, n_rows, ld, dtype, offsets, n_songs, scores, status):
    mu = np.zeros(d); cov = np.eye(d)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    return lib.fad_frechet_batched_vs_baseline(d, mu.ctypes.data, cov.ctypes.data, rows.ctypes.data, n_rows, ld, dtype,
                                               off.ctypes.data_as(C.POINTER(C.c_int64)), n_songs, 1, 0, 0, None,
                                               scores.ctypes.data, status.ctypes.data)


def test_batched_vs_baseline_rejects_bad_arguments_before_any_device_call():
    K, lib = _lib()
    d = 8
    rows = np.zeros((10, d), dtype=np.float32)
    scores = np.full(3, 7.0); status = np.full(3, 5, dtype=np.int32)
    assert _call(lib, d, rows, 10, d, K.FAD_F32, [0, 6, 4], 2, scores, status) == K.FAD_ERR_INVALID      # decreasing
    assert _call(lib, d, rows, 10, d, K.FAD_F32, [0, 4, 11], 2, scores, status) == K.FAD_ERR_INVALID     # past n_rows
    assert _call(lib, d, rows, 10, d, K.FAD_F32, [-1, 4], 1, scores, status) == K.FAD_ERR_INVALID        # before row 0
    assert _call(lib, d, rows, 10, d - 1, K.FAD_F32, [0, 4], 1, scores, status) == K.FAD_ERR_SHAPE       # ld < d
    assert _call(lib, d, rows, 10, d, 7, [0, 4], 1, scores, status) == K.FAD_ERR_INVALID                 # unknown dtype
    assert _call(lib, 0, rows, 10, d, K.FAD_F32, [0, 4], 1, scores, status) == K.FAD_ERR_INVALID         # d < 1
    assert np.all(scores == 7.0) and np.all(status == 5)                                                 # nothing written
    assert _call(lib, d, rows, 10, d, K.FAD_F32, [3], 0, scores, status) == K.FAD_OK                     # no songs: nothing to do
    assert np.all(scores == 7.0) and np.all(status == 5)
