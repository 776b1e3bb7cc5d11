"""Lloyd's k-means (fad_kmeans), host side (no GPU): the float64 reference of tests/kmeans_reference.py against scikit-learn on
well-separated data, its tie rule and empty-cluster rule, the seeding recipe of fadtk_amd.mauve, the prototype, and the refusals of the
Python layers and of the library itself, which come before any device is opened."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("kmeans_reference", Path(__file__).resolve().parent / "kmeans_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _separated(n, k, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, d)) * 20
    which = rng.integers(0, k, n)
    return (centres[which] + rng.standard_normal((n, d))).astype(np.float32), which, centres


def test_reference_against_sklearn_on_separated_data():
    cluster = pytest.importorskip("sklearn.cluster")
    x, which, centres = _separated(600, 6, 8, 0)
    init = (centres + 0.5).astype(np.float32)
    want = cluster.KMeans(n_clusters=6, init=init, n_init=1, algorithm="lloyd", tol=0, max_iter=50).fit(x.astype(np.float64))
    got = R.lloyd(x, init, 50)
    assert got["converged"] == 1
    np.testing.assert_array_equal(got["labels"], want.labels_)
    np.testing.assert_allclose(got["centroids"], want.cluster_centers_, rtol=1e-6, atol=1e-6)
    assert got["inertia"] == pytest.approx(want.inertia_, rel=1e-9)
    np.testing.assert_array_equal(got["labels"], which)


def test_reference_loop_on_its_own_terms():
    x, which, centres = _separated(400, 5, 3, 1)
    init = x[R.seed_rows(400, 5, 0, 0)]
    got = R.lloyd(x, init, 50)
    assert got["converged"] == 1 and got["iterations"] < 50 and len(got["inertia_trace"]) == got["iterations"]
    assert (np.diff(got["inertia_trace"]) <= 0).all()
    labels, d2, _ = R.assign(x, got["centroids"])                      # the labels belong to the returned centroids
    np.testing.assert_array_equal(labels, got["labels"])
    np.testing.assert_array_equal(R.update(x, labels, got["centroids"])[0], got["centroids"])      # the fixed point
    short = R.lloyd(x, init, 1)                                        # the loop ran out: one more assignment
    assert short["converged"] == 0 and short["iterations"] == 1 and len(short["inertia_trace"]) == 2
    pure = R.lloyd(x, init, 0)
    assert pure["iterations"] == 0 and len(pure["inertia_trace"]) == 1 and np.array_equal(pure["centroids"], init)
    np.testing.assert_array_equal(pure["labels"], R.assign(x, init)[0])


def test_equal_distances_go_to_the_smaller_index():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [5.0, 5.0]])
    c = np.array([[2.0, 0.0], [0.0, 0.0], [2.0, 0.0], [0.0, 0.0]], np.float32)      # centroids 2 and 3 repeat 0 and 1; row 1 is between
    labels, d2, _ = R.assign(x, c)
    assert labels.tolist() == [1, 0, 0, 0] and d2.tolist() == [0.0, 1.0, 0.0, 34.0]


def test_an_empty_cluster_keeps_its_centroid():
    x = np.array([[0.0], [1.0], [10.0], [11.0]])
    init = np.array([[0.25], [1000.0], [10.75]], np.float32)
    got = R.lloyd(x, init, 10)
    assert got["counts"].tolist() == [2, 0, 2] and got["empty_clusters"] == 1 and got["converged"] == 1
    assert got["centroids"][:, 0].tolist() == [0.5, 1000.0, 10.5]
    cent, counts = R.update(x, np.array([0, 0, 2, 2]), init)
    assert cent[1, 0] == np.float32(1000.0) and counts.tolist() == [2, 0, 2]
    third = np.array([[1.0], [1.0], [2.0]])
    assert R.update(third, np.array([0, 0, 0]), np.zeros((1, 1), np.float32))[0][0, 0] == np.float32(4.0 / 3.0)    # float32 of the float64 mean


def test_the_seeding_recipe():
    from fadtk_amd import mauve
    rows = mauve.seed_rows(1000, 17, seed=3, restart=2)
    want = np.sort(np.random.default_rng([3, 2]).choice(1000, 17, replace=False))
    np.testing.assert_array_equal(rows, want)
    np.testing.assert_array_equal(rows, R.seed_rows(1000, 17, 3, 2))
    assert len(set(rows.tolist())) == 17 and (np.diff(rows) > 0).all()
    assert not np.array_equal(rows, mauve.seed_rows(1000, 17, seed=3, restart=3))
    assert not np.array_equal(rows, mauve.seed_rows(1000, 17, seed=4, restart=2))
    np.testing.assert_array_equal(mauve.seed_rows(5, 5, 0, 0), np.arange(5))
    a, b = np.arange(12, dtype=np.float16).reshape(4, 3), np.arange(12, 30, dtype=np.float16).reshape(6, 3)
    got = mauve._gather_rows([a, b], np.array([1, 3, 4, 9]))           # pooled rows -> float32, across the sets
    assert got.dtype == np.float32 and got.tolist() == [[3, 4, 5], [9, 10, 11], [12, 13, 14], [27, 28, 29]]
    assert mauve.default_clusters(1000, 250) == 25 and mauve.default_clusters(5, 900) == 2 and mauve.default_clusters(10 ** 7, 10 ** 7) == 65536


def test_prototype_header_and_alias():
    import fadtk.mauve as alias
    import fadtk_amd
    from fadtk_amd import _capi, mauve
    res, args = _capi.SIGNATURES["fad_kmeans"]
    assert res is C.c_int and len(args) == 18 and _capi.SIGNATURES["fad_kmeans_last_plan"] == (C.c_int, [C.POINTER(C.c_int64)])
    assert [f for f, _ in _capi.FadKmeansResult._fields_] == ["inertia", "n", "k", "iterations", "converged", "changed_last", "empty_clusters",
                                                             "assignments"]
    header = (ROOT / "include" / "fad_hip.h").read_text()
    assert re.search(r"\bint\s+fad_kmeans\s*\(", header) and "fad_kmeans_result_t" in header
    assert "int fad_kmeans_last_plan(int64_t out[6]);" in header
    lib = _capi.load_library()
    assert hasattr(lib, "fad_kmeans") and hasattr(lib, "fad_kmeans_last_plan") and lib.fad_version() == 2
    assert alias.calc_mauve is mauve.calc_mauve and alias.calc_kmeans is mauve.calc_kmeans and alias.main is mauve.main
    assert alias.CSV_HEADER == mauve.CSV_HEADER and fadtk_amd.calc_mauve is mauve.calc_mauve and fadtk_amd.Mauve is mauve.Mauve


def test_value_errors_before_the_library(monkeypatch):
    from fadtk_amd import _capi, hip, mauve

    def no_library(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load_library", no_library)
    x, y = np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32)
    for bad in (0, -3, 65537, 2.5, True):
        with pytest.raises(ValueError, match="clusters"):
            mauve.calc_kmeans(x, bad)
        with pytest.raises(ValueError, match="clusters"):
            mauve.calc_mauve(x, y, clusters=bad)
    with pytest.raises(ValueError, match="clusters"):
        mauve.calc_kmeans(x, None)
    with pytest.raises(ValueError, match="pooled rows"):
        mauve.calc_kmeans(x, 21)
    with pytest.raises(ValueError, match="pooled rows"):
        mauve.calc_mauve(x, y, clusters=51)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="iterations"):
            mauve.calc_kmeans(x, 3, iterations=bad)
        with pytest.raises(ValueError, match="seed"):
            mauve.calc_mauve(x, y, seed=bad)
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="redo"):
            mauve.calc_mauve(x, y, redo=bad)
    for bad in (0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale"):
            mauve.calc_mauve(x, y, scale=bad)
    with pytest.raises(ValueError, match="points"):
        mauve.calc_mauve(x, y, points=1)
    with pytest.raises(ValueError, match="different dimensions"):
        mauve.calc_mauve(x, np.zeros((30, 5), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        mauve.calc_mauve(x[0], y)
    with pytest.raises(ValueError, match="at least 1 row"):
        mauve.calc_mauve(x[:0], y)
    with pytest.raises(ValueError, match="outside 1 .. 2048"):
        mauve.calc_kmeans(np.zeros((3, 2049), np.float32), 2)
    with pytest.raises(ValueError, match="1 .. 8 row sets"):
        mauve.calc_kmeans([x] * 9, 2)
    with pytest.raises(ValueError, match=r"init must be \[3, 4\]"):
        mauve.calc_kmeans(x, 3, init=np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError, match="max_rows"):
        mauve.Mauve(None, max_rows=0)
    # hip.kmeans: its own checks, also before the library
    init = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="float16, bfloat16 or float32"):
        hip.kmeans(x.astype(np.float64), init)
    with pytest.raises(ValueError, match="init has D = 4"):
        hip.kmeans(np.zeros((20, 5), np.float32), init)
    with pytest.raises(ValueError, match="same dtype"):
        hip.kmeans([x, y.astype(np.float16)], init)
    with pytest.raises(ValueError, match="NaN/Inf"):
        hip.kmeans(x, np.full((3, 4), np.nan, np.float32))
    with pytest.raises(ValueError, match="iterations"):
        hip.kmeans(x, init, iterations=-1)
    with pytest.raises(ValueError, match="pooled rows"):
        hip.kmeans(x, np.zeros((21, 4), np.float32))
    with pytest.raises(ValueError, match="1 .. 8 row sets"):
        hip.kmeans([], init)


def test_library_refusals_come_before_the_device():
    """the library's own argument checks need no GPU: they come before the device is opened (FAD_ERR_NO_DEVICE where there is none)"""
    import torch
    from fadtk_amd import _capi
    lib = _capi.load_library()
    x = np.random.default_rng(0).standard_normal((50, 6)).astype(np.float32)
    init = x[:4].copy()
    cent, lab, cnt = np.full((4, 6), 7, np.float32), np.full(50, 7, np.int32), np.full(4, 7, np.int64)
    res = _capi.FadKmeansResult()

    def call(n=50, d=6, ld=6, k=4, dt=_capi.FAD_F32, ini=init, it=3, sets=1, out=C.byref(res), rows=x):
        ptrs = (C.c_void_p * max(sets, 1))(*[rows.ctypes.data if rows is not None else None] * max(sets, 1))
        ns = (C.c_int64 * max(sets, 1))(*[n] * max(sets, 1))
        lds = (C.c_int64 * max(sets, 1))(*[ld] * max(sets, 1))
        return lib.fad_kmeans(ptrs, ns, lds, sets, d, dt, 0, k, ini.ctypes.data if ini is not None else None, it, cent.ctypes.data,
                              lab.ctypes.data, cnt.ctypes.data, None, None, out, 0, None)
    INVALID = _capi.FAD_ERR_INVALID
    assert call(dt=_capi.FAD_F64) == INVALID and call(dt=99) == INVALID
    assert call(d=0) == INVALID and call(d=2049, ld=2049) == INVALID and call(ld=5) == INVALID
    assert call(k=0) == INVALID and call(k=51) == INVALID and call(k=65537) == INVALID
    assert call(it=-1) == INVALID and call(sets=0) == INVALID and call(sets=9) == INVALID
    assert call(out=None) == INVALID and call(ini=None) == INVALID and call(rows=None) == INVALID
    assert call(n=0) == _capi.FAD_ERR_TOO_FEW_ROWS
    bad = init.copy()
    bad[1, 1] = np.nan
    assert call(ini=bad) == _capi.FAD_ERR_NOT_FINITE
    assert (cent == 7).all() and (lab == 7).all() and (cnt == 7).all()
    plan = (C.c_int64 * 6)(*[9] * 6)
    assert lib.fad_kmeans_last_plan(plan) == 0 and list(plan) == [0] * 6
    assert lib.fad_kmeans_last_plan(None) == INVALID
    if not torch.cuda.is_available():
        assert call() == _capi.FAD_ERR_NO_DEVICE
