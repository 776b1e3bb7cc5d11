"""Nearest baseline rows and authenticity, host side (no GPU): the float64 reference against brute-force loops, the C ABI surface, the
errors raised before any library call, the per-song aggregation of fadtk_amd.nearest on hand-built results, and the command line."""
import ctypes as C
import importlib.util
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("nearest_reference", Path(__file__).resolve().parent / "nearest_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _lib():
    from fadtk_amd import _capi
    if not _capi.LIB_PATH.exists():
        from fadtk_amd.build import build_library
        build_library(verbose=False)
    return _capi, _capi.load_library()


def _brute(x, y, k):
    def d2(a, b):
        return float(sum((float(p) - float(q)) ** 2 for p, q in zip(a, b)))
    idx, dist = [], []
    for b in y:
        keys = sorted((d2(a, b), i) for i, a in enumerate(x))[:k]
        idx.append([i for _, i in keys])
        dist.append([v for v, _ in keys])
    r1 = [min(d2(x[i], x[j]) for j in range(len(x)) if j != i) for i in range(len(x))]
    copied = [dist[j][0] <= r1[idx[j][0]] for j in range(len(y))]
    return idx, dist, [r1[row[0]] for row in idx], copied


@pytest.mark.parametrize("k", [1, 3, 7])
def test_reference_matches_brute_force_loops(k):
    rng = np.random.default_rng(5 + k)
    x = rng.integers(-2, 3, size=(14, 3)).astype(np.float64)
    y = rng.integers(-2, 3, size=(12, 3)).astype(np.float64) + (rng.random((12, 3)) < 0.3)
    x[6] = x[2]                                      # duplicate rows: ties broken by the smaller index, r1^2 = 0
    x[11] = x[2]
    y[3] = x[2]                                      # y rows on top of x rows: d^2 = 0, copied even where r1^2 = 0
    y[8] = x[5]
    idx, dist, nn_r2, copied = _brute(x, y, k)
    gi, gd = R.nearest(x, y, k)
    assert gi.tolist() == idx and gd.tolist() == dist
    a = R.authenticity(x, y)
    assert a["nn_radius2"].tolist() == nn_r2 and a["copied_rows"].tolist() == copied
    assert a["copied_rows"][3] and a["copied_rows"][8] and a["dist2"][3] == 0 and a["nn_radius2"][3] == 0
    assert a["index"][3] == 2                        # the smallest of the three equal rows
    assert a["copied"] == sum(copied) and a["authenticity"] == 1 - sum(copied) / len(y)
    br = R.bracket(x, y, k, 0.0)                     # no margin: the bracket closes on the exact value
    assert br["copied_lo"] == br["copied_hi"] == a["copied"]
    assert R.valid_knn(gi, gd, br, k).all()


def test_bracket_widens_with_the_margin():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((80, 6))
    y = np.concatenate([x[:20] + 1e-4 * rng.standard_normal((20, 6)), rng.standard_normal((40, 6))])
    exact = R.authenticity(x, y)
    br = R.bracket(x, y, 4, 1e-3)
    assert br["copied_lo"] <= exact["copied"] <= br["copied_hi"]
    idx, d2 = R.nearest(x, y, 4)
    assert R.valid_knn(idx, d2, br, 4).all()
    bad = idx.copy()
    bad[:, 0] = idx[:, 3]
    bad[:, 3] = idx[:, 0]
    assert not R.valid_knn(bad, d2, R.bracket(x, y, 4, 0.0), 4).all()


def test_header_declares_and_capi_binds_nearest():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fad_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fad_nearest\s*\(", text) and "fad_nearest_result_t" in text
    _capi, lib = _lib()
    assert "fad_nearest" in _capi.SIGNATURES and hasattr(lib, "fad_nearest")
    assert [f for f, _ in _capi.FadNearestResult._fields_] == ["authenticity", "n", "m", "k", "copied"]
    assert C.sizeof(_capi.FadNearestResult) == 5 * 8
    assert lib.fad_version() == 2


def test_nearest_argument_errors_come_before_the_device():
    _capi, lib = _lib()
    x = np.random.default_rng(0).standard_normal((16, 8)).astype(np.float16)
    idx = np.zeros(16 * 16, np.int32)
    d2 = np.zeros(16 * 16, np.float32)
    res = _capi.FadNearestResult()

    def call(n=16, m=16, k=5, auth=1, dtype=_capi.FAD_F16, d=8, ld=8, index=idx.ctypes.data, dist2=d2.ctypes.data, out=True):
        return lib.fad_nearest(x.ctypes.data, n, ld, x.ctypes.data, m, ld, d, dtype, 0, k, auth, index, dist2, None,
                               C.byref(res) if out else None, 0, None)
    assert call(k=0) == _capi.FAD_ERR_INVALID
    assert call(k=17) == _capi.FAD_ERR_INVALID
    assert call(index=None) == _capi.FAD_ERR_INVALID
    assert call(dist2=None) == _capi.FAD_ERR_INVALID
    assert call(out=False) == _capi.FAD_ERR_INVALID
    assert call(dtype=_capi.FAD_F64) == _capi.FAD_ERR_INVALID
    assert call(dtype=9) == _capi.FAD_ERR_INVALID
    assert call(d=0) == _capi.FAD_ERR_INVALID
    assert call(ld=4) == _capi.FAD_ERR_INVALID
    assert call(n=4, k=5) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(m=0) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(n=1, k=1, auth=1) == _capi.FAD_ERR_TOO_FEW_ROWS
    assert call(n=1, k=1, auth=0) != _capi.FAD_ERR_TOO_FEW_ROWS          # one baseline row is enough without authenticity
    assert call(n=5, m=1, k=5) != _capi.FAD_ERR_TOO_FEW_ROWS               # n = k and a single evaluation row


def test_nearest_python_errors_raise_before_the_library():
    from fadtk_amd import calc_authenticity, calc_nearest_neighbours, hip
    x = np.zeros((8, 4), np.float32)
    for a, b, k in ((x, x, 0), (x, x, 17), (x[:4], x, 5), (x, x[:0], 1), (x, x[:, :3], 2), (x[0], x, 2), (x[None], x, 2)):
        with pytest.raises(ValueError):
            calc_nearest_neighbours(a, b, k=k)
    for a, b in ((x[:1], x), (x, x[:0]), (x, x[:, :3])):
        with pytest.raises(ValueError):
            calc_authenticity(a, b)
    with pytest.raises(ValueError):
        hip.nearest(x, x, k=0)
    with pytest.raises(ValueError):
        hip.nearest(x[:1], x, k=1, authenticity=True)
    with pytest.raises(ValueError, match="cast"):
        hip.nearest(x.astype(np.float64), x, k=2)


def test_song_rows_aggregation():
    from fadtk_amd.nearest import song_rows
    # baseline files: f0 rows 0..3, f1 rows 4..9, f2 rows 10..10
    base_off = [0, 4, 10, 11]
    # song A (3 rows): nearest rows 5, 7, 1; song B (2 rows): a tie at d^2 = 0.25 between rows 10 and 2 -> the smaller index 2;
    # song C (4 rows): all in f1, two copied
    index = [5, 7, 1, 10, 2, 4, 9, 6, 8]
    dist2 = [0.5, 0.0, 2.0, 0.25, 0.25, 1.0, 1.0, 3.0, 0.75]
    nn_r2 = [0.5, 0.1, 1.0, 0.2, 0.3, 0.5, 1.0, 1.0, 0.75]
    rows = song_rows(index, np.asarray(dist2, np.float32), np.asarray(nn_r2, np.float32), [0, 3, 5, 9], base_off)
    assert rows[0] == {"copied_share": 2 / 3, "min_distance": 0.0, "nearest_file": 1, "match_share": 2 / 3}
    assert rows[1]["nearest_file"] == 0 and rows[1]["match_share"] == 0.5 and rows[1]["min_distance"] == 0.5
    assert rows[1]["copied_share"] == 0.5                 # 0.25 <= 0.3 copied, 0.25 > 0.2 not
    assert rows[2] == {"copied_share": 0.5, "min_distance": float(np.sqrt(np.float64(np.float32(0.75)))), "nearest_file": 1,
                       "match_share": 1.0}


def test_song_rows_sort_order():
    from fadtk_amd.nearest import sort_song_rows
    rows = [("c", 0.0, 3.0), ("a", 1.0, 0.5), ("b", 1.0, 0.1), ("e", 0.5, 2.0), ("d", 0.0, 3.0)]
    assert [r[0] for r in sort_song_rows(rows)] == ["b", "a", "e", "c", "d"]


def test_keep_songs_drops_unreadable_wrong_d_and_empty(caplog):
    from fadtk_amd.nearest import keep_songs
    files = ["ok", "none", "wide", "flat", "empty", "ok2"]
    embds = [np.zeros((3, 4)), None, np.zeros((3, 5)), np.zeros(4), np.zeros((0, 4)), np.zeros((1, 4))]
    with caplog.at_level("ERROR", logger="fadtk_amd"):
        keep = keep_songs(files, embds, 4)
    assert [f for f, _ in keep] == ["ok", "ok2"]
    assert "wide" in caplog.text and "flat" in caplog.text and "empty" in caplog.text


def test_score_individual_leaves_an_existing_csv(tmp_path):
    from fadtk_amd import NearestNeighbours

    class Toy:
        name = "toy"
        sr = 16000
    csv = tmp_path / "out.csv"
    csv.write_text("keep me\n")
    assert NearestNeighbours(Toy()).score_individual(tmp_path / "nowhere", tmp_path / "nowhere", csv) == csv
    assert csv.read_text() == "keep me\n"


def test_nearest_refuses_statistics_baseline(tmp_path):
    from fadtk_amd import NearestNeighbours

    class Toy:
        name = "toy"
        sr = 16000
    npz = tmp_path / "base.npz"
    np.savez(npz, **{"toy.mu": np.zeros(4), "toy.cov": np.eye(4)})
    with pytest.raises(ValueError, match="statistics"):
        NearestNeighbours(Toy()).score(npz, tmp_path)


def test_nearest_cli_help_parses():
    r = subprocess.run([sys.executable, "-m", "fadtk_amd.nearest", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    for flag in ("-k", "-w", "--indiv", "baseline", "eval", "csv"):
        assert flag in r.stdout
