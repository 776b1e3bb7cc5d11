"""MAUVE and the PRD curve end to end on the GPU (fadtk_amd.mauve over fad_kmeans): a set against itself, two separated halves, the
histograms against the returned labels, the restarts, and the command line on two cached directories."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
_here = Path(__file__).resolve().parent
_spec = importlib.util.spec_from_file_location("kmeans_reference", _here / "kmeans_reference.py")
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
_spec = importlib.util.spec_from_file_location("mauve_reference", _here / "mauve_reference.py")
MR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MR)


def _blobs(n, centres, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    return (centres[rng.integers(0, len(centres), n)] + spread * rng.standard_normal((n, centres.shape[1]))).astype(np.float32)


def test_a_set_against_itself():
    from fadtk_amd import calc_mauve
    centres = np.random.default_rng(0).standard_normal((6, 24)) * 4
    x = _blobs(900, centres, 1).astype(np.float16)
    got = calc_mauve(x, x.copy(), clusters=30, iterations=20, redo=2, seed=1)
    np.testing.assert_array_equal(got["labels_x"], got["labels_y"])                   # two copies of a row share their cell
    np.testing.assert_array_equal(got["p_hist"], got["q_hist"])
    assert got["mauve"] == pytest.approx(1.0, abs=1e-9)
    assert got["f_beta"] == pytest.approx(1.0, abs=1e-9) and got["f_beta_inv"] == pytest.approx(1.0, abs=1e-9)
    assert got["clusters"] == 30 and got["n"] == got["m"] == 900


def test_two_separated_halves():
    """Baseline and evaluation rows on two sites 40 apart in every coordinate; the k-means, seeded from rows of both, keeps every cell
    on one side (the reference, run from the winning restart's init, shares none), so the histograms are disjoint."""
    from fadtk_amd import calc_mauve, mauve
    rng = np.random.default_rng(2)
    x = rng.standard_normal((500, 16)).astype(np.float32)
    y = (rng.standard_normal((400, 16)) + 40.0).astype(np.float32)
    got = calc_mauve(x, y, clusters=12, iterations=30, redo=3, seed=0)
    z = np.concatenate([x, y])
    ref = R.lloyd(z, z[mauve.seed_rows(900, 12, 0, got["restart"])], 30)
    px, py = np.bincount(ref["labels"][:500], minlength=12), np.bincount(ref["labels"][500:], minlength=12)
    assert not ((px > 0) & (py > 0)).any()                                            # the reference shares no cell
    assert not ((got["p_hist"] > 0) & (got["q_hist"] > 0)).any()
    assert got["mauve"] < 0.05 and got["f_beta"] == 0.0 and got["f_beta_inv"] == 0.0
    assert got["mauve"] == pytest.approx(MR.metrics((got["p_hist"] * 500).round().tolist(), (got["q_hist"] * 400).round().tolist())["mauve"],
                                         rel=1e-9)


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_histograms_are_the_bincounts_and_redo_takes_the_smallest_inertia(dt):
    from fadtk_amd import calc_kmeans, calc_mauve, hip, mauve
    centres = np.random.default_rng(3).standard_normal((9, 12)) * 3
    x = _blobs(700, centres, 4).astype(np.float16 if dt == "fp16" else np.float32)
    y = _blobs(650, centres[:6], 5, spread=1.3).astype(x.dtype)
    got = calc_mauve(x, y, clusters=None, iterations=25, redo=4, seed=7)
    k = mauve.default_clusters(700, 650)
    assert got["clusters"] == k == 65 and got["labels_x"].shape == (700,) and got["labels_y"].shape == (650,)
    np.testing.assert_array_equal(got["p_hist"], np.bincount(got["labels_x"], minlength=k) / 700.0)
    np.testing.assert_array_equal(got["q_hist"], np.bincount(got["labels_y"], minlength=k) / 650.0)
    want = MR.metrics(np.bincount(got["labels_x"], minlength=k).tolist(), np.bincount(got["labels_y"], minlength=k).tolist())
    assert got["mauve"] == pytest.approx(want["mauve"], rel=1e-9) and got["f_beta"] == pytest.approx(want["f_beta"], rel=1e-9)
    assert 0.0 < got["mauve"] < 1.0
    # every restart on its own, from the documented seeding: the smallest inertia wins, ties to the smaller restart
    z = np.concatenate([x, y]).astype(np.float32)
    runs = [hip.kmeans([x, y], z[mauve.seed_rows(1350, k, 7, r)], iterations=25) for r in range(4)]
    inertias = [r["inertia"] for r in runs]
    best = int(np.argmin(inertias))
    assert got["restart"] == best and got["inertia"] == inertias[best] and len(set(inertias)) > 1
    np.testing.assert_array_equal(np.concatenate([got["labels_x"], got["labels_y"]]), runs[best]["labels"])
    km = calc_kmeans([x, y], k, iterations=25, redo=4, seed=7)
    assert km["restart"] == best and km["inertias"].tolist() == inertias
    one = calc_kmeans([x, y], k, iterations=25, init=z[mauve.seed_rows(1350, k, 7, 1)])
    assert one["restart"] is None and one["inertia"] == inertias[1]
    assert calc_mauve(y, x, clusters=k, iterations=25, redo=1, seed=7)["clusters"] == k


def test_command_line_on_two_cached_directories(tmp_path, capsys):
    from fadtk_amd import mauve
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((5, 128)) * 2
    base, evl = tmp_path / "base", tmp_path / "evl"
    for d, sizes, use in ((base, (40, 41, 42), centres), (evl, (25, 31, 30), centres[:3])):
        (d / "embeddings" / "vggish").mkdir(parents=True)
        for i, rows in enumerate(sizes):
            (d / f"f{i}.wav").write_bytes(b"")                  # the audio itself is never read: every file has its cache
            np.save(d / "embeddings" / "vggish" / f"f{i}.npy", _blobs(rows, use, 10 + i))
    csv, cells = tmp_path / "out" / "mauve.csv", tmp_path / "out" / "cells.csv"
    args = ["vggish", str(base), str(evl), str(csv), "--clusters", "8", "--iterations", "20", "--redo", "2", "--seed", "1", "--cells", str(cells),
            "-w", "2"]
    for _ in range(2):
        mauve.main(args)
    printed = capsys.readouterr().out.split()
    lines = csv.read_text().splitlines()
    assert lines[0] + "\n" == mauve.CSV_HEADER and len(lines) == 3 and lines[1] == lines[2]
    row = dict(zip(mauve.CSV_HEADER.strip().split(","), lines[1].split(",")))
    assert (row["model"], row["n"], row["m"], row["clusters"], row["redo"], row["seed"], row["max_rows"]) == ("vggish", "123", "86", "8", "2", "1", "")
    assert printed[-1] == row["mauve"] and 0.0 < float(row["mauve"]) <= 1.0
    cell_rows = [line.split(",") for line in cells.read_text().splitlines()]
    assert ",".join(cell_rows[0]) + "\n" == mauve.CELLS_CSV_HEADER and len(cell_rows) == 9
    assert sum(int(r[1]) for r in cell_rows[1:]) == 123 and sum(int(r[2]) for r in cell_rows[1:]) == 86
    assert sorted(int(r[0]) for r in cell_rows[1:]) == list(range(8))
    ratios = [float(r[5]) for r in cell_rows[1:] if int(r[1]) + int(r[2])]
    assert ratios == sorted(ratios)                                                   # the cells the evaluation set misses first
    other = tmp_path / "kad.csv"
    other.write_text("model,baseline,eval,kad\n")
    with pytest.raises(SystemExit):
        mauve.main(["vggish", str(base), str(evl), str(other)])
    mauve.main(["vggish", str(base), str(evl), "--max-rows", "50", "--clusters", "4", "--redo", "1"])
    assert 0.0 < float(capsys.readouterr().out.split()[-1]) <= 1.0
