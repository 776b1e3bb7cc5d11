"""MAUVE and the PRD curve from two cell histograms (fadtk_amd.mauve.histogram_metrics), host side (no GPU): against the independent
restatement of tests/mauve_reference.py, the closed forms of equal and of disjoint histograms, the symmetry in the two arguments to the
bit, histograms with empty cells, and the CSV files."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("mauve_reference", Path(__file__).resolve().parent / "mauve_reference.py")
MR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MR)


def _hists(k, seed, empty=0):
    rng = np.random.default_rng(seed)
    p, q = rng.integers(1, 50, k), rng.integers(1, 50, k)
    if empty:
        p[rng.choice(k, empty, replace=False)] = 0
        q[rng.choice(k, empty, replace=False)] = 0
    return p, q


@pytest.mark.parametrize("k,seed,empty", [(2, 0, 0), (10, 1, 0), (37, 2, 9), (500, 3, 120)])
def test_against_the_independent_restatement(k, seed, empty):
    from fadtk_amd import mauve
    p, q = _hists(k, seed, empty)
    got, want = mauve.histogram_metrics(p, q), MR.metrics(p.tolist(), q.tolist())
    for key in ("mauve", "f_beta", "f_beta_inv"):
        assert got[key] == pytest.approx(want[key], rel=1e-10, abs=1e-12), key
    np.testing.assert_allclose(got["divergence_curve"], want["divergence_curve"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got["prd_precision"], want["prd_precision"], rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(got["prd_recall"], want["prd_recall"], rtol=1e-10, atol=1e-15)
    assert got["divergence_curve"].shape == (27, 2) and got["prd_precision"].shape == (1001,)
    assert got["p_hist"].sum() == pytest.approx(1.0) and got["q_hist"].sum() == pytest.approx(1.0)
    assert 0 < got["mauve"] <= 1 and 0 <= got["f_beta"] <= 1 and 0 <= got["f_beta_inv"] <= 1
    other = mauve.histogram_metrics(p, q, scale=2.0, points=9)
    assert other["divergence_curve"].shape == (11, 2)
    assert other["mauve"] == pytest.approx(MR.metrics(p.tolist(), q.tolist(), 2.0, 9)["mauve"], rel=1e-10)


def test_equal_histograms_give_one():
    from fadtk_amd import mauve
    for counts in ([5, 1, 0, 7, 3], [1], list(range(1, 200))):
        got = mauve.histogram_metrics(counts, counts)
        assert got["mauve"] == pytest.approx(1.0, abs=1e-9)
        assert got["f_beta"] == pytest.approx(1.0, abs=1e-9) and got["f_beta_inv"] == pytest.approx(1.0, abs=1e-9)
    got = mauve.histogram_metrics([2, 4, 6], [1, 2, 3])                 # the same frequencies from other counts
    assert got["mauve"] == pytest.approx(1.0, abs=1e-9)


def test_disjoint_supports_give_the_closed_form():
    from fadtk_amd import mauve
    got = mauve.histogram_metrics([3, 1, 0, 0, 0], [0, 0, 2, 2, 5], scale=5.0, points=25)
    lam = np.linspace(1e-6, 1 - 1e-6, 25)
    # r = lam p + (1 - lam) q: KL(q || r) = -ln(1 - lam), KL(p || r) = -ln(lam)
    np.testing.assert_allclose(got["divergence_curve"][:25, 0], (1 - lam) ** 5, rtol=1e-9)
    np.testing.assert_allclose(got["divergence_curve"][:25, 1], lam ** 5, rtol=1e-9)
    assert got["divergence_curve"][25:].tolist() == [[0.0, 1.0], [1.0, 0.0]]
    assert got["f_beta"] == 0.0 and got["f_beta_inv"] == 0.0 and (got["prd_precision"] == 0).all() and (got["prd_recall"] == 0).all()
    assert got["mauve"] == pytest.approx(MR.metrics([3, 1, 0, 0, 0], [0, 0, 2, 2, 5])["mauve"], rel=1e-10) and got["mauve"] < 0.01


@pytest.mark.parametrize("k,seed,empty", [(3, 5, 1), (40, 6, 0), (300, 7, 80)])
def test_swapped_arguments_give_the_same_mauve_to_the_bit(k, seed, empty):
    from fadtk_amd import mauve
    p, q = _hists(k, seed, empty)
    a, b = mauve.histogram_metrics(p, q), mauve.histogram_metrics(q, p)
    assert a["mauve"] == b["mauve"]
    np.testing.assert_array_equal(a["divergence_curve"][:25], b["divergence_curve"][:25][::-1, ::-1])
    # the PRD curve mirrors: precision of (p, q) at lam is recall of (q, p) at 1 / lam
    assert a["f_beta"] == pytest.approx(b["f_beta_inv"], rel=1e-6) and a["f_beta_inv"] == pytest.approx(b["f_beta"], rel=1e-6)


def test_histograms_with_empty_cells():
    from fadtk_amd import mauve
    got = mauve.histogram_metrics([4, 0, 0, 6], [2, 3, 0, 5])           # a cell only q reaches, a cell nobody reaches
    want = MR.metrics([4, 0, 0, 6], [2, 3, 0, 5])
    assert np.isfinite(got["mauve"]) and got["mauve"] == pytest.approx(want["mauve"], rel=1e-10)
    assert got["f_beta"] == pytest.approx(want["f_beta"], rel=1e-10) and got["f_beta_inv"] == pytest.approx(want["f_beta_inv"], rel=1e-10)
    assert np.isfinite(got["divergence_curve"]).all()
    dropped = mauve.histogram_metrics([4, 6], [2, 5])                   # ... and the empty cell does not matter
    assert mauve.histogram_metrics([4, 0, 6], [2, 0, 5])["mauve"] == dropped["mauve"]
    for bad in (([1, 2], [1, 2, 3]), ([0, 0], [1, 1]), ([[1, 2]], [[1, 2]])):
        with pytest.raises(ValueError, match="histograms"):
            mauve.histogram_metrics(*bad)


def test_csv_files(tmp_path):
    from fadtk_amd import mauve
    res = mauve.histogram_metrics([3, 0, 4, 0, 1], [1, 2, 0, 0, 5])
    res.update(clusters=5, inertia=12.5, iterations=7, converged=1, empty_clusters=1, n=8, m=8,
               labels_x=np.array([0, 0, 0, 2, 2, 2, 2, 4]), labels_y=np.array([0, 1, 1, 4, 4, 4, 4, 4]))
    target = tmp_path / "sub" / "mauve.csv"
    mauve.append_csv(target, mauve.csv_row("vggish", "a", "b", res, redo=5, seed=0, scale=5.0))
    mauve.append_csv(target, mauve.csv_row("vggish", "a", "c", res, redo=1, seed=2, scale=2.0, max_rows=100))
    lines = target.read_text().splitlines()
    assert lines[0] + "\n" == mauve.CSV_HEADER and len(lines) == 3
    assert lines[1].startswith(f"vggish,a,b,8,8,{res['mauve']!r},") and lines[1].endswith(",5,12.5,7,1,1,5,0,5.0,")
    assert lines[2].endswith(",1,2,2.0,100") and all(len(line.split(",")) == len(mauve.CSV_HEADER.split(",")) for line in lines)
    other = tmp_path / "kad.csv"
    other.write_text("model,baseline,eval,kad\n")
    with pytest.raises(ValueError, match="another file"):
        mauve.append_csv(other, "x")
    with pytest.raises(ValueError, match="another file"):
        mauve.write_cells_csv(other, res)
    with pytest.raises(ValueError, match="another file"):
        mauve.write_cells_csv(target, res)                               # the run CSV is not a cells CSV
    assert other.read_text() == "model,baseline,eval,kad\n"
    cells = tmp_path / "cells.csv"
    assert mauve.write_cells_csv(cells, res) == 5 and mauve.write_cells_csv(cells, res) == 5        # one with this header is replaced
    rows = [line.split(",") for line in cells.read_text().splitlines()]
    assert ",".join(rows[0]) + "\n" == mauve.CELLS_CSV_HEADER and len(rows) == 6
    # the cell the evaluation set misses first, then by ln(q / p) ascending, the cell only it reaches after them, the empty cell last
    assert [r[0] for r in rows[1:]] == ["2", "0", "4", "1", "3"]
    assert rows[1][1:3] == ["4", "0"] and rows[1][5] == "-inf" and rows[4][5] == "inf" and rows[5][5] == "nan"
    assert float(rows[2][5]) == pytest.approx(np.log((1 / 8) / (3 / 8)))


def test_command_line_refuses_another_header_before_any_work(tmp_path, monkeypatch):
    from fadtk_amd import fad_batch, mauve

    def no_work(*a, **k):
        raise AssertionError("work was started")
    monkeypatch.setattr(fad_batch, "cache_embedding_files", no_work)
    other = tmp_path / "kad.csv"
    other.write_text("model,baseline,eval,kad\n")
    for args in ([str(other)], ["--cells", str(other)], [str(tmp_path / "new.csv"), "--cells", str(other)]):
        with pytest.raises(SystemExit) as e:
            mauve.main(["vggish", str(tmp_path), str(tmp_path), *args])
        assert e.value.code == 2
    for args in (["--clusters", "0"], ["--redo", "0"], ["--iterations", "-1"], ["--scale", "0"], ["--max-rows", "0"], ["--seed", "-1"]):
        with pytest.raises(SystemExit) as e:
            mauve.main(["vggish", str(tmp_path), str(tmp_path), *args])
        assert e.value.code == 2
    assert other.read_text() == "model,baseline,eval,kad\n"
