"""Nearest baseline rows and authenticity: which evaluation songs lie on top of which baseline (training) files.

An addition beyond fadtk, computed by the same library on the same embedding caches as KAD.  For every evaluation row y_j the k
nearest baseline rows x_i, in ascending order of (d^2, i) on the float32 squared distances (``fad_nearest``, include/fad_hip.h).
Authenticity (Alaa et al. 2022, "How Faithful is your Synthetic Data?"): with nn(j) y_j's nearest baseline row and r1(i) the
distance from x_i to its nearest OTHER baseline row, y_j is copied when d(y_j, x_nn(j)) <= r1(nn(j)) (non-strict: an exact copy always
counts), and

    authenticity = 1 - copied / m

The n x m distance matrix is never stored: one cross pass (and one radius pass for authenticity) on the matrix cores.

Per song (``--indiv``): every frame of every evaluation file in one call, and per file ``path,copied_share,min_distance,
nearest_baseline,match_share``: the share of its frames that are copied, its smallest frame distance to the baseline, the baseline
file of that closest frame pair, and the share of its frames whose nearest baseline row lies in that file.  Rows are sorted by
copied_share (descending), then min_distance.

    python -m fadtk_amd.nearest <model> <baseline_dir> <eval_dir> [csv] [-k K] [-w N] [--indiv]
"""
from __future__ import annotations

import logging
import time
import traceback
from argparse import ArgumentParser
from pathlib import Path
from typing import List, Sequence, Union

import numpy as np

from .utils import PathLike, tmap, write

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,k,authenticity,copied,m,median_distance,median_kth_distance,time\n"
INDIV_HEADER = "path,copied_share,min_distance,nearest_baseline,match_share"
MAX_K = 16


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def _check(x, y, k: int, authenticity: bool):
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"nearest needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"nearest: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"nearest: k must be in 1 .. {MAX_K}, got {k}")
    need = max(int(k), 2) if authenticity else int(k)
    if sx[0] < need or sy[0] < 1:
        raise ValueError(f"nearest with k = {k}{' and authenticity' if authenticity else ''} needs at least {need} baseline rows and "
                         f"1 evaluation row, got {sx[0]} and {sy[0]}")


def calc_nearest_neighbours(x, y, k: int = 1, device: int = 0):
    """The k nearest rows of the baseline x to every row of y, on the GPU (``fad_nearest``) -> (distances [m, k] float64, the square
    roots of the float32 squared distances; indices [m, k] int64), ascending in (distance, index).  numpy arrays or torch CUDA tensors
    of float16 / bfloat16 / float32."""
    _check(x, y, k, False)
    from . import hip
    res = hip.nearest(x, y, k=int(k), authenticity=False, device=device)
    return np.sqrt(res["dist2"].astype(np.float64)), res["index"].astype(np.int64)


def calc_authenticity(x, y, device: int = 0, details: bool = False) -> dict:
    """Authenticity of the rows of y against the baseline x (``fad_nearest`` with k = 1) -> dict of ``authenticity``, ``copied`` (rows
    of y within the nearest-neighbour radius of their nearest baseline row), ``n`` and ``m``.  ``details=True`` adds per-row arrays:
    ``index`` [m] (int64, the nearest baseline row), ``distance`` [m] and ``nn_radius`` [m] (float64 square roots of the float32
    squared values compared) and ``copied_rows`` [m] (bool)."""
    _check(x, y, 1, True)
    from . import hip
    res = hip.nearest(x, y, k=1, authenticity=True, device=device)
    out = {"authenticity": float(res["authenticity"]), "copied": int(res["copied"]), "n": int(res["n"]), "m": int(res["m"])}
    if details:
        out.update(index=res["index"][:, 0].astype(np.int64), distance=np.sqrt(res["dist2"][:, 0].astype(np.float64)),
                   nn_radius=np.sqrt(res["nn_radius2"].astype(np.float64)), copied_rows=res["dist2"][:, 0] <= res["nn_radius2"])
    return out


def song_rows(index, dist2, nn_radius2, song_offsets: Sequence[int], base_offsets: Sequence[int]) -> List[dict]:
    """Per-song aggregation of one k = 1 call over the concatenated songs.  Song s is rows [song_offsets[s], song_offsets[s + 1]) of
    the evaluation rows, baseline file f rows [base_offsets[f], base_offsets[f + 1]) of the baseline.  ``index``, ``dist2`` and
    ``nn_radius2`` are per evaluation row (float32 squared values as fad_nearest returns them) -> per song a dict of ``copied_share``,
    ``min_distance`` (float64 square root of the smallest float32 d^2), ``nearest_file`` (the file of the row with the smallest
    (d^2, index): the closest frame pair, ties to the smaller baseline row) and ``match_share`` (share of the song's rows whose nearest
    row lies in that file)."""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    dist2 = np.asarray(dist2, dtype=np.float32).reshape(-1)
    nn_radius2 = np.asarray(nn_radius2, dtype=np.float32).reshape(-1)
    so = np.asarray(song_offsets, dtype=np.int64)
    file_of = np.searchsorted(np.asarray(base_offsets, dtype=np.int64), index, side="right") - 1
    copied = dist2 <= nn_radius2
    out = []
    for s in range(so.shape[0] - 1):
        a, b = int(so[s]), int(so[s + 1])
        best = a + int(np.lexsort((index[a:b], dist2[a:b]))[0])            # smallest (d^2, index)
        f = int(file_of[best])
        out.append({"copied_share": float(copied[a:b].mean()), "min_distance": float(np.sqrt(np.float64(dist2[best]))),
                    "nearest_file": f, "match_share": float((file_of[a:b] == f).mean())})
    return out


def sort_song_rows(rows: Sequence[tuple]) -> list:
    """(path, copied_share, min_distance, ...) rows -> sorted by copied_share descending, then min_distance, then path."""
    return sorted(rows, key=lambda r: (-r[1], r[2], str(r[0])))


class NearestNeighbours:
    """Nearest baseline files and authenticity between two directories of audio, over the embedding caches FrechetAudioDistance
    writes and reads.  The baseline is loaded per file, so that every baseline row maps back to its file."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0):
        from .fad import FrechetAudioDistance
        self.ml = ml
        self.device_index = device
        self.fad = FrechetAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def _dir(self, path: PathLike) -> Path:
        p = Path(path)
        bundled = Path(__file__).parent / "stats" / (str(path).lower() + ".npz")
        if p.is_file() or (not p.exists() and bundled.exists()):
            raise ValueError(f"nearest needs the embedding rows of a dataset directory; {path} is a statistics file (mu, cov only)")
        if not p.is_dir():
            raise ValueError(f"nearest: {path} is not a directory")
        return p

    def load_baseline(self, baseline: PathLike):
        """-> (rows [n x D], files, offsets [F + 1]): the baseline's rows file by file; files with no frames are left out."""
        files = sorted(self._dir(baseline).glob("*.*"))
        embds, files = self.fad._load_embeddings(files, concat=False)
        keep = [(f, e) for f, e in zip(files, embds) if e.ndim == 2 and e.shape[0] > 0]
        for f, e in zip(files, embds):
            if not (e.ndim == 2 and e.shape[0] > 0):
                log.error(f"Baseline embedding of {f} has shape {e.shape}: left out")
        if not keep:
            raise ValueError(f"nearest: no baseline rows in {baseline}")
        offsets = np.concatenate([[0], np.cumsum([e.shape[0] for _, e in keep])]).astype(np.int64)
        return np.concatenate([e for _, e in keep], axis=0), [f for f, _ in keep], offsets

    def score(self, baseline: PathLike, eval: PathLike, k: int = 1) -> dict:
        """Set-level results: ``authenticity``, ``copied``, ``n``, ``m``, ``k``, ``median_distance`` (median over the evaluation rows of
        the nearest baseline distance) and ``median_kth_distance`` (of the k-th nearest)."""
        x = self.fad.load_embeddings(self._dir(baseline))
        y = self.fad.load_embeddings(self._dir(eval))
        x, (y,) = _one_dtype(x, [y])
        _check(x, y, k, True)
        from . import hip
        res = hip.nearest(x, y, k=int(k), authenticity=True, device=self.device_index)
        dist = np.sqrt(res["dist2"].astype(np.float64))
        return {"authenticity": float(res["authenticity"]), "copied": int(res["copied"]), "n": int(res["n"]), "m": int(res["m"]),
                "k": int(k), "median_distance": float(np.median(dist[:, 0])), "median_kth_distance": float(np.median(dist[:, -1]))}

    def score_individual(self, baseline: PathLike, eval_dir: PathLike, csv_name: Union[Path, str]) -> Path:
        """Per eval file ``path,copied_share,min_distance,nearest_baseline,match_share`` lines under a header, every song in one
        ``fad_nearest`` call (k = 1), sorted by copied_share descending, then min_distance.  Files whose embedding is missing,
        unreadable, of another D or empty are logged and dropped.  A ``str`` name goes under data/nearest-individual/<model>/; an
        existing CSV is left as it is."""
        csv = Path(csv_name)
        if isinstance(csv_name, str):
            csv = Path("data") / "nearest-individual" / self.ml.name / csv_name
        if csv.exists():
            log.info(f"CSV file {csv} already exists, exiting...")
            return csv
        x, base_files, base_off = self.load_baseline(baseline)
        files = list(Path(eval_dir).glob("*.*"))

        def _read(f):
            try:
                return self.fad.read_embedding_file(f)
            except Exception as e:      # noqa: BLE001
                traceback.print_exc()
                log.error(f"An error occurred finding the nearest baseline rows using model {self.ml.name} on file {f}")
                log.error(e)
                return None

        embds = tmap(_read, files, desc="Loading embeddings", max_workers=self.fad.audio_load_worker)
        keep = keep_songs(files, embds, x.shape[1])
        rows = []
        if keep:
            x, ys = _one_dtype(x, [e for _, e in keep])
            _check(x, ys[0], 1, True)
            from . import hip
            off = np.concatenate([[0], np.cumsum([e.shape[0] for e in ys])]).astype(np.int64)
            res = hip.nearest(x, np.concatenate(ys, axis=0), k=1, authenticity=True, device=self.device_index)
            for (f, _), r in zip(keep, song_rows(res["index"][:, 0], res["dist2"][:, 0], res["nn_radius2"], off, base_off)):
                rows.append((f, r["copied_share"], r["min_distance"], base_files[r["nearest_file"]], r["match_share"]))
        lines = [INDIV_HEADER] + [",".join(str(v).replace(",", "_") for v in row) for row in sort_song_rows(rows)]
        write(csv, "\n".join(lines) + "\n")
        return csv


def keep_songs(files, embds, d: int) -> list:
    """(file, embedding) pairs of the songs that can be scored: read, 2-D with D columns and at least one frame; the others logged."""
    keep = []
    for f, e in zip(files, embds):
        if e is None:
            continue
        if e.ndim != 2 or e.shape[1] != d:
            log.error(f"Embedding of {f} has shape {e.shape}; expected [*, {d}]")
        elif e.shape[0] < 1:
            log.error(f"Nearest baseline rows of {f} dropped: the embedding has no frames")
        else:
            keep.append((f, e))
    return keep


def _one_dtype(x, ys):
    """One dtype for the call: float64 caches are narrowed to float32, mixed dtypes go to float32."""
    dts = {x.dtype, *(e.dtype for e in ys)}
    if len(dts) > 1 or np.float64 in dts:
        return x.astype(np.float32), [e.astype(np.float32) for e in ys]
    return x, list(ys)


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.nearest", description="Nearest baseline rows and authenticity (did the evaluated "
                       "set copy the baseline, and which songs?) between two directories of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline (training) dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the set-level result to this CSV; with --indiv: where per-song rows go "
                                                    "(default nearest-individual-results.csv)")
    p.add_argument("-k", type=int, default=1, help="nearest baseline rows per evaluation row, 1 .. 16 (default 1; --indiv uses 1)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    p.add_argument("--indiv", action="store_true", help="one row per song of the eval directory: copied share, nearest baseline file")
    a = p.parse_args(argv)
    model = models[a.model]

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    nn = NearestNeighbours(model, audio_load_worker=a.workers, load_model=False)
    if a.indiv:
        assert Path(a.eval).is_dir(), "Individual nearest rows require a directory as the evaluation dataset"
        out = Path(a.csv or "nearest-individual-results.csv")
        nn.score_individual(a.baseline, a.eval, out)
        log.info(f"Per-song nearest baseline files saved to {out}")
        return
    res = nn.score(a.baseline, a.eval, k=a.k)
    if a.csv:
        target = Path(a.csv)
        target.parent.mkdir(parents=True, exist_ok=True)
        if not target.is_file():
            target.write_text(CSV_HEADER)
        with open(target, "a") as fh:
            fh.write(f"{model.name},{a.baseline},{a.eval},{a.k},{res['authenticity']!r},{res['copied']},{res['m']},"
                     f"{res['median_distance']!r},{res['median_kth_distance']!r},{time.time()}\n")
        log.info(f"Nearest-neighbour result appended to {a.csv}")
    log.info(f"Authenticity {model.name} of {a.eval} against {a.baseline}: {res['authenticity']} ({res['copied']} of {res['m']} rows "
             f"copied), median nearest distance {res['median_distance']}")
    for key in ("authenticity", "copied", "median_distance", "median_kth_distance"):
        print(f"{key} {res[key]!r}")


if __name__ == "__main__":
    main()
