"""Kernel Audio Distance (KAD): the unbiased kernel MMD^2 (Gaussian by default) between two sets of embedding rows.

An addition beyond fadtk's FAD (Chung et al. 2025, "KAD: No More FAD! An Effective and Efficient Evaluation Metric for Audio
Generation"), computed by the same library on the same embedding caches:

    k(a, b) = exp(-|a - b|^2 / (2 sigma^2))
    MMD^2   = mean_{i != j} k(x_i, x_j) + mean_{i != j} k(y_i, y_j) - 2 mean_{i, j} k(x_i, y_j)

``kernel`` / ``--kernel`` picks the KAD toolkit's other kernels with the same bandwidth convention, t = |a - b|^2 / (2 sigma^2):
``"iq"`` k = 1 / (1 + t) and ``"imq"`` k = 1 / sqrt(1 + t), the heavy-tailed choices for sets far apart, where the Gaussian saturates.

x is the baseline, y the evaluation set: all frames of all cached ``.npy`` files of a directory, concatenated (the rows FAD feeds
to ``calc_embd_statistics``).  sigma defaults to the median pairwise distance within the baseline
(``np.median(scipy.spatial.distance.pdist(x))``).  The score is reported as ``scale * MMD^2`` (scale 1 by default) and may be
negative: the estimator is unbiased.

Per song (``--indiv``): KAD between the baseline and each file of the evaluation directory alone, one sigma for all, every song in
one batched GPU call (``fad_kad_individual``); ``path,score`` lines sorted by |score|, like fadtk's per-song FAD.

    python -m fadtk_amd.kad <model> <baseline_dir> <eval_dir> [csv] [--bandwidth S] [--kernel K] [--scale F] [-w N] [--indiv]
    python -m fadtk_amd.kad <model> <baseline_dir> <eval_dir> [csv] --bandwidths S1,S2,... | --bandwidth-factors F1,F2,...

Several evaluation sets against one baseline, with standard errors and paired comparisons (``fad_kad_uncertainty``, a first-order
estimate): ``calc_kernel_audio_distance_uncertainty`` / ``KernelAudioDistance.score_many``, and ``python -m fadtk_amd.kad_compare``.
Several bandwidths in one fused GPU call (``fad_kad_sweep``), a ladder around the median by default, and their mixture kernel:
``calc_kernel_audio_distance_sweep`` / ``KernelAudioDistance.score_sweep``, and ``--bandwidths S1,S2,...`` or
``--bandwidth-factors F1,F2,...`` on the command line (one CSV row per bandwidth).
Whether a set is distinguishable from the baseline at all (a two-sample permutation test, ``fad_kad_permutation_test``):
``calc_kernel_audio_distance_permutation_test`` / ``KernelAudioDistance.permutation_test``, and ``python -m fadtk_amd.kad_permutation``.
"""
from __future__ import annotations

import logging
import math
import time
import traceback
from argparse import ArgumentParser
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Sequence, Union

import numpy as np

from .utils import PathLike, tmap, write

log = logging.getLogger("fadtk_amd")
CSV_HEADER = "model,baseline,eval,kad,bandwidth,scale,time\n"
KAD_KERNELS = ("gaussian", "iq", "imq")
INDIV_BYTES = 4 << 30          # song rows per fad_kad_individual call at most (a larger set is split; sigma comes from the first call)


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape


def _check_kernel(kernel) -> str:
    """the kernel name, or a ValueError -- before any file is read or the native library is loaded"""
    from .hip import kad_kernel_code
    kad_kernel_code(kernel)
    return kernel


def _csv_forms(header: str, kernel: str):
    """-> (the header this kernel's rows go under, the other form, what a row gains): the Gaussian kernel writes header and rows as
    they are; another kernel adds one trailing column ``kernel`` to both."""
    plain, extended = header, header.rstrip("\n") + ",kernel\n"
    return (plain, extended, "") if kernel == "gaussian" else (extended, plain, f",{kernel}")


def check_csv(target: PathLike, header: str, kernel: str = "gaussian") -> None:
    """Refuse (ValueError) a CSV that begins with the header of the other form: no CSV mixes rows with and without the kernel column."""
    mine, other, _ = _csv_forms(header, kernel)
    if Path(target).is_file():
        with open(target) as fh:
            first = fh.readline()
        if first.rstrip("\r\n") == other.rstrip("\n"):
            raise ValueError(f"{target} has the header {other.strip()!r}; a row for kernel {kernel!r} goes under {mine.strip()!r}: "
                             "write it to another file")


def append_csv(target: PathLike, header: str, rows: Sequence[str], kernel: str = "gaussian") -> None:
    """Append ``rows`` (no line ends) to the CSV ``target`` under ``header`` (written when the file is new), in the form of ``kernel``
    (_csv_forms); a file of the other form is refused, untouched (check_csv)."""
    mine, _, tail = _csv_forms(header, kernel)
    check_csv(target, header, kernel)
    target = Path(target)
    target.parent.mkdir(parents=True, exist_ok=True)
    if not target.is_file():
        target.write_text(mine)
    with open(target, "a") as fh:
        for row in rows:
            fh.write(row + tail + "\n")


def calc_kernel_audio_distance(x, y, bandwidth: Optional[float] = None, scale: float = 1.0, device: int = 0, details: bool = False,
                               kernel: str = "gaussian"):
    """scale * MMD^2 between the rows of x (baseline) and y, on the GPU (``fad_kad_k``).  numpy arrays or torch CUDA tensors of
    float16 / bfloat16 / float32.  ``kernel``: "gaussian", "iq" or "imq".  ``details=True`` returns (value, dict of the fad_kad_result
    fields)."""
    _check_kernel(kernel)
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"KAD needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"KAD: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"KAD needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    from . import hip
    res = hip.kad(x, y, bandwidth=bandwidth, device=device, kernel=kernel)
    value = float(scale) * res["mmd2"]
    return (value, res) if details else value


SWEEP_FACTORS = (0.25, 0.5, 1, 2, 4)         # the default ladder: the baseline's median distance halved and doubled twice


@dataclass
class KadSweep:
    """KAD at B bandwidths (``fad_kad_sweep``).  ``values`` [B] = scale * MMD^2 at ``bandwidths`` [B] (the sigma values used, in the
    order asked for); ``mixture`` = the mean of ``values``: scale * MMD^2 under the mixture kernel (1 / B) sum_b k_b, exact by linearity
    of the U-statistic.  ``details``: hip.kad_sweep's arrays."""
    values: np.ndarray
    bandwidths: np.ndarray
    mixture: float
    scale: float
    kernel: str
    details: dict = field(repr=False, default_factory=dict)


def _sweep_request(bandwidths, factors):
    """-> (bandwidths, factors) with exactly one of them set: ``bandwidths`` overrides the default ``factors``; giving both is a
    ValueError, as is a list hip.kad_sweep_bandwidths refuses -- before any file is read or the native library is loaded."""
    from .hip import kad_sweep_bandwidths
    if bandwidths is not None:
        if factors is not None and factors is not SWEEP_FACTORS:
            raise ValueError("KAD sweep: give bandwidths or factors, not both")
        factors = None
    kad_sweep_bandwidths(bandwidths, factors)
    return bandwidths, factors


def calc_kernel_audio_distance_sweep(x, y, bandwidths=None, factors=SWEEP_FACTORS, scale: float = 1.0, device: int = 0,
                                     kernel: str = "gaussian") -> KadSweep:
    """scale * MMD^2 between the rows of x (baseline) and y at several bandwidths, in one GPU call (``fad_kad_sweep``) -> KadSweep.
    ``factors`` (default 0.25, 0.5, 1, 2, 4) are multiples of the median pairwise distance of x; ``bandwidths`` gives the sigma values
    themselves and overrides the default factors (giving both is an error); 1 .. 32 finite values > 0 either way.  Each value carries the
    bits of calc_kernel_audio_distance at that bandwidth.  Shapes, dtypes and ``kernel`` as calc_kernel_audio_distance takes them."""
    _check_kernel(kernel)
    bandwidths, factors = _sweep_request(bandwidths, factors)
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"KAD needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"KAD: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"KAD needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    from . import hip
    res = hip.kad_sweep(x, y, bandwidths=bandwidths, factors=factors, device=device, kernel=kernel)
    scale = float(scale)
    values = scale * res["mmd2"]
    return KadSweep(values=values, bandwidths=res["bandwidth"], mixture=float(np.mean(values)), scale=scale, kernel=kernel, details=res)


def calc_kernel_audio_distance_individual(x, songs: Sequence, bandwidth: Optional[float] = None, scale: float = 1.0, device: int = 0,
                                          details: bool = False, max_bytes: int = INDIV_BYTES, kernel: str = "gaussian"):
    """scale * MMD^2 between the rows of x (baseline) and each song [m_s x D] alone, one sigma for all (``bandwidth=None``: the median
    pairwise distance of x), on the GPU (``fad_kad_individual``) -> float64 array [S], NaN for songs with fewer than 2 frames or a
    non-finite row.  numpy arrays or torch CUDA tensors; mixed dtypes are cast to float32.  Songs whose rows together exceed
    ``max_bytes`` go in several calls, the later ones with the first call's sigma (and every call with ``kernel``: "gaussian", "iq"
    or "imq").  ``details=True`` returns (values, dict of hip.kad_individual's arrays and kxx_mean / bandwidth / n)."""
    _check_kernel(kernel)
    from . import hip
    sx = _shape_of(x)
    if len(sx) != 2 or sx[0] < 2:
        raise ValueError(f"KAD needs a 2-D baseline of at least 2 rows, got shape {sx}")
    shapes = [_shape_of(y) for y in songs]
    for sh in shapes:
        if len(sh) != 2 or (sh[0] > 0 and sh[1] != sx[1]):
            raise ValueError(f"KAD: a song of shape {sh} against a baseline of D = {sx[1]}")
    torch_in = hip.K._is_torch(x)
    if torch_in:
        import torch
        dts = {x.dtype, *(y.dtype for y in songs)}
        if len(dts) > 1:
            x, songs = x.float(), [y.float() for y in songs]
        cat = lambda parts: torch.cat(parts, 0) if parts else x[:0]                  # noqa: E731
    else:
        x = np.asarray(x)
        songs = [np.asarray(y) for y in songs]
        if len({x.dtype, *(y.dtype for y in songs)}) > 1:
            x, songs = x.astype(np.float32), [y.astype(np.float32) for y in songs]
        cat = lambda parts: np.concatenate(parts, 0) if parts else x[:0]             # noqa: E731
    row_bytes = max(1, sx[1] * (x.element_size() if torch_in else x.itemsize))
    S = len(songs)
    res = {k: np.full(S, np.nan) for k in ("mmd2", "kyy_mean", "kxy_mean")}
    res["status"] = np.zeros(S, dtype=np.int32)
    s0, bw = 0, bandwidth
    while True:                                   # batches of whole songs under the byte budget (at least one song each)
        s1, rows = s0, 0
        while s1 < S and (s1 == s0 or rows + shapes[s1][0] * row_bytes <= max_bytes):
            rows += shapes[s1][0] * row_bytes
            s1 += 1
        part = [y.reshape(-1, sx[1]) if shapes[s0 + i][0] == 0 else y for i, y in enumerate(songs[s0:s1])]
        off = np.concatenate([[0], np.cumsum([shapes[s][0] for s in range(s0, s1)], dtype=np.int64)])
        r = hip.kad_individual(x, cat(part), off, bandwidth=bw, device=device, kernel=kernel)
        for k in ("mmd2", "kyy_mean", "kxy_mean", "status"):
            res[k][s0:s1] = r[k]
        res.update(kxx_mean=r["kxx_mean"], bandwidth=r["bandwidth"], n=r["n"])
        bw, s0 = r["bandwidth"], s1
        if s0 >= S:
            break
    values = float(scale) * res["mmd2"]
    return (values, res) if details else values


@dataclass
class KadUncertainty:
    """KAD of S evaluation sets against one baseline with the first-order covariance of the estimates (``fad_kad_uncertainty``).
    ``values`` [S] = scale * MMD^2, ``stderr`` [S] = |scale| * sqrt(cov_ss), ``cov`` [S, S] = scale^2 * cov.  A first-order
    (Hoeffding-projection) estimate: meaningful when the sets differ from the baseline; when a set has the baseline's distribution it
    understates the spread, so it is not a test of "same distribution"."""
    values: np.ndarray
    stderr: np.ndarray
    cov: np.ndarray
    bandwidth: float
    scale: float
    details: dict = field(repr=False, default_factory=dict)

    def compare(self):
        """-> (z, p), both [S, S]: z[s, t] = (values[s] - values[t]) / sqrt(cov_ss + cov_tt - 2 cov_st), the paired difference of
        sets s and t in standard errors, and its two-sided p = erfc(|z| / sqrt 2).  The diagonal (and a pair whose difference has no
        spread) gives z = 0, p = 1."""
        S = len(self.values)
        z, p = np.zeros((S, S)), np.ones((S, S))
        for s in range(S):
            for t in range(S):
                var = self.cov[s, s] + self.cov[t, t] - 2.0 * self.cov[s, t]
                if s != t and var > 0:
                    z[s, t] = (self.values[s] - self.values[t]) / math.sqrt(var)
                    p[s, t] = math.erfc(abs(z[s, t]) / math.sqrt(2.0))
        return z, p


def calc_kernel_audio_distance_uncertainty(x, ys: Sequence, bandwidth: Optional[float] = None, scale: float = 1.0, device: int = 0,
                                           rows: bool = False, kernel: str = "gaussian") -> KadUncertainty:
    """KAD between the rows of x (baseline) and each evaluation set in ``ys`` (1 .. 64 of them), one sigma for all (``bandwidth=None``:
    the median pairwise distance of x), with standard errors and the covariance of the S estimates, in one GPU call
    (``fad_kad_uncertainty``).  ``scale`` multiplies values and stderr by |scale| (the values by scale) and cov by scale^2;
    ``compare()`` of the result gives the paired z and p matrices.  numpy arrays or torch CUDA tensors of float16 / bfloat16 /
    float32; mixed dtypes are cast to float32.  ``rows=True`` keeps the per-row projections in ``details``.  ``kernel``: "gaussian",
    "iq" or "imq".  The estimate is first-order: see KadUncertainty."""
    _check_kernel(kernel)
    from . import hip
    sx = _shape_of(x)
    if len(sx) != 2 or sx[0] < 2:
        raise ValueError(f"KAD needs a 2-D baseline of at least 2 rows, got shape {sx}")
    ys = list(ys)
    for sh in (_shape_of(y) for y in ys):
        if len(sh) != 2 or sh[1] != sx[1]:
            raise ValueError(f"KAD: an evaluation set of shape {sh} against a baseline of D = {sx[1]}")
        if sh[0] < 2:
            raise ValueError(f"KAD needs at least 2 rows per set, got {sh[0]}")
    if hip.K._is_torch(x):
        if len({x.dtype, *(y.dtype for y in ys)}) > 1:
            x, ys = x.float(), [y.float() for y in ys]
    else:
        x, ys = np.asarray(x), [np.asarray(y) for y in ys]
        if len({x.dtype, *(y.dtype for y in ys)}) > 1:
            x, ys = x.astype(np.float32), [y.astype(np.float32) for y in ys]
    res = hip.kad_uncertainty(x, ys, bandwidth=bandwidth, device=device, rows=rows, kernel=kernel)
    scale = float(scale)
    return KadUncertainty(values=scale * res["mmd2"], stderr=abs(scale) * res["stderr"], cov=scale * scale * res["cov"],
                          bandwidth=res["bandwidth"], scale=scale, details=res)


def random_labellings(n: int, m: int, permutations: int, seed: int = 0, device: int = 0, chunk: int = 64):
    """``permutations`` random labellings of N = n + m pooled rows, each with exactly n ones, packed to words [P, ceil(N / 32)] (int32
    holding the uint32 bits) on cuda:``device``: a seeded torch generator there, a stable argsort of uniform keys per labelling, packed
    on the device ``chunk`` labellings at a time.  The same (n, m, permutations, seed) gives the same words on every run."""
    import torch
    from .hip import pack_labels_torch
    N = n + m
    dev = torch.device("cuda", device)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    out = []
    for p0 in range(0, permutations, chunk):
        b = min(chunk, permutations - p0)
        keys = torch.rand((b, N), generator=gen, device=dev)
        idx = torch.argsort(keys, dim=1, stable=True)[:, :n]
        u = torch.zeros((b, N), dtype=torch.bool, device=dev)
        u.scatter_(1, idx, True)
        out.append(pack_labels_torch(u))
    return torch.cat(out)


def calc_kernel_audio_distance_permutation_test(x, y, permutations: int = 1000, seed: int = 0, bandwidth: Optional[float] = None,
                                                scale: float = 1.0, labels=None, return_labels: bool = False, device: int = 0,
                                                kernel: str = "gaussian") -> dict:
    """Is y distinguishable from the baseline x at all?  The two-sample permutation test of KAD (``fad_kad_permutation_test``): the
    rows are pooled, relabelled at random ``permutations`` times with the sizes held at n and m, and MMD^2 is recomputed for every
    labelling in one fused GPU pass; p = (1 + #{null >= observed}) / (P + 1).  ``bandwidth=None``: the median pairwise distance of the
    POOLED rows, which keeps the test exact (KAD's default, the baseline's median, would make it approximate); a given sigma is used as
    is.  Labellings come from a seeded generator on the device unless ``labels`` gives them (bool / uint8 [P, N] or packed words
    [P, ceil(N / 32)]).  numpy arrays or torch CUDA tensors of float16 / bfloat16 / float32.  -> dict: ``kad`` (scale * MMD^2),
    ``mmd2``, ``p_value``, ``null`` [P] (MMD^2 of every random labelling), ``bandwidth``, ``kxx_mean``, ``kyy_mean``, ``kxy_mean``,
    ``n``, ``m``, ``permutations``, ``seed`` (None when labels are given) and, with ``return_labels``, ``labels`` (packed words).
    ``kernel``: "gaussian", "iq" or "imq"."""
    _check_kernel(kernel)
    from . import hip
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"KAD needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"KAD: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"KAD needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    if labels is None:
        if not 1 <= int(permutations) <= hip.KAD_MAX_PERMUTATIONS:
            raise ValueError(f"KAD permutation test takes 1 .. {hip.KAD_MAX_PERMUTATIONS} permutations, got {permutations}")
        labels = random_labellings(sx[0], sy[0], int(permutations), seed=seed, device=device)
    else:
        seed = None
    if hip.K._is_torch(x) and hip.K._is_torch(y):
        if x.dtype != y.dtype:                     # one dtype, as calc_kernel_audio_distance_uncertainty casts mixed sets
            x, y = x.float(), y.float()
    elif not hip.K._is_torch(x) and not hip.K._is_torch(y):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
    res = hip.kad_permutation_test(x, y, labels, bandwidth=bandwidth, device=device, kernel=kernel)
    out = {"kad": float(scale) * res["mmd2"], "mmd2": res["mmd2"], "p_value": res["p_value"], "null": res["null"],
           "bandwidth": res["bandwidth"], "kxx_mean": res["kxx_mean"], "kyy_mean": res["kyy_mean"], "kxy_mean": res["kxy_mean"],
           "n": int(res["n"]), "m": int(res["m"]), "permutations": int(len(res["null"])), "seed": seed}
    if return_labels:
        out["labels"] = labels
    return out


AGGREGATE_FACTORS = (0.125, 0.25, 0.5, 1, 2)   # the default ladder of the aggregated test: down from the pooled median, where a median-sigma test is blind


def _aggregate_request(bandwidths, factors):
    """-> (bandwidths, factors) with exactly one of them set, as _sweep_request: ``bandwidths`` overrides the default ``factors``;
    giving both, or a list hip.kad_permutation_sweep refuses, is a ValueError -- before any file is read or the library is loaded."""
    from .hip import _kad_perm_sweep_bandwidths
    if bandwidths is not None:
        if factors is not None and factors is not AGGREGATE_FACTORS:
            raise ValueError("KAD aggregated test: give bandwidths or factors, not both")
        factors = None
    _kad_perm_sweep_bandwidths(bandwidths, factors)
    return bandwidths, factors


def calc_kernel_audio_distance_aggregated_test(x, y, permutations: int = 1000, seed: int = 0, factors=AGGREGATE_FACTORS, bandwidths=None,
                                               kernel: str = "gaussian", scale: float = 1.0, labels=None, return_labels: bool = False,
                                               device: int = 0) -> dict:
    """Is y distinguishable from the baseline x at any of several scales?  calc_kernel_audio_distance_permutation_test at B bandwidths
    on the same labellings in one fused GPU call (``fad_kad_permutation_sweep``), and one p-value over all of them: the single-step
    min-p correction with uniform weights, exact under exchangeability.  A test at the pooled median alone is blind to differences
    that live at another scale.  ``factors`` (default 1/8, 1/4, 1/2, 1, 2) are multiples of the median pairwise distance of the POOLED
    rows; ``bandwidths`` gives the sigma values themselves and overrides the default factors (giving both is an error); 1 .. 16 finite
    values > 0.  -> dict: ``p_aggregated``, ``p_values`` [B], ``kad`` [B] (scale * MMD^2), ``mmd2`` [B], ``bandwidths`` [B] (the sigma
    values used), ``null`` [B, P], ``kxx_mean``, ``kyy_mean``, ``kxy_mean`` [B], ``n``, ``m``, ``permutations``, ``seed`` (None when
    labels are given) and, with ``return_labels``, ``labels``.  Everything else as calc_kernel_audio_distance_permutation_test."""
    _check_kernel(kernel)
    bandwidths, factors = _aggregate_request(bandwidths, factors)
    from . import hip
    sx, sy = _shape_of(x), _shape_of(y)
    if len(sx) != 2 or len(sy) != 2:
        raise ValueError(f"KAD needs two 2-D row matrices, got shapes {sx} and {sy}")
    if sx[1] != sy[1]:
        raise ValueError(f"KAD: the sets have different dimensions ({sx[1]} and {sy[1]})")
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"KAD needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    if labels is None:
        if not 1 <= int(permutations) <= hip.KAD_MAX_PERMUTATIONS:
            raise ValueError(f"KAD permutation test takes 1 .. {hip.KAD_MAX_PERMUTATIONS} permutations, got {permutations}")
        labels = random_labellings(sx[0], sy[0], int(permutations), seed=seed, device=device)
    else:
        seed = None
    if hip.K._is_torch(x) and hip.K._is_torch(y):
        if x.dtype != y.dtype:
            x, y = x.float(), y.float()
    elif not hip.K._is_torch(x) and not hip.K._is_torch(y):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
    res = hip.kad_permutation_sweep(x, y, labels, bandwidths=bandwidths, factors=factors, device=device, kernel=kernel)
    out = {"p_aggregated": res["p_aggregated"], "p_values": res["p_values"], "kad": float(scale) * res["mmd2"], "mmd2": res["mmd2"],
           "bandwidths": res["bandwidth"], "null": res["null"], "kxx_mean": res["kxx_mean"], "kyy_mean": res["kyy_mean"],
           "kxy_mean": res["kxy_mean"], "n": res["n"], "m": res["m"], "permutations": int(res["null"].shape[1]), "seed": seed}
    if return_labels:
        out["labels"] = labels
    return out


class KernelAudioDistance:
    """KAD between two directories of audio, over the embedding caches FrechetAudioDistance writes and reads."""

    def __init__(self, ml, audio_load_worker: int = 8, load_model: bool = False, device: int = 0):
        from .fad import FrechetAudioDistance
        self.ml = ml
        self.device_index = device
        self.fad = FrechetAudioDistance(ml, audio_load_worker=audio_load_worker, load_model=load_model, device=device)

    def load_rows(self, path: PathLike) -> np.ndarray:
        p = Path(path)
        bundled = Path(__file__).parent / "stats" / (str(path).lower() + ".npz")
        if p.is_file() or (not p.exists() and bundled.exists()):
            raise ValueError(f"KAD needs the embedding rows of a dataset directory; {path} is a statistics file (mu, cov only)")
        if not p.is_dir():
            raise ValueError(f"KAD: {path} is not a directory")
        return self.fad.load_embeddings(p)

    def score(self, baseline: PathLike, eval: PathLike, bandwidth: Optional[float] = None, scale: float = 1.0, details: bool = False,
              kernel: str = "gaussian"):
        _check_kernel(kernel)
        x = self.load_rows(baseline)
        y = self.load_rows(eval)
        if x.dtype == np.float64:             # embedding caches are float32 / float16; a float64 cache is narrowed explicitly
            x = x.astype(np.float32)
        if y.dtype == np.float64:
            y = y.astype(np.float32)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_kernel_audio_distance(x, y, bandwidth=bandwidth, scale=scale, device=self.device_index, details=details,
                                          kernel=kernel)

    def score_sweep(self, baseline: PathLike, eval: PathLike, bandwidths=None, factors=SWEEP_FACTORS, scale: float = 1.0,
                    kernel: str = "gaussian") -> KadSweep:
        """KAD of ``eval`` against ``baseline`` at several bandwidths in one GPU call (calc_kernel_audio_distance_sweep), the rows
        narrowed as ``score`` narrows them."""
        _check_kernel(kernel)
        bandwidths, factors = _sweep_request(bandwidths, factors)
        x = self.load_rows(baseline)
        y = self.load_rows(eval)
        if x.dtype == np.float64:
            x = x.astype(np.float32)
        if y.dtype == np.float64:
            y = y.astype(np.float32)
        if x.dtype != y.dtype:
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_kernel_audio_distance_sweep(x, y, bandwidths=bandwidths, factors=factors, scale=scale, device=self.device_index,
                                                kernel=kernel)

    def score_many(self, baseline: PathLike, eval_dirs: Sequence[PathLike], bandwidth: Optional[float] = None,
                   scale: float = 1.0, kernel: str = "gaussian") -> KadUncertainty:
        """KAD of every directory in ``eval_dirs`` against one baseline, with standard errors and their covariance, in one GPU call
        (calc_kernel_audio_distance_uncertainty); ``compare()`` of the result gives the paired z / p matrices."""
        _check_kernel(kernel)
        x = self.load_rows(baseline)
        ys = [self.load_rows(e) for e in eval_dirs]
        if len({x.dtype, *(y.dtype for y in ys)}) > 1 or x.dtype == np.float64:      # one dtype; float64 caches are narrowed
            x, ys = x.astype(np.float32), [y.astype(np.float32) for y in ys]
        return calc_kernel_audio_distance_uncertainty(x, ys, bandwidth=bandwidth, scale=scale, device=self.device_index, kernel=kernel)

    def permutation_test(self, baseline: PathLike, eval_dir: PathLike, permutations: int = 1000, seed: int = 0,
                         bandwidth: Optional[float] = None, scale: float = 1.0, kernel: str = "gaussian") -> dict:
        """The KAD permutation test of ``eval_dir`` against ``baseline`` (calc_kernel_audio_distance_permutation_test), sigma from the
        pooled rows by default."""
        _check_kernel(kernel)
        x = self.load_rows(baseline)
        y = self.load_rows(eval_dir)
        if x.dtype != y.dtype or x.dtype == np.float64:
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_kernel_audio_distance_permutation_test(x, y, permutations=permutations, seed=seed, bandwidth=bandwidth, scale=scale,
                                                           device=self.device_index, kernel=kernel)

    def aggregated_test(self, baseline: PathLike, eval_dir: PathLike, permutations: int = 1000, seed: int = 0, factors=AGGREGATE_FACTORS,
                        bandwidths=None, scale: float = 1.0, kernel: str = "gaussian") -> dict:
        """The aggregated KAD permutation test of ``eval_dir`` against ``baseline`` over several bandwidths
        (calc_kernel_audio_distance_aggregated_test), factors of the pooled median by default."""
        _check_kernel(kernel)
        bandwidths, factors = _aggregate_request(bandwidths, factors)
        x = self.load_rows(baseline)
        y = self.load_rows(eval_dir)
        if x.dtype != y.dtype or x.dtype == np.float64:
            x, y = x.astype(np.float32), y.astype(np.float32)
        return calc_kernel_audio_distance_aggregated_test(x, y, permutations=permutations, seed=seed, factors=factors, bandwidths=bandwidths,
                                                          kernel=kernel, scale=scale, device=self.device_index)

    def score_individual(self, baseline: PathLike, eval_dir: PathLike, csv_name: Union[Path, str], bandwidth: Optional[float] = None,
                         scale: float = 1.0, kernel: str = "gaussian") -> Path:
        """Per-file KAD against the baseline, written as ``path,score`` lines sorted by |score| (FrechetAudioDistance.score_individual's
        format).  All songs go in one batched GPU call with one sigma; files whose embedding is missing, unreadable, of another D or
        shorter than two frames are logged and dropped.  A ``str`` name goes under data/kad-individual/<model>/; an existing CSV is
        left as it is."""
        _check_kernel(kernel)
        csv = Path(csv_name)
        if isinstance(csv_name, str):
            csv = Path("data") / "kad-individual" / self.ml.name / csv_name
        if csv.exists():
            log.info(f"CSV file {csv} already exists, exiting...")
            return csv
        x = self.load_rows(baseline)
        files = list(Path(eval_dir).glob("*.*"))

        def _read(f):
            try:
                return self.fad.read_embedding_file(f)
            except Exception as e:      # noqa: BLE001
                traceback.print_exc()
                log.error(f"An error occurred calculating individual KAD using model {self.ml.name} on file {f}")
                log.error(e)
                return None

        embds = tmap(_read, files, desc="Loading embeddings", max_workers=self.fad.audio_load_worker)
        keep = []
        for f, e in zip(files, embds):
            if e is None:
                continue
            if e.ndim != 2 or e.shape[1] != x.shape[1]:
                log.error(f"Embedding of {f} has shape {e.shape}; expected [*, {x.shape[1]}]")
            elif e.shape[0] < 2:
                log.error(f"Individual KAD of {f} dropped: {e.shape[0]} frame(s), KAD needs at least 2")
            else:
                keep.append((f, e))
        dts = {x.dtype, *(e.dtype for _, e in keep)}
        if len(dts) > 1 or np.float64 in dts:      # one dtype for the call; float64 caches are narrowed, as score() does
            x, keep = x.astype(np.float32), [(f, e.astype(np.float32)) for f, e in keep]
        pairs = []
        if keep:
            values, res = calc_kernel_audio_distance_individual(x, [e for _, e in keep], bandwidth=bandwidth, scale=scale,
                                                                device=self.device_index, details=True, kernel=kernel)
            for (f, _), v, st in zip(keep, values, res["status"]):
                if st == 0:
                    pairs.append((f, np.float64(v)))
                else:
                    log.error(f"An error occurred calculating individual KAD using model {self.ml.name} on file {f} (status {st}: "
                              f"{'fewer than two frames' if st == -6 else 'non-finite rows'})")
        pairs = sorted(pairs, key=lambda p: np.abs(p[1]))
        write(csv, "\n".join(",".join(str(v).replace(",", "_") for v in row) for row in pairs))
        return csv


def _float_list(text: str):
    """argparse type of --bandwidths / --bandwidth-factors: comma-separated numbers"""
    return [float(t) for t in text.split(",")]


def main(argv=None):
    from .cli import _registry, _setup_logging
    _setup_logging()
    models = _registry()
    p = ArgumentParser(prog="python -m fadtk_amd.kad", description="Kernel Audio Distance (unbiased kernel MMD^2, Gaussian by default) "
                       "between two directories of audio, on one GPU")
    p.add_argument("model", type=str, choices=list(models), help="embedding model")
    p.add_argument("baseline", type=str, help="baseline dataset directory")
    p.add_argument("eval", type=str, help="directory to evaluate")
    p.add_argument("csv", type=str, nargs="?", help="append the result to this CSV; with --indiv: where per-song scores go "
                                                    "(default kad-individual-results.csv)")
    bw = p.add_mutually_exclusive_group()
    bw.add_argument("--bandwidth", type=float, default=None, help="kernel sigma (default: median pairwise distance of the baseline)")
    bw.add_argument("--bandwidths", type=_float_list, default=None, metavar="S1,S2,...",
                    help="several kernel sigmas in one fused pass: one CSV row and one printed value per bandwidth (1 .. 32 values > 0)")
    bw.add_argument("--bandwidth-factors", type=_float_list, default=None, metavar="F1,F2,...",
                    help="as --bandwidths, each a multiple of the median pairwise distance of the baseline (1 is the default bandwidth)")
    p.add_argument("--kernel", type=str, choices=list(KAD_KERNELS), default="gaussian",
                   help="gaussian exp(-t), iq 1 / (1 + t) or imq 1 / sqrt(1 + t), t = d^2 / (2 sigma^2) (default gaussian); a CSV written "
                        "for iq or imq has one more column, kernel")
    p.add_argument("--scale", type=float, default=1.0, help="factor applied to the reported MMD^2 (default 1)")
    p.add_argument("-w", "--workers", type=int, default=8, help="number of workers")
    p.add_argument("--indiv", action="store_true", help="one score per song of the eval directory")
    a = p.parse_args(argv)
    sweep = a.bandwidths is not None or a.bandwidth_factors is not None
    if sweep and a.indiv:
        p.error("--bandwidths / --bandwidth-factors cannot be combined with --indiv")
    if sweep:
        try:
            _sweep_request(a.bandwidths, a.bandwidth_factors)
        except ValueError as e:
            p.error(str(e))
    model = models[a.model]
    if a.csv and not a.indiv:
        check_csv(a.csv, CSV_HEADER, a.kernel)             # before any work: a CSV of the other form is refused

    from .fad_batch import cache_embedding_files
    for dataset in (a.baseline, a.eval):
        if Path(dataset).is_dir():
            cache_embedding_files(dataset, model, workers=a.workers)
    kad = KernelAudioDistance(model, audio_load_worker=a.workers, load_model=False)
    if a.indiv:
        assert Path(a.eval).is_dir(), "Individual KAD requires a directory as the evaluation dataset"
        out = Path(a.csv or "kad-individual-results.csv")
        kad.score_individual(a.baseline, a.eval, out, bandwidth=a.bandwidth, scale=a.scale, kernel=a.kernel)
        log.info(f"Individual KAD scores saved to {out}")
        return
    if sweep:
        r = kad.score_sweep(a.baseline, a.eval, bandwidths=a.bandwidths, factors=a.bandwidth_factors, scale=a.scale, kernel=a.kernel)
        values, sigmas = [float(v) for v in r.values], [float(s) for s in r.bandwidths]
        if a.csv:                                          # one row per bandwidth; no mixture row: the header has one bandwidth column
            now = time.time()
            append_csv(a.csv, CSV_HEADER, [f"{model.name},{a.baseline},{a.eval},{v!r},{s!r},{a.scale!r},{now}" for v, s in zip(values, sigmas)],
                       a.kernel)
            log.info(f"{len(values)} KAD scores appended to {a.csv}")
        for v, s in zip(values, sigmas):
            log.info(f"The KAD {model.name} score between {a.baseline} and {a.eval} is: {v} (bandwidth {s})")
        log.info(f"The KAD {model.name} score between {a.baseline} and {a.eval} under the mixture of these {len(values)} kernels is: {r.mixture}")
        for v in values:
            print(v)
        return
    value, res = kad.score(a.baseline, a.eval, bandwidth=a.bandwidth, scale=a.scale, details=True, kernel=a.kernel)
    if a.csv:
        append_csv(a.csv, CSV_HEADER, [f"{model.name},{a.baseline},{a.eval},{value!r},{res['bandwidth']!r},{a.scale!r},{time.time()}"],
                   a.kernel)
        log.info(f"KAD score appended to {a.csv}")
    log.info(f"The KAD {model.name} score between {a.baseline} and {a.eval} is: {value} (bandwidth {res['bandwidth']})")
    print(value)


if __name__ == "__main__":
    main()
