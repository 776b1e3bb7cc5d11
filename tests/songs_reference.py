"""float64 numpy reference of the per-song FAD against one baseline for the per-song tests (test plumbing, not product).

For one song's stored frames (float16 / float32 / float64 numpy rows, or bfloat16 torch rows), upcast to float64:
  mean for the mean term -- mean_mode 0: the exact float64 mean; mean_mode 1: np.mean in the frames' own dtype (float16 / float32), the
      float32 np.mean of the widened frames rounded to bfloat16 (round to nearest even) for bfloat16, the float64 mean for float64;
  Sigma_s = np.cov(rows, rowvar=False);
  tr sqrt(Sigma_b Sigma_s) in symmetric form: B = sqrt(Sigma_b) from eigh of (Sigma_b + Sigma_b^T) / 2, then sum sqrt(max(lambda, 0)) over
      eigvalsh(B Sigma_s B) -- one eigvalsh per song, B once per baseline;
  score = ||mu_b - mean||^2 + tr Sigma_b + tr Sigma_s - 2 tr sqrt.
A song with fewer than two frames or any non-finite frame, or a baseline covariance with a non-finite entry, gives None (the reference's
eig raises and the song is dropped)."""
import numpy as np


def _is_bf16(rows):
    return type(rows).__module__.split(".")[0] == "torch" and str(rows.dtype) == "torch.bfloat16"


def as_f64(rows):
    """The stored frames widened to float64 (numpy)."""
    if type(rows).__module__.split(".")[0] == "torch":
        import torch
        return rows.detach().cpu().to(torch.float64).numpy()
    return np.asarray(rows, dtype=np.float64)


def song_mean(rows, mean_mode):
    x = as_f64(rows)
    if mean_mode == 0:
        return x.mean(axis=0)
    if _is_bf16(rows):
        import torch
        m32 = np.mean(x.astype(np.float32), axis=0)
        return torch.from_numpy(m32).to(torch.bfloat16).to(torch.float64).numpy()
    a = np.asarray(rows)
    if a.dtype == np.float64:
        return x.mean(axis=0)
    return np.mean(a, axis=0).astype(np.float64)


class Baseline:
    def __init__(self, mu_b, cov_b):
        self.mu = np.asarray(mu_b, dtype=np.float64)
        cov = np.asarray(cov_b, dtype=np.float64)
        self.finite = bool(np.isfinite(cov).all() and np.isfinite(self.mu).all())
        self.tr = float(np.trace(cov))
        if self.finite:
            w, v = np.linalg.eigh(0.5 * (cov + cov.T))
            self.root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T

    def tr_sqrt(self, cov_s):
        lam = np.linalg.eigvalsh(self.root @ cov_s @ self.root)
        return float(np.sqrt(np.maximum(lam, 0.0)).sum())

    def parts(self, rows):
        """-> (mean terms {0: .., 1: ..}, tr Sigma_s - 2 tr sqrt + tr Sigma_b) or None: what every mean mode shares computed once."""
        x = as_f64(rows)
        if x.shape[0] < 2 or not self.finite or not np.isfinite(x).all():
            return None
        cov_s = np.atleast_2d(np.cov(x, rowvar=False))
        rest = self.tr + float(np.trace(cov_s)) - 2.0 * self.tr_sqrt(cov_s)
        mt = {m: float(((self.mu - song_mean(rows, m)) ** 2).sum()) for m in (0, 1)}
        return mt, rest

    def score(self, rows, mean_mode=1):
        p = self.parts(rows)
        return None if p is None else p[0][mean_mode] + p[1]


def individual_scores(mu_b, cov_b, songs, mean_mode=1):
    b = Baseline(mu_b, cov_b)
    return [b.score(s, mean_mode) for s in songs]
