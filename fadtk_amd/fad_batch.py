"""Batch embedding driver -- mirror of fadtk/fad_batch.py:15-48 for one process per GPU.

fadtk splits the uncached files into ``workers`` contiguous chunks and embeds them in a spawn pool,
every worker loading its own copy of the model on cuda:0.  Here the unit of parallelism is the GPU:
when launched under torchrun (RANK / WORLD_SIZE set) each rank takes one contiguous shard of the
files and embeds it on its own device; ``workers`` becomes the number of host threads that decode /
resample audio ahead of the GPU.  Results land in the same cache layout
(<dir>/embeddings/<model>/<stem>.npy, float16).
"""
from __future__ import annotations

import logging
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Union

from . import dist
from .fad import FrechetAudioDistance
from .utils import get_cache_embedding_path

log = logging.getLogger("fadtk_amd")


class _DeviceFeeder:
    """Collects per-file float16 embeddings while they are still in HBM and folds them into an ``OnlineStats`` a
    group at a time (>= 64 files or 64 MiB of frames per GPU call: one launch of each kernel per group, per-file
    column sums never leave the device).  The reference instead writes every file, reads it back and merges per-file
    (mean, scatter, n) triplets on the host (fad_batch.py:43-48 + utils.py:19-46)."""
    GROUP_FILES, GROUP_BYTES = 64, 64 << 20

    def __init__(self, stats):
        self.stats = stats
        self.pending, self.bytes = [], 0

    def add(self, dev):
        self.pending.append(dev)
        self.bytes += dev.numel() * dev.element_size()
        if len(self.pending) >= self.GROUP_FILES or self.bytes >= self.GROUP_BYTES:
            self.flush()

    def add_host(self, arr):
        """A cached .npy: goes in as its own group (its dtype may differ from the device embeddings')."""
        self.flush()
        self.stats.add_group(arr, [arr.shape[0]])

    def flush(self):
        if not self.pending:
            return
        import torch
        pending, self.pending, self.bytes = self.pending, [], 0       # whatever happens below, this group is not retried
        sizes = [int(t.shape[0]) for t in pending]
        rows = torch.cat(pending, dim=0) if len(pending) > 1 else pending[0]
        self.stats.add_group(rows.contiguous(), sizes)


class _CacheWriter:
    """The embedding cache files (fad.py:188-201: part of the contract) leave the GPU loop: ONE device-to-host copy per group of files
    and the ``np.save`` calls run on a writer thread while the next group is embedded.  (The reference -- and rounds 1-5 here -- did a
    synchronous copy and an ``np.save`` per file inside the loop.)"""

    def __init__(self):
        self.pool = ThreadPoolExecutor(max_workers=1)
        self.jobs = []

    @staticmethod
    def _write(items, host):
        import numpy as np
        o = 0
        for cache, n in items:
            cache.parent.mkdir(parents=True, exist_ok=True)
            np.save(cache, host[o:o + n])
            o += n

    def submit(self, items, devs):
        """items: [(cache path, frames)], devs: the float16 device tensors in the same order."""
        import torch
        rows = torch.cat(devs, dim=0) if len(devs) > 1 else devs[0]
        host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
        host.copy_(rows, non_blocking=True)
        done = torch.cuda.Event()
        done.record()

        def job():
            done.synchronize()
            self._write(items, host.numpy())
        self.jobs.append(self.pool.submit(job))

    def submit_host(self, cache, embd):
        self.jobs.append(self.pool.submit(self._write, [(cache, embd.shape[0])], embd))

    def close(self):
        err = None
        for j in self.jobs:
            try:
                j.result()
            except Exception as e:      # noqa: BLE001
                err = err or e
        self.pool.shutdown()
        if err is not None:
            raise err


def _cache_embedding_batch(fs, ml, workers: int = 8, feeder=None, **kwargs):
    """Embed a list of files on this process's GPU; audio decode runs ``workers`` files ahead, ``ml.batch_files`` files share ONE
    front-end launch and ONE forward (``ModelLoader._get_embedding_batch``), the cache files are written behind the loop.
    With ``feeder`` (a _DeviceFeeder) every embedding is also accumulated while it is still in HBM."""
    import numpy as np
    fad = FrechetAudioDistance(ml, audio_load_worker=workers, **kwargs)
    if not fs:
        return
    import torch
    group_files = max(1, int(getattr(ml, "batch_files", 1)))
    depth = max(1, workers, group_files)
    on_gpu = torch.cuda.is_available() and getattr(ml, "device", None) is not None and ml.device.type == "cuda"
    writer = _CacheWriter()

    def embed_group(group):
        """group: [(file, cache, audio)] -> [(file, cache, float16 frames or None)]; a failing group is retried file by file so that
        only the file that fails is dropped (a bad file must not take the shard -- or its neighbours -- down)."""
        try:
            embs = ml._get_embedding_batch([a for _, _, a in group]) if len(group) > 1 else [ml._get_embedding(group[0][2])]
        except Exception as e:      # noqa: BLE001
            if len(group) == 1:
                log.error(f"Embedding {group[0][0]} with {ml.name} failed: {e}")
                return [(group[0][0], group[0][1], None)]
            return [r for g in group for r in embed_group([g])]
        out = []
        for (f, cache, _), e in zip(group, embs):
            e = e.detach()
            out.append((f, cache, (e.to(torch.float16) if e.dtype == torch.float32 else e).contiguous()))   # (model_loader.py:47-48)
        return out

    def flush(group):
        if not group:
            return
        done = [(f, cache, e) for f, cache, e in embed_group(group) if e is not None]
        if not done:
            return
        if on_gpu:
            writer.submit([(cache, int(e.shape[0])) for _, cache, e in done], [e for _, _, e in done])
        for _, cache, e in done:
            if not on_gpu:
                writer.submit_host(cache, e.cpu().numpy())
            if feeder is not None:
                # a GPU / library error of a group flush (64 files) is not this file's fault: it propagates, the shard
                # stops at once instead of embedding everything that follows for nothing
                feeder.add(e)

    try:
        with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
            pending = []
            it = iter(fs)

            def submit():
                f = next(it, None)
                if f is not None:
                    pending.append((f, pool.submit(fad.load_audio, f)))

            for _ in range(depth):
                submit()
            group = []
            while pending:
                f, fut = pending.pop(0)
                submit()
                cache = get_cache_embedding_path(ml.name, f)
                if cache.exists():
                    if feeder is not None:
                        flush(group); group = []                     # (the statistics take the files in order)
                        feeder.add_host(np.load(cache))
                    continue
                log.info(f"Loading {f} using {ml.name}")
                try:                                 # only the audio of THIS file is the file's own business
                    audio = fut.result()
                except Exception as e:      # noqa: BLE001  a bad file must not take the shard down
                    log.error(f"Embedding {f} with {ml.name} failed: {e}")
                    continue
                group.append((f, cache, audio))
                if len(group) >= group_files:
                    flush(group); group = []
            flush(group)
    finally:
        writer.close()
    if feeder is not None:
        feeder.flush()


def _select_device(ml, kwargs):
    """One process per GPU: under torchrun every rank drives the GPU named by LOCAL_RANK."""
    if dist.world_size() > 1:
        import torch
        if torch.cuda.is_available():
            torch.cuda.set_device(dist.env_local_rank())
            ml.device = torch.device("cuda", dist.env_local_rank())
            kwargs.setdefault("device", dist.env_local_rank())
        return dist.env_local_rank()
    return int(kwargs.get("device", 0))


def cache_embedding_files(files: Union[list, str, Path], ml, workers: int = 8, **kwargs):
    """Get embeddings for all audio files in a directory (or list), skipping cached ones.
    Multi-rank: rank 0 lists the uncached files and every rank shards THAT list (ranks listing on their own while
    others already write cache files would shard different lists), and no rank leaves before the closing barrier."""
    dist.init()
    todo = None
    if dist.rank() == 0:
        if isinstance(files, (str, Path)):
            files = sorted(Path(files).glob("*.*"))
        todo = [Path(f) for f in files if not get_cache_embedding_path(ml.name, f).exists()]
    todo = dist.broadcast_object(todo)
    if len(todo) == 0:
        log.info("All files already have embeddings, skipping.")
        dist.barrier()
        return
    log.info(f"[Frechet Audio Distance] Loading {len(todo)} audio files...")
    _select_device(ml, kwargs)
    _cache_embedding_batch(dist.shard(todo), ml, workers, **kwargs)
    dist.barrier()


def embed_and_accumulate(directory: Union[str, Path], ml, workers: int = 8, compat: bool = True, **kwargs):
    """One pass over a dataset: embed every file on this rank's GPU, keep the (float16) frames in HBM long enough
    to fold them into running (n, sum x, sum x x^T), write the usual embedding cache, all-reduce the packed
    statistics once (RCCL over xGMI) and let rank 0 store ``<dir>/stats/<model>/{mu,cov}.npy`` -- the cache
    ``FrechetAudioDistance.load_stats`` picks up, so a following ``score`` never re-reads the .npy files.

    compat=True adds the sum-reducible per-file mean terms (``fad_moments_update_file_means``) so that the result is
    what the reference's online path gives, including its per-file float16 rounding of the means (which is worth up to
    3e-4 of the FAD for files of a few frames); compat=False is the plain raw-moment estimate.  All accumulators of a
    rank live in one device buffer (``dist.SharedStats``): the exchange of the path is ONE in-place all-reduce.
    Returns (mu, cov) on every rank.
    """
    from .utils import OnlineStats, write_stats_cache
    directory = Path(directory)
    dist.init()
    files = dist.broadcast_object(sorted(p for p in directory.glob("*.*") if p.is_file()) if dist.rank() == 0 else None)
    dev_index = _select_device(ml, kwargs)
    d = ml.num_features
    shared = dist.SharedStats(d, 4 if compat else 1, dev_index, extra=2)
    stats = OnlineStats(d, dev_index, compat, shared=shared)
    _cache_embedding_batch(dist.shard(files), ml, workers, feeder=_DeviceFeeder(stats), **kwargs)
    import torch
    shared.extra.copy_(torch.tensor([stats.n_short, stats.n_empty], dtype=torch.float64))
    shared.allreduce()                                                 # the one collective of the data path
    stats.n_short, stats.n_empty = (int(round(v)) for v in shared.extra.cpu().tolist())
    mu, cov = stats.finish()
    n = stats.frames.count
    shared.close()
    if not compat:
        assert n >= 2, f"FAD requires at least two embedding window frames, you have {n}."
    if dist.rank() == 0:
        write_stats_cache(directory / "stats" / ml.name, mu, cov)
    dist.barrier()
    log.info(f"[{ml.name}] {n} frames from {len(files)} files accumulated on {dist.world_size()} GPU(s)")
    return mu, cov
