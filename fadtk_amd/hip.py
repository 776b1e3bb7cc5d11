"""Thin object layer over the C ABI: running moments, Frechet distance, batched per-song FAD.

Everything here forwards to libfad_hip.so; numpy is only used to own host buffers.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _capi as K


class Moments:
    """Running (n, sum x, sum x x^T) of frames in float64 HBM (``fad_moments_*``).

    Replaces ``np.mean``/``np.cov`` of fadtk/fad.py:48 and the per-file merge of
    fadtk/utils.py:13-45.  ``update`` accepts numpy arrays (host, staged over PCIe by the library)
    or torch CUDA tensors (used in place, on torch's current stream).
    """

    def __init__(self, d: int, device: int = 0):
        self._lib = K.load_library()
        K.require_gpu(device)
        self.d = int(d)
        self.device = int(device)
        h = C.c_void_p()
        K.check(self._lib.fad_moments_create(self.d, self.device, C.byref(h)), "fad_moments_create")
        self._h = h

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._lib.fad_moments_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _stream(self) -> int:
        return K.current_stream_ptr(self.device)

    # -- accumulation
    def bind(self, tensor) -> "Moments":
        """Keep the packed statistics in ``tensor`` (float64 CUDA, ``packed_len`` elements, contiguous) and reset.
        Collectives can then run over the tensor in place; the handle holds a reference to keep it alive."""
        assert tensor.is_cuda and tensor.dtype.is_floating_point and tensor.element_size() == 8
        assert tensor.numel() == self.packed_len and tensor.is_contiguous() and tensor.device.index == self.device
        K.check(self._lib.fad_moments_bind(self._h, C.c_void_p(tensor.data_ptr())), "fad_moments_bind")
        self._bound = tensor
        return self

    def reset(self):
        K.check(self._lib.fad_moments_reset(self._h, self._stream()), "fad_moments_reset")

    def release_inputs(self, staging: bool = True):
        """Forget the last device tensor fed (kept alive for the enqueued kernels -- call this only after something synchronised,
        e.g. finalize() or a collected score) and, with ``staging``, give back a host-input staging area above 256 MiB: a cached
        handle must not pin the caller's frames in HBM between calls, nor a large share of it -- but freeing and re-allocating the
        102 MB of a config-3 set on every call (hipFree synchronises, hipMalloc maps pages) cost ~0.5 ms of a 2.7 ms
        calc_embd_statistics (round 5); 256 MiB is 0.1 % of this GPU's memory."""
        self._keep = None
        if staging:
            K.check(self._lib.fad_moments_trim(self._h, 256 << 20), "fad_moments_trim")

    def settle(self):
        """Make a pending reset visible in the packed buffer (the zeroing is deferred until something reads it)."""
        K.check(self._lib.fad_moments_settle(self._h, self._stream()), "fad_moments_settle")

    def update(self, rows) -> "Moments":
        ptr, n, d, ld, code, on_dev, keep = K.rows_view(rows)
        if d != self.d:
            raise AssertionError(f"frame matrix has {d} features, accumulator has {self.d}")
        K.check(self._lib.fad_moments_update(self._h, ptr, n, ld, code, on_dev, self._stream()), "fad_moments_update")
        if on_dev:
            self._keep = keep          # torch tensor must outlive the enqueued kernels
        return self

    def update_segmented(self, rows, offsets: Sequence[int], want_sums: bool = True, sums_on_device: bool = False, want_runsums: bool = False):
        """Feed files/songs stored back to back; returns per-segment column sums [S x D] float64 -- a numpy array, or
        (``sums_on_device`` with device rows) a torch CUDA tensor that never leaves HBM.  ``want_runsums``: returns ``(sums, runsums)``
        with numpy's float32 running column sums per segment [S x D] float32 (``fad_moments_update_segmented_ref``; None for float64
        rows, whose numpy sum is the exact one)."""
        ptr, n, d, ld, code, on_dev, keep = K.rows_view(rows)
        if d != self.d:
            raise AssertionError(f"frame matrix has {d} features, accumulator has {self.d}")
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        n_seg = off.shape[0] - 1
        sums = None
        sums_ptr = None
        sums_dev = None
        runs, runs_ptr, runs_dev = None, None, None
        want_runsums = want_runsums and code != K.FAD_F64 and n_seg > 0
        if want_sums and n_seg > 0:
            if on_dev:
                import torch
                sums_dev = torch.empty((n_seg, self.d), dtype=torch.float64, device=keep.device)   # every entry is written (segment_gather_sums)
                sums_ptr = sums_dev.data_ptr()
            else:
                sums = np.zeros((n_seg, self.d), dtype=np.float64)
                sums_ptr = sums.ctypes.data
        if want_runsums:
            if on_dev:
                import torch
                runs_dev = torch.empty((n_seg, self.d), dtype=torch.float32, device=keep.device)
                runs_ptr = runs_dev.data_ptr()
            else:
                runs = np.zeros((n_seg, self.d), dtype=np.float32)
                runs_ptr = runs.ctypes.data
            K.check(self._lib.fad_moments_update_segmented_ref(
                self._h, ptr, n, ld, code, off.ctypes.data_as(C.POINTER(C.c_int64)), n_seg, sums_ptr, runs_ptr, on_dev,
                self._stream()), "fad_moments_update_segmented_ref")
        else:
            K.check(self._lib.fad_moments_update_segmented(
                self._h, ptr, n, ld, code, off.ctypes.data_as(C.POINTER(C.c_int64)), n_seg, sums_ptr, on_dev,
                self._stream()), "fad_moments_update_segmented")
        if on_dev:
            self._keep = keep
        if sums_dev is not None:
            sums = sums_dev if sums_on_device else sums_dev.cpu().numpy()
        if runs_dev is not None:
            runs = runs_dev if sums_on_device else runs_dev.cpu().numpy()
        return (sums, runs) if want_runsums else sums

    @staticmethod
    def update_multi(accs: Sequence["Moments"], blocks: Sequence) -> None:
        """``accs[i].update(blocks[i])`` for up to 32 accumulators of one dimension with ONE launch of each kernel
        (``fad_moments_update_multi``); every block must be a device tensor of one common dtype."""
        assert 1 <= len(accs) == len(blocks) <= 32
        views = [K.rows_view(b) for b in blocks]
        code = views[0][4]
        for a, v in zip(accs, views):
            if v[1] > 0 and v[2] != a.d:
                raise AssertionError(f"frame matrix has {v[2]} features, accumulator has {a.d}")
            if not v[5] or v[4] != code:
                raise AssertionError("update_multi needs device tensors of one common dtype")
        m = len(accs)
        hs = (C.c_void_p * m)(*[a._h for a in accs])
        ptrs = (C.c_void_p * m)(*[v[0] for v in views])
        ns = (C.c_int64 * m)(*[v[1] for v in views])
        lds = (C.c_int64 * m)(*[max(v[3], a.d) for a, v in zip(accs, views)])
        K.check(accs[0]._lib.fad_moments_update_multi(m, hs, ptrs, ns, lds, code, accs[0]._stream()), "fad_moments_update_multi")
        for a, v in zip(accs, views):
            a._keep = v[6]

    @staticmethod
    def update_multi_indexed(accs: Sequence["Moments"], rows, indices: Sequence) -> None:
        """``accs[i].update(rows[indices[i]])`` for up to 16 accumulators WITHOUT materialising the gathered matrices
        (``fad_moments_update_multi_indexed``): ``rows`` one resident device tensor [n_src x D], ``indices[i]`` int32 device tensors
        (1-D, values in [0, n_src)).  The resamples with replacement of FAD-inf (fad.py:333-337)."""
        import torch
        assert 1 <= len(accs) == len(indices) <= 16
        v = K.rows_view(rows)
        if not v[5]:
            raise AssertionError("update_multi_indexed needs a device tensor")
        m = len(accs)
        for a in accs:
            if v[2] != a.d:
                raise AssertionError(f"frame matrix has {v[2]} features, accumulator has {a.d}")
        idx = [i if (i.dtype == torch.int32 and i.is_contiguous()) else i.to(torch.int32).contiguous() for i in indices]
        for i in idx:
            assert i.is_cuda and i.dim() == 1
        hs = (C.c_void_p * m)(*[a._h for a in accs])
        ips = (C.c_void_p * m)(*[i.data_ptr() for i in idx])
        ns = (C.c_int64 * m)(*[int(i.numel()) for i in idx])
        K.check(accs[0]._lib.fad_moments_update_multi_indexed(m, hs, v[0], int(v[1]), int(max(v[3], accs[0].d)), v[4], ips, ns, accs[0]._stream()),
                "fad_moments_update_multi_indexed")
        for a, i in zip(accs, idx):
            a._keep = (v[6], i)

    @staticmethod
    def prepared_update_multi(accs: Sequence["Moments"], blocks: Sequence) -> "PreparedMultiUpdate":
        """``update_multi`` for a loop that feeds the SAME accumulators from the SAME device tensors again and again: see PreparedMultiUpdate."""
        return PreparedMultiUpdate(accs, blocks)

    @staticmethod
    def update_file_means(exact: "Moments", rounded: "Moments", weighted: "Moments", seg_sums, sizes, dtype_code: int, seg_runsums=None) -> None:
        """Accumulate the per-file mean rows of the online statistics (``fad_moments_update_file_means[_ref]``).
        ``seg_sums`` [F x D] float64 and ``sizes`` [F] int64: both numpy, or both torch CUDA tensors (sizes may stay on the host);
        ``seg_runsums`` [F x D] float32 (where ``seg_sums`` lives) = numpy's per-file running sums: the rounded means are then the
        reference's own (utils.py:16), else the rounded exact means."""
        lib = exact._lib
        if K._is_torch(seg_sums) and seg_sums.is_cuda:
            import torch
            sums_t = seg_sums.to(torch.float64).contiguous()
            n_files = int(sums_t.shape[0])
            if K._is_torch(sizes) and sizes.is_cuda:
                sizes_t = sizes.to(torch.int64).contiguous()
                flag, sizes_ptr, keep = 3, sizes_t.data_ptr(), sizes_t
            else:                                       # the usual case: sums in HBM, sizes known on the host
                sz = np.ascontiguousarray(np.asarray(sizes.cpu() if K._is_torch(sizes) else sizes, dtype=np.int64))
                flag, sizes_ptr, keep = 1, sz.ctypes.data, sz
            if seg_runsums is not None:
                runs_t = seg_runsums.to(torch.float32).contiguous()
                assert runs_t.is_cuda and tuple(runs_t.shape) == tuple(sums_t.shape)
                K.check(lib.fad_moments_update_file_means_ref(exact._h, rounded._h, weighted._h, sums_t.data_ptr(), runs_t.data_ptr(),
                                                              sizes_ptr, n_files, int(dtype_code), flag | 4, exact._stream()),
                        "fad_moments_update_file_means_ref")
                exact._keep = (sums_t, runs_t, keep)
            else:
                K.check(lib.fad_moments_update_file_means(exact._h, rounded._h, weighted._h, sums_t.data_ptr(),
                                                          sizes_ptr, n_files, int(dtype_code), flag, exact._stream()),
                        "fad_moments_update_file_means")
                exact._keep = (sums_t, keep)
        else:
            sums = K.f64_host(seg_sums)
            sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64))
            if seg_runsums is not None:
                runs = np.ascontiguousarray(np.asarray(seg_runsums, dtype=np.float32))
                assert runs.shape == sums.shape
                K.check(lib.fad_moments_update_file_means_ref(exact._h, rounded._h, weighted._h, sums.ctypes.data, runs.ctypes.data,
                                                              sz.ctypes.data, int(sums.shape[0]), int(dtype_code), 0, exact._stream()),
                        "fad_moments_update_file_means_ref")
            else:
                K.check(lib.fad_moments_update_file_means(exact._h, rounded._h, weighted._h, sums.ctypes.data,
                                                          sz.ctypes.data, int(sums.shape[0]), int(dtype_code), 0, exact._stream()),
                        "fad_moments_update_file_means")

    def merge(self, other: "Moments") -> "Moments":
        K.check(self._lib.fad_moments_merge(self._h, other._h, self._stream()), "fad_moments_merge")
        return self

    def allreduce_rccl(self, comm_ptr: int) -> "Moments":
        """Sum the statistics of all ranks in place through the caller's ``ncclComm_t`` (its address as an int).
        Python hosts normally go through ``fadtk_amd.dist.allreduce_moments`` (torch.distributed) instead."""
        K.check(self._lib.fad_moments_allreduce(self._h, C.c_void_p(comm_ptr), self._stream()), "fad_moments_allreduce")
        return self

    # -- packed statistics (what an RCCL all-reduce runs over)
    @property
    def packed_len(self) -> int:
        return 1 + self.d + self.d * self.d

    def export(self) -> np.ndarray:
        out = np.empty(self.packed_len, dtype=np.float64)
        K.check(self._lib.fad_moments_export(self._h, out.ctypes.data, 0, self._stream()), "fad_moments_export")
        return out

    def export_to(self, tensor):
        """Copy the packed statistics into a float64 torch CUDA tensor of ``packed_len`` elements."""
        assert tensor.is_cuda and tensor.numel() == self.packed_len and tensor.is_contiguous()
        K.check(self._lib.fad_moments_export(self._h, tensor.data_ptr(), 1, self._stream()), "fad_moments_export")
        return tensor

    def import_(self, packed) -> "Moments":
        if K._is_torch(packed) and packed.is_cuda:
            assert packed.numel() == self.packed_len and packed.is_contiguous()
            K.check(self._lib.fad_moments_import(self._h, packed.data_ptr(), 1, self._stream()), "fad_moments_import")
        else:
            a = K.f64_host(packed, (self.packed_len,))
            K.check(self._lib.fad_moments_import(self._h, a.ctypes.data, 0, self._stream()), "fad_moments_import")
        return self

    @property
    def count(self) -> int:
        n = C.c_int64()
        K.check(self._lib.fad_moments_count(self._h, C.byref(n), self._stream()), "fad_moments_count")
        return int(n.value)

    def finalize(self, ddof: int = 1) -> Tuple[np.ndarray, np.ndarray, int]:
        """-> (mu [D] float64, cov [D x D] float64, n).  n < 2 raises AssertionError (fad.py:46-47)."""
        mu = np.empty(self.d, dtype=np.float64)
        cov = np.empty((self.d, self.d), dtype=np.float64)
        n = C.c_int64()
        K.check(self._lib.fad_moments_finalize(self._h, int(ddof), mu.ctypes.data, cov.ctypes.data, C.byref(n), 0,
                                               self._stream()), "fad_moments_finalize")
        return mu, cov, int(n.value)

    # -- timing of the dominant kernel (bench.py)
    def set_reference_mean(self, on: bool = True, detached: bool = False) -> None:
        """Carry numpy's float32 running column sums beside the exact ones (``fad_moments_set_reference_mean``): ``finalize`` then
        returns the mean ``np.mean(frames, axis=0)`` has (fadtk/fad.py:48) before its final cast -- bit for bit after the caller's
        ``astype`` -- instead of the exact mean.  The walk runs on a stream of its own beside the update's other kernels;
        ``detached=True``: the caller vouches that the frames it feeds are complete at the call and stay unchanged until the statistics
        are next read -- the walk then waits for nothing and holds nothing up (see include/fad_hip.h)."""
        K.check(self._lib.fad_moments_set_reference_mean(self._h, (2 if detached else 1) if on else 0))

    def set_timing(self, on=True):
        """True / 1: events around the tile kernel and behind the reduce; 2: around the tile kernel only; False / 0: off."""
        K.check(self._lib.fad_moments_set_timing(self._h, 2 if on == 2 else (1 if on else 0)))

    def last_timing(self):
        a, b, v = C.c_float(), C.c_float(), C.c_int()
        K.check(self._lib.fad_moments_last_timing(self._h, C.byref(a), C.byref(b), C.byref(v)))
        return float(a.value), float(b.value), int(v.value)


def cu_masked_stream(cus_per_xcd, device: int = 0, xcds: int = 8, cus_in_xcd: int = 32):
    """A torch stream confined to CUs `cus_per_xcd` = range(lo, hi) of every XCD (diagnostics: bench.py --chain-cus).  Mask bit
    i = CU i of the runtime's numbering, XCD-interleaved: CU c of XCD x is bit c * xcds + x."""
    import torch
    lib = K.load_library()
    K.require_gpu(device)
    words = (xcds * cus_in_xcd + 31) // 32
    mask = (C.c_uint32 * words)()
    for c in cus_per_xcd:
        for x in range(xcds):
            bit = c * xcds + x
            mask[bit // 32] |= (1 << (bit % 32))
    ptr = C.c_void_p()
    K.check(lib.fad_stream_create_cu_mask(int(device), mask, words, C.byref(ptr)), "fad_stream_create_cu_mask")
    return torch.cuda.ExternalStream(ptr.value, device=torch.device("cuda", device))


def frechet(mu1, cov1, mu2, cov2, eps: float = 1e-6, max_iter: int = 0, tol: float = 0.0, device: int = 0):
    """``fad_frechet`` on host float64 arrays -> (fad, diag dict).  Shapes are checked by the caller."""
    lib = K.load_library()
    K.require_gpu(device)
    mu1 = K.f64_host(mu1)
    mu2 = K.f64_host(mu2)
    d = mu1.shape[0]
    cov1 = K.f64_host(cov1, (d, d))
    cov2 = K.f64_host(cov2, (d, d))
    out = C.c_double()
    diag = K.FadDiag()
    st = lib.fad_frechet(d, mu1.ctypes.data, cov1.ctypes.data, mu2.ctypes.data, cov2.ctypes.data, float(eps),
                         int(max_iter), float(tol), 0, int(device), K.current_stream_ptr(device), C.byref(out),
                         C.byref(diag))
    K.check(st, "fad_frechet")
    return float(out.value), diag.as_dict()


def frechet_from_moments(m1: Moments, m2: Moments, ddof: int = 1, eps: float = 1e-6, max_iter: int = 0,
                         tol: float = 0.0, mean_dtype: int = -1):
    """FAD straight from two accumulators, all in HBM (``fad_frechet_from_moments``).  ``mean_dtype`` = ``K.FAD_F16``
    gives the reference's value for float16 embeddings (means and mean term rounded the way numpy does)."""
    lib = K.load_library()
    out = C.c_double()
    diag = K.FadDiag()
    st = lib.fad_frechet_from_moments(m1._h, m2._h, int(ddof), float(eps), int(max_iter), float(tol), int(mean_dtype),
                                      K.current_stream_ptr(m1.device), C.byref(out), C.byref(diag))
    K.check(st, "fad_frechet_from_moments")
    return float(out.value), diag.as_dict()


class FrechetJob:
    """A score in flight (``fad_frechet_from_moments_begin``): the whole square-root chain is enqueued on the stream that
    was current when it was created; ``result()`` waits for it -> (fad, diag dict).

    The slot behind a job belongs to the host thread that created it (the library keeps its workspaces per thread and frees
    them when the thread ends), so ``result()`` / ``cancel()`` from another thread raise, and a job that is garbage-collected
    on another thread -- or after its thread has gone -- is left alone instead of touching a workspace that may no longer
    exist."""

    def __init__(self, m1: Moments, m2: Moments, ddof: int = 1, eps: float = 1e-6, mean_dtype: int = -1):
        import threading
        self._lib = K.load_library()
        self._owner = threading.get_ident()
        job = C.c_void_p()
        K.check(self._lib.fad_frechet_from_moments_begin(m1._h, m2._h, int(ddof), float(eps), int(mean_dtype),
                                                         K.current_stream_ptr(m1.device), C.byref(job)),
                "fad_frechet_from_moments_begin")
        self._job = job

    def _on_owner_thread(self) -> bool:
        import threading
        return threading.get_ident() == self._owner

    def result(self):
        if self._job is None:
            raise RuntimeError("this job was collected already")
        if not self._on_owner_thread():
            raise RuntimeError("a FrechetJob must be collected by the thread that created it (its slot is thread-local)")
        out, diag = C.c_double(), K.FadDiag()
        job, self._job = self._job, None
        K.check(self._lib.fad_frechet_end(job, C.byref(out), C.byref(diag)), "fad_frechet_end")
        return float(out.value), diag.as_dict()

    def cancel(self):
        """Give the slot back without collecting the score (waits for the enqueued kernels)."""
        if self._job is not None:
            if not self._on_owner_thread():
                raise RuntimeError("a FrechetJob must be cancelled by the thread that created it (its slot is thread-local)")
            job, self._job = self._job, None
            K.check(self._lib.fad_frechet_cancel(job), "fad_frechet_cancel")

    def __del__(self):            # a job dropped without result(): its slot must not stay taken (8 per thread)
        try:
            if getattr(self, "_job", None) is not None:
                if self._on_owner_thread():
                    self.cancel()
                else:             # the slot is thread-local: it stays taken until its thread ends -- say so instead of failing later
                    import warnings
                    warnings.warn("a FrechetJob was dropped on a thread other than the one that created it: its slot (8 per thread "
                                  "and device) stays busy until that thread ends; call result() or cancel() on the owner thread",
                                  ResourceWarning, stacklevel=2)
        except Exception:         # noqa: BLE001  interpreter shutdown, library gone
            pass


class PreparedMultiUpdate:
    """``Moments.update_multi(accs, blocks)`` with the views and ctypes tables built ONCE: a loop that scores resident sets over and over
    (bench.py's; a service that re-scores a fixed evaluation set against changing baselines) spends 5-6 us of Python per frame matrix in
    ``update_multi`` -- 0.2 ms for the 32 matrices of a batch, during which the GPU waits for its first launch.  ``run()`` is one call into
    the library (two with ``reset=True``: ``fad_moments_reset_multi`` first).  The tensors are kept alive by the object."""

    def __init__(self, accs, blocks):
        assert 1 <= len(accs) == len(blocks) <= 32
        views = [K.rows_view(b) for b in blocks]
        code = views[0][4]
        for a, v in zip(accs, views):
            if v[1] > 0 and v[2] != a.d:
                raise AssertionError(f"frame matrix has {v[2]} features, accumulator has {a.d}")
            if not v[5] or v[4] != code:
                raise AssertionError("update_multi needs device tensors of one common dtype")
        m = len(accs)
        self._accs, self._keep, self._m, self._code = list(accs), [v[6] for v in views], m, code
        self._hs = (C.c_void_p * m)(*[a._h for a in accs])
        self._ptrs = (C.c_void_p * m)(*[v[0] for v in views])
        self._ns = (C.c_int64 * m)(*[v[1] for v in views])
        self._lds = (C.c_int64 * m)(*[max(v[3], a.d) for a, v in zip(accs, views)])
        self._lib = accs[0]._lib

    def run(self, reset: bool = False) -> None:
        st = self._accs[0]._stream()
        if reset:
            K.check(self._lib.fad_moments_reset_multi(self._m, self._hs, st), "fad_moments_reset_multi")
        K.check(self._lib.fad_moments_update_multi(self._m, self._hs, self._ptrs, self._ns, self._lds, self._code, st), "fad_moments_update_multi")
        for a, k in zip(self._accs, self._keep):
            a._keep = k


class FrechetMultiJob:
    """Up to MAX_PAIRS scores in flight as ONE batch (``fad_frechet_from_moments_multi_begin``): pair b = (pairs[b][0], pairs[b][1]);
    the eight launches of the square-root chain carry all of them.  ``result()`` -> [(fad, diag dict), ...] in order.  Thread
    rules as FrechetJob."""

    MAX_PAIRS = 32                 # FAD_MULTI_MAX_PAIRS (include/fad_hip.h)

    def __init__(self, pairs, ddof: int = 1, eps: float = 1e-6, mean_dtype: int = -1):
        import threading
        self._lib = K.load_library()
        self._owner = threading.get_ident()
        self._n = len(pairs)
        if not 1 <= self._n <= self.MAX_PAIRS:
            raise ValueError(f"a FrechetMultiJob holds 1..{self.MAX_PAIRS} pairs")
        a = (C.c_void_p * self._n)(*[p[0]._h for p in pairs])
        b = (C.c_void_p * self._n)(*[p[1]._h for p in pairs])
        job = C.c_void_p()
        K.check(self._lib.fad_frechet_from_moments_multi_begin(self._n, a, b, int(ddof), float(eps), int(mean_dtype),
                                                               K.current_stream_ptr(pairs[0][0].device), C.byref(job)),
                "fad_frechet_from_moments_multi_begin")
        self._job = job

    def result(self):
        import threading
        if self._job is None:
            raise RuntimeError("this job was collected already")
        if threading.get_ident() != self._owner:
            raise RuntimeError("a FrechetMultiJob must be collected by the thread that created it (its slot is thread-local)")
        out = (C.c_double * self._n)()
        diag = (K.FadDiag * self._n)()
        job, self._job = self._job, None
        K.check(self._lib.fad_frechet_multi_end(job, self._n, out, diag), "fad_frechet_multi_end")
        return [(float(out[i]), diag[i].as_dict()) for i in range(self._n)]

    def result_arrays(self):
        """``result()`` without the per-pair Python objects: (float64 array of the distances, the ctypes array of fad_diag_t records --
        ``diags[i].as_dict()`` on demand).  Thirty-two dicts of diagnostics cost more host time than the library's own collection."""
        import threading
        if self._job is None:
            raise RuntimeError("this job was collected already")
        if threading.get_ident() != self._owner:
            raise RuntimeError("a FrechetMultiJob must be collected by the thread that created it (its slot is thread-local)")
        out = np.empty(self._n, dtype=np.float64)
        diag = (K.FadDiag * self._n)()
        job, self._job = self._job, None
        K.check(self._lib.fad_frechet_multi_end(job, self._n, out.ctypes.data_as(C.POINTER(C.c_double)), diag), "fad_frechet_multi_end")
        return out, diag

    def cancel(self):
        import threading
        if self._job is not None and threading.get_ident() == self._owner:
            job, self._job = self._job, None
            K.check(self._lib.fad_frechet_cancel(job), "fad_frechet_cancel")

    def __del__(self):
        try:
            self.cancel()
        except Exception:         # noqa: BLE001
            pass


def frechet_batched(mu_b, cov_b, rows, offsets: Sequence[int], mean_mode: int = 1, device: int = 0):
    """Per-song FAD against one baseline (``fad_frechet_batched_vs_baseline``).

    -> (scores float64 [S], status int32 [S]); songs with < 2 frames get NaN and FAD_ERR_TOO_FEW_ROWS.
    """
    lib = K.load_library()
    K.require_gpu(device)
    base_on_dev = K._is_torch(mu_b) and K._is_torch(cov_b) and mu_b.is_cuda and cov_b.is_cuda
    if base_on_dev:                 # a baseline that already lives in HBM (float64) is used in place: no 8 D^2-byte upload per call
        import torch
        mu_t = mu_b.to(torch.float64).contiguous(); cov_t = cov_b.to(torch.float64).contiguous()
        d = int(mu_t.shape[0])
        assert tuple(cov_t.shape) == (d, d)
    else:
        mu_b = K.f64_host(mu_b)
        d = mu_b.shape[0]
        cov_b = K.f64_host(cov_b, (d, d))
    ptr, n, dd, ld, code, on_dev, keep = K.rows_view(rows, host_bf16=True)      # (host bfloat16 rows: their means rounded as on the device)
    if n > 0 and dd != d:
        raise AssertionError(f"songs have {dd} features, baseline has {d}")
    if base_on_dev and not on_dev:
        mu_b, cov_b, base_on_dev = mu_t.cpu().numpy(), cov_t.cpu().numpy(), False      # host rows: the library stages everything itself
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    n_songs = off.shape[0] - 1
    scores = np.full(max(n_songs, 0), np.nan, dtype=np.float64)
    status = np.zeros(max(n_songs, 0), dtype=np.int32)
    if on_dev:
        # baseline must live where the rows live
        import torch
        if not base_on_dev:
            mu_t = torch.from_numpy(mu_b).to(keep.device)
            cov_t = torch.from_numpy(cov_b).to(keep.device)
        elif mu_t.device != keep.device:
            mu_t, cov_t = mu_t.to(keep.device), cov_t.to(keep.device)
        mu_p, cov_p = mu_t.data_ptr(), cov_t.data_ptr()
    else:
        mu_p, cov_p = mu_b.ctypes.data, cov_b.ctypes.data
    st = lib.fad_frechet_batched_vs_baseline(d, mu_p, cov_p, ptr, n, max(ld, d), code,
                                             off.ctypes.data_as(C.POINTER(C.c_int64)), n_songs, int(mean_mode),
                                             on_dev, int(device), K.current_stream_ptr(device),
                                             scores.ctypes.data, status.ctypes.data)
    K.check(st, "fad_frechet_batched_vs_baseline")
    return scores, status


# ---------------------------------------------------------------------------------------------
# log-mel front ends (csrc/logmel.hip)
# ---------------------------------------------------------------------------------------------
def _clips_view(clips, device: int):
    """list of 1-D arrays (numpy / torch) or one 1-D array -> (ptr, offsets int64[n+1], on_device, keepalive)."""
    if not isinstance(clips, (list, tuple)):
        clips = [clips]
    if len(clips) and K._is_torch(clips[0]) and clips[0].is_cuda:
        import torch
        flat = torch.cat([c.reshape(-1).to(torch.float32) for c in clips]) if len(clips) > 1 else \
            clips[0].reshape(-1).to(torch.float32).contiguous()
        lens = [int(c.numel()) for c in clips]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return flat.data_ptr(), off, 1, flat
    arrs = [np.asarray(c.cpu().numpy() if K._is_torch(c) else c, dtype=np.float32).reshape(-1) for c in clips]
    flat = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(0, np.float32)
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    return flat.ctypes.data, off, 0, flat


def _out_buffer(shape, on_dev: int, like):
    if on_dev:
        import torch
        t = torch.empty(shape, dtype=torch.float32, device=like.device)
        return t, t.data_ptr()
    a = np.empty(shape, dtype=np.float32)
    return a, a.ctypes.data


def vggish_num_examples(n_samples: int) -> int:
    return int(K.load_library().fad_logmel_vggish_num_examples(int(n_samples)))


def logmel_vggish(clips, device: int = 0):
    """16 kHz mono clips -> (examples [E, 96, 64] float32, example_offsets int64 [n_clips + 1])."""
    lib = K.load_library()
    K.require_gpu(device)
    ptr, off, on_dev, keep = _clips_view(clips, device)
    n = len(off) - 1
    total = sum(vggish_num_examples(int(off[i + 1] - off[i])) for i in range(n))
    out, optr = _out_buffer((total, 96, 64), on_dev, keep)
    ex_off = np.zeros(n + 1, dtype=np.int64)
    K.check(lib.fad_logmel_vggish(ptr, off.ctypes.data_as(C.POINTER(C.c_int64)), n, optr, total,
                                  ex_off.ctypes.data_as(C.POINTER(C.c_int64)), on_dev, device,
                                  K.current_stream_ptr(device)), "fad_logmel_vggish")
    return out, ex_off


def logmel_whisper(clips, n_mels: int = 80, device: int = 0):
    """16 kHz mono clips -> [n_clips, n_mels, 3000] float32 (each clip padded / cut to 30 s)."""
    lib = K.load_library()
    K.require_gpu(device)
    ptr, off, on_dev, keep = _clips_view(clips, device)
    n = len(off) - 1
    out, optr = _out_buffer((n, n_mels, 3000), on_dev, keep)
    K.check(lib.fad_logmel_whisper(ptr, off.ctypes.data_as(C.POINTER(C.c_int64)), n, int(n_mels), optr, on_dev, device,
                                   K.current_stream_ptr(device)), "fad_logmel_whisper")
    return out


def logmel_htsat(clips, device: int = 0):
    """48 kHz mono clips of ONE common length -> [n_clips, 1 + n/480, 64] float32 (dB log-mel).  Clips of 512 samples or
    fewer are refused (AssertionError, FAD_ERR_SHAPE): the centred STFT reflects 512 samples at each end, which needs a longer
    clip -- torch.stft(center=True, pad_mode="reflect") on the reference's path refuses them too."""
    lib = K.load_library()
    K.require_gpu(device)
    ptr, off, on_dev, keep = _clips_view(clips, device)
    n = len(off) - 1
    frames = 1 + int(off[1] - off[0]) // 480 if n else 1
    out, optr = _out_buffer((n, frames, 64), on_dev, keep)
    K.check(lib.fad_logmel_htsat(ptr, off.ctypes.data_as(C.POINTER(C.c_int64)), n, frames, optr, on_dev, device,
                                 K.current_stream_ptr(device)), "fad_logmel_htsat")
    return out


def resample_kaiser(wav, orig_sr: int, new_sr: int, quantize_pcm16: bool = False, device: int = 0):
    """Mono float32 audio (numpy, or a torch CUDA tensor that stays on the device) resampled from ``orig_sr`` to
    ``new_sr`` with fadtk's Kaiser-windowed sinc filter (fad.py:151-159); ``quantize_pcm16`` adds the reference's
    16-bit cache-file round trip."""
    lib = K.load_library()
    K.require_gpu(device)
    ptr, off, on_dev, keep = _clips_view([wav], device)
    n = int(off[1])
    n_out = int(lib.fad_resample_num_samples(n, int(orig_sr), int(new_sr)))
    if n_out < 0:
        K.check(n_out, "fad_resample_num_samples")
    out, optr = _out_buffer((n_out,), on_dev, keep)
    K.check(lib.fad_resample_kaiser(ptr, n, int(orig_sr), int(new_sr), int(bool(quantize_pcm16)), optr, n_out, on_dev, device,
                                    K.current_stream_ptr(device)), "fad_resample_kaiser")
    return out


# ---------------------------------------------------------------------------------------------- Kernel Audio Distance
def _kad_rows(x, what: str):
    """-> rows_view of a float16 / bfloat16 / float32 frame matrix; float64 and other dtypes are refused, not converted."""
    if K._is_torch(x):
        import torch
        ok = x.dtype in (torch.float16, torch.bfloat16, torch.float32)
    else:
        x = np.asarray(x)
        ok = x.dtype in (np.float16, np.float32)
    if not ok:
        raise ValueError(f"KAD takes float16, bfloat16 or float32 rows; {what} is {x.dtype}: cast it (e.g. .astype(np.float32))")
    return K.rows_view(x)


def _kad_pair(x, y, what: str, device: int):
    """-> (_kad_rows(x), _kad_rows(y)); a numpy set next to a torch CUDA one (or a CPU tensor next to a CUDA one) is copied to the device."""
    if K._is_torch(x) != K._is_torch(y) or (K._is_torch(x) and x.is_cuda != y.is_cuda):
        import torch
        dev = torch.device("cuda", device)
        x = x if K._is_torch(x) else torch.from_numpy(np.ascontiguousarray(x))
        y = y if K._is_torch(y) else torch.from_numpy(np.ascontiguousarray(y))
        x, y = x.to(dev), y.to(dev)
    return _kad_rows(x, "x"), _kad_rows(y, what)


def _kad_bandwidth(bandwidth: Optional[float]) -> float:
    """-> the C ABI's bandwidth argument: 0 for None (the median), else a value > 0."""
    bw = 0.0 if bandwidth is None else float(bandwidth)
    if bandwidth is not None and not bw > 0:
        raise ValueError(f"KAD: bandwidth must be > 0, got {bandwidth}")
    return bw


KAD_KERNELS = {"gaussian": K.FAD_KAD_GAUSSIAN, "iq": K.FAD_KAD_IQ, "imq": K.FAD_KAD_IMQ}


def kad_kernel_code(kernel: str) -> int:
    """-> the C ABI's kernel argument (FAD_KAD_*) of a kernel name: "gaussian" exp(-t), "iq" 1 / (1 + t) or "imq" 1 / sqrt(1 + t),
    t = |a - b|^2 / (2 sigma^2).  Any other name is a ValueError, raised before the native library is touched."""
    if not isinstance(kernel, str) or kernel not in KAD_KERNELS:
        raise ValueError(f"KAD: kernel must be one of {', '.join(map(repr, KAD_KERNELS))}, got {kernel!r}")
    return KAD_KERNELS[kernel]


def kad_last_plan() -> dict:
    """``fad_kad_last_plan``: how this thread's last KAD-family call cut its passes into launches -> dict of ``passes``, ``launches``,
    ``min_launches`` and ``max_launches`` (of one pass) and ``slots_per_workgroup`` (the most any launch's workgroups walk)."""
    out = (C.c_int64 * 5)()
    K.check(K.load_library().fad_kad_last_plan(out), "fad_kad_last_plan")
    return dict(zip(("passes", "launches", "min_launches", "max_launches", "slots_per_workgroup"), map(int, out)))


def kad_median_distance(x, device: int = 0) -> float:
    """``fad_kad_median_distance``: np.median(scipy.spatial.distance.pdist(x)) of one set of rows (numpy on the host, or a torch CUDA
    tensor used in place on torch's current stream)."""
    lib = K.load_library()
    ptr, n, d, ld, code, on_dev, keep = _kad_rows(x, "x")
    out = C.c_double()
    K.check(lib.fad_kad_median_distance(ptr, n, ld, d, code, on_dev, C.byref(out), int(device), K.current_stream_ptr(device)),
            "fad_kad_median_distance")
    return float(out.value)


def kad(x, y, bandwidth: Optional[float] = None, device: int = 0, kernel: str = "gaussian") -> dict:
    """``fad_kad_k``: the unbiased kernel MMD^2 between the rows of x (baseline) and y -> dict of fad_kad_result
    (mmd2, kxx_mean, kyy_mean, kxy_mean, bandwidth, n, m).  ``bandwidth=None``: the median pairwise distance of x.  ``kernel``:
    "gaussian" (the default), "iq" or "imq" (kad_kernel_code).
    Both sets are numpy arrays or both torch CUDA tensors of one dtype (float16 / bfloat16 / float32)."""
    kf = kad_kernel_code(kernel)
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"KAD: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("KAD: x and y must have the same dtype")
    res = K.FadKadResult()
    bw = _kad_bandwidth(bandwidth)
    K.check(lib.fad_kad_k(px, n, ldx, py, m, ldy, d, cx, dev_x, bw, kf, C.byref(res), int(device), K.current_stream_ptr(device)), "fad_kad")
    return res.as_dict()


KAD_MAX_BANDWIDTHS = 32


def kad_sweep_bandwidths(bandwidths=None, factors=None):
    """-> (float64 array [B], relative): the C ABI's bandwidth list of ``fad_kad_sweep`` and whether it holds factors of the baseline's
    median distance.  Exactly one of the two is given, 1 .. 32 finite values > 0; anything else is a ValueError, raised before the
    native library is touched."""
    if (bandwidths is None) == (factors is None):
        raise ValueError("KAD sweep: give exactly one of bandwidths (sigma values) and factors (of the baseline's median distance)")
    what, given = ("factors", factors) if bandwidths is None else ("bandwidths", bandwidths)
    try:
        v = np.array(list(given) if not isinstance(given, np.ndarray) else given, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"KAD sweep: {what} must be a sequence of numbers, got {given!r}") from None
    if not 1 <= v.size <= KAD_MAX_BANDWIDTHS:
        raise ValueError(f"KAD sweep takes 1 .. {KAD_MAX_BANDWIDTHS} {what}, got {v.size}")
    if not (np.isfinite(v) & (v > 0)).all():
        raise ValueError(f"KAD sweep: every one of {what} must be finite and > 0, got {v.tolist()}")
    return np.ascontiguousarray(v), int(bandwidths is None)


def kad_sweep(x, y, bandwidths=None, factors=None, device: int = 0, kernel: str = "gaussian") -> dict:
    """``fad_kad_sweep``: ``kad`` at B bandwidths in one call -- both sets packed once, a tile's dot products formed once for up to 8
    bandwidths -> dict of float64 arrays ``mmd2``, ``kxx_mean``, ``kyy_mean``, ``kxy_mean``, ``bandwidth`` [B] in the order given, plus
    ``n`` and ``m``.  ``bandwidths``: the sigma values themselves; ``factors``: multiples of the median pairwise distance of x (found
    once; the factor 1 is ``kad``'s default).  Exactly one of the two, 1 .. 32 finite values > 0.  Entry b carries the bits of
    ``kad(x, y, bandwidth=sigma_b)``.  x, y and ``kernel`` as ``kad`` takes them."""
    kf = kad_kernel_code(kernel)
    bw, relative = kad_sweep_bandwidths(bandwidths, factors)
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"KAD: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("KAD: x and y must have the same dtype")
    B = int(bw.size)
    res = (K.FadKadResult * B)()
    K.check(lib.fad_kad_sweep(px, n, ldx, py, m, ldy, d, cx, dev_x, bw.ctypes.data_as(C.POINTER(C.c_double)), B, relative, kf, res,
                              int(device), K.current_stream_ptr(device)), "fad_kad_sweep")
    out = {k: np.array([getattr(r, k) for r in res], dtype=np.float64) for k in ("mmd2", "kxx_mean", "kyy_mean", "kxy_mean", "bandwidth")}
    out.update(n=int(res[0].n), m=int(res[0].m))
    return out


def kad_individual(x, rows, offsets: Sequence[int], bandwidth: Optional[float] = None, device: int = 0,
                   kernel: str = "gaussian") -> dict:
    """``fad_kad_individual_k``: KAD between the baseline rows x and every song s = rows[offsets[s]:offsets[s + 1]], one sigma for all
    (``bandwidth=None``: the median pairwise distance of x) -> dict of float64 arrays ``mmd2``, ``kyy_mean``, ``kxy_mean`` and int32
    ``status`` [S] (NaN where status is FAD_ERR_TOO_FEW_ROWS or FAD_ERR_NOT_FINITE), plus ``kxx_mean``, ``bandwidth`` and ``n``.
    ``kernel``: "gaussian", "iq" or "imq".  x and rows are both numpy arrays or both torch CUDA tensors of one dtype (float16 /
    bfloat16 / float32)."""
    kf = kad_kernel_code(kernel)
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, rows, "rows", device)
    if m > 0 and d != dy:
        raise ValueError(f"KAD: x has D = {d}, the songs have D = {dy}")
    if m > 0 and cx != cy:
        raise ValueError("KAD: x and the songs must have the same dtype")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if off.ndim != 1 or off.shape[0] < 1:
        raise ValueError("KAD: offsets must be a 1-D sequence of S + 1 row indices")
    S = off.shape[0] - 1
    bw = _kad_bandwidth(bandwidth)
    out = {k: np.full(S, np.nan) for k in ("mmd2", "kyy_mean", "kxy_mean")}
    out["status"] = np.zeros(S, dtype=np.int32)
    res = K.FadKadResult()
    K.check(lib.fad_kad_individual_k(px, n, ldx, py if m > 0 else None, m, max(ldy, d), off.ctypes.data_as(C.POINTER(C.c_int64)), S, d,
                                     cx, dev_x, bw, kf, C.byref(res), out["mmd2"].ctypes.data, out["kyy_mean"].ctypes.data,
                                     out["kxy_mean"].ctypes.data, out["status"].ctypes.data, int(device), K.current_stream_ptr(device)),
            "fad_kad_individual")
    out.update(kxx_mean=res.kxx_mean, bandwidth=res.bandwidth, n=res.n)
    return out


KAD_MAX_SETS = 64


def kad_uncertainty(x, ys: Sequence, bandwidth: Optional[float] = None, device: int = 0, rows: bool = False,
                    kernel: str = "gaussian") -> dict:
    """``fad_kad_uncertainty_k``: KAD between the baseline rows x and each evaluation set ys[s] (1 <= S <= 64), one sigma for all
    (``bandwidth=None``: the median pairwise distance of x), with the first-order covariance of the S estimates -> dict of float64
    arrays ``mmd2``, ``kyy_mean``, ``kxy_mean``, ``stderr`` [S] and ``cov`` [S, S], plus ``kxx_mean``, ``bandwidth``, ``n`` and ``m``
    [S] (int64).  ``rows=True`` adds the per-row projections ``proj_x`` [S, n] (a^s_i) and ``proj_y`` (a list of [m_s] arrays, b^s_l).
    A first-order (Hoeffding-projection) estimate: meaningful for sets that differ from the baseline; for a set with the baseline's own
    distribution it understates the spread (include/fad_hip.h).  ``kernel``: "gaussian", "iq" or "imq".  x and every set are numpy
    arrays, or all torch CUDA tensors, of one dtype (float16 / bfloat16 / float32)."""
    kf = kad_kernel_code(kernel)
    ys = list(ys)
    if not 1 <= len(ys) <= KAD_MAX_SETS:
        raise ValueError(f"KAD uncertainty takes 1 .. {KAD_MAX_SETS} evaluation sets, got {len(ys)}")
    lib = K.load_library()
    views = []
    for s, y in enumerate(ys):
        vx, vy = _kad_pair(x, y, f"ys[{s}]", device)
        views.append(vy)
    px, n, d, ldx, cx, dev_x, kx = vx
    S = len(ys)
    for s, (py, m, dy, ldy, cy, dev_y, ky) in enumerate(views):
        if d != dy:
            raise ValueError(f"KAD: x has D = {d}, ys[{s}] has D = {dy}")
        if cx != cy or dev_x != dev_y:
            raise ValueError("KAD: x and every set must have the same dtype and live on the same side (host or device)")
    ptrs = (C.c_void_p * S)(*[v[0] for v in views])
    ms = np.array([v[1] for v in views], dtype=np.int64)
    lds = np.array([v[3] for v in views], dtype=np.int64)
    bw = _kad_bandwidth(bandwidth)
    res = (K.FadKadResult * S)()
    cov = np.zeros((S, S))
    proj_x = np.zeros((S, n)) if rows else None
    proj_y = np.zeros(int(ms.sum())) if rows else None
    K.check(lib.fad_kad_uncertainty_k(px, n, ldx, ptrs, ms.ctypes.data_as(C.POINTER(C.c_int64)), lds.ctypes.data_as(C.POINTER(C.c_int64)),
                                      S, d, cx, dev_x, bw, kf, res, cov.ctypes.data, proj_x.ctypes.data if rows else None,
                                      proj_y.ctypes.data if rows else None, int(device), K.current_stream_ptr(device)), "fad_kad_uncertainty")
    out = {k: np.array([getattr(r, k) for r in res]) for k in ("mmd2", "kyy_mean", "kxy_mean")}
    out.update(stderr=np.sqrt(np.diag(cov)), cov=cov, kxx_mean=res[0].kxx_mean, bandwidth=res[0].bandwidth, n=int(res[0].n),
               m=np.array([r.m for r in res], dtype=np.int64))
    if rows:
        out["proj_x"] = proj_x
        out["proj_y"] = np.split(proj_y, np.cumsum(ms)[:-1])
    return out


KAD_MAX_PERMUTATIONS = 65536


def kad_label_words(n_rows: int) -> int:
    """words of one packed labelling of N pooled rows: ceil(N / 32)"""
    return (int(n_rows) + 31) // 32


def _kad_labels(labels, N: int, device: int):
    """-> (ptr, P, on_device, keepalive) of labellings as the C ABI takes them: [P x ceil(N / 32)] uint32 words (numpy uint32 / int32,
    or a torch CUDA int32 tensor used in place), or a bool / uint8 [P x N] 0/1 matrix (numpy: packed on the host; torch: on the
    device)."""
    W = kad_label_words(N)
    if K._is_torch(labels):
        import torch
        if labels.dim() != 2:
            raise ValueError(f"KAD permutation test: labels must be 2-D, got shape {tuple(labels.shape)}")
        if labels.dtype in (torch.bool, torch.uint8):
            if labels.shape[1] != N:
                raise ValueError(f"KAD permutation test: 0/1 labels must have N = {N} columns, got {labels.shape[1]}")
            labels = pack_labels_torch(labels)
        elif labels.dtype != torch.int32 and getattr(torch, "uint32", None) != labels.dtype:
            raise ValueError(f"KAD permutation test: packed labels must be 32-bit words, got {labels.dtype}")
        if labels.shape[1] != W:
            raise ValueError(f"KAD permutation test: packed labels must have ceil(N / 32) = {W} words per row, got {labels.shape[1]}")
        if not labels.is_cuda:
            labels = labels.numpy().view(np.uint32)
        else:
            labels = labels.contiguous()
            return labels.data_ptr(), labels.shape[0], 1, labels
    a = np.asarray(labels)
    if a.ndim != 2:
        raise ValueError(f"KAD permutation test: labels must be 2-D, got shape {a.shape}")
    if a.dtype in (np.bool_, np.uint8):
        if a.shape[1] != N:
            raise ValueError(f"KAD permutation test: 0/1 labels must have N = {N} columns, got {a.shape[1]}")
        if a.dtype == np.uint8 and a.size and a.max() > 1:
            raise ValueError("KAD permutation test: uint8 labels must be 0 or 1")
        a = pack_labels(a)
    elif a.dtype in (np.uint32, np.int32):
        a = np.ascontiguousarray(a).view(np.uint32)
    else:
        raise ValueError(f"KAD permutation test: labels must be bool / uint8 [P, N] or 32-bit words [P, ceil(N / 32)], got {a.dtype}")
    if a.shape[1] != W:
        raise ValueError(f"KAD permutation test: packed labels must have ceil(N / 32) = {W} words per row, got {a.shape[1]}")
    return a.ctypes.data, a.shape[0], 0, a


def pack_labels(u) -> np.ndarray:
    """0/1 labellings [P, N] (numpy) -> packed words [P, ceil(N / 32)] uint32: bit (i & 31) of word i >> 5 is row i."""
    u = np.asarray(u).astype(bool)
    P, N = u.shape
    W = kad_label_words(N)
    pad = np.zeros((P, 32 * W), dtype=bool)
    pad[:, :N] = u
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little").view("<u4").astype(np.uint32))


def pack_labels_torch(u):
    """0/1 labellings [P, N] (torch, on their device) -> packed words [P, ceil(N / 32)] as int32 (the uint32 bits)."""
    import torch
    P, N = u.shape
    W = kad_label_words(N)
    bits = torch.zeros((P, 32 * W), dtype=torch.int64, device=u.device)
    bits[:, :N] = u.to(torch.int64)
    shifts = torch.arange(32, device=u.device, dtype=torch.int64)
    words = (bits.view(P, W, 32) << shifts).sum(dim=2)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def kad_permutation_test(x, y, labels, bandwidth: Optional[float] = None, device: int = 0, kernel: str = "gaussian") -> dict:
    """``fad_kad_permutation_test_k``: the two-sample permutation test of KAD on the pooled rows Z = [x; y] -> dict of fad_kad_result
    for the observed labelling (mmd2 = t_0, kxx_mean, kyy_mean, kxy_mean, bandwidth, n, m), ``null`` [P] (t of every labelling in
    ``labels``) and ``p_value`` = (1 + #{null >= t_0}) / (P + 1).  ``labels``: the P random labellings (each with exactly n ones over
    the N = n + m rows), packed words [P, ceil(N / 32)] (bit i & 31 of word i >> 5 is row i) or a 0/1 matrix [P, N]; the observed one
    is added by the library.  ``bandwidth=None``: the median pairwise distance of Z (exact test); a given sigma is used as is.
    ``kernel``: "gaussian", "iq" or "imq"."""
    kf = kad_kernel_code(kernel)
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"KAD: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("KAD: x and y must have the same dtype")
    pl, P, dev_l, kl = _kad_labels(labels, n + m, device)
    if not 1 <= P <= KAD_MAX_PERMUTATIONS:
        raise ValueError(f"KAD permutation test takes 1 .. {KAD_MAX_PERMUTATIONS} labellings, got {P}")
    bw = _kad_bandwidth(bandwidth)
    res = K.FadKadResult()
    null = np.zeros(P)
    pv = C.c_double()
    K.check(lib.fad_kad_permutation_test_k(px, n, ldx, py, m, ldy, d, cx, dev_x, bw, kf, pl, P, dev_l, C.byref(res), null.ctypes.data,
                                           C.byref(pv), int(device), K.current_stream_ptr(device)), "fad_kad_permutation_test")
    out = res.as_dict()
    out.update(null=null, p_value=float(pv.value))
    return out


KAD_PERM_MAX_BANDWIDTHS = 16


def _kad_perm_sweep_bandwidths(bandwidths=None, factors=None):
    """kad_sweep_bandwidths for the permutation sweep: the same list and refusals, 1 .. 16 values."""
    bw, relative = kad_sweep_bandwidths(bandwidths, factors)
    if bw.size > KAD_PERM_MAX_BANDWIDTHS:
        raise ValueError(f"KAD permutation sweep takes 1 .. {KAD_PERM_MAX_BANDWIDTHS} {'factors' if relative else 'bandwidths'}, got {bw.size}")
    return bw, relative


def kad_permutation_sweep(x, y, labels, bandwidths=None, factors=None, device: int = 0, kernel: str = "gaussian") -> dict:
    """``fad_kad_permutation_sweep``: ``kad_permutation_test`` at B bandwidths on the same labellings in one call, and the min-p
    aggregate over them -> dict of float64 arrays ``mmd2``, ``kxx_mean``, ``kyy_mean``, ``kxy_mean``, ``bandwidth``, ``p_values`` [B]
    in the order given, ``null`` [B, P], ``p_aggregated``, ``n`` and ``m``.  ``bandwidths``: the sigma values themselves; ``factors``:
    multiples of the median pairwise distance of the POOLED rows (found once; every test stays exact, and the factor 1 is
    ``kad_permutation_test``'s default sigma).  Exactly one of the two, 1 .. 16 finite values > 0.  Entry b carries the bits of
    ``kad_permutation_test(x, y, labels, bandwidth=sigma_b)``.  x, y, ``labels`` and ``kernel`` as ``kad_permutation_test`` takes
    them."""
    kf = kad_kernel_code(kernel)
    bw, relative = _kad_perm_sweep_bandwidths(bandwidths, factors)
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"KAD: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("KAD: x and y must have the same dtype")
    pl, P, dev_l, kl = _kad_labels(labels, n + m, device)
    if not 1 <= P <= KAD_MAX_PERMUTATIONS:
        raise ValueError(f"KAD permutation test takes 1 .. {KAD_MAX_PERMUTATIONS} labellings, got {P}")
    B = int(bw.size)
    res = (K.FadKadResult * B)()
    null = np.zeros((B, P))
    pv = np.zeros(B)
    pa = C.c_double()
    K.check(lib.fad_kad_permutation_sweep(px, n, ldx, py, m, ldy, d, cx, dev_x, bw.ctypes.data_as(C.POINTER(C.c_double)), B, relative, kf,
                                          pl, P, dev_l, res, null.ctypes.data, pv.ctypes.data, C.byref(pa), int(device),
                                          K.current_stream_ptr(device)), "fad_kad_permutation_sweep")
    out = {k: np.array([getattr(r, k) for r in res], dtype=np.float64) for k in ("mmd2", "kxx_mean", "kyy_mean", "kxy_mean", "bandwidth")}
    out.update(n=int(res[0].n), m=int(res[0].m), null=null, p_values=pv, p_aggregated=float(pa.value))
    return out


def kad_aggregate(t) -> dict:
    """``fad_kad_aggregate`` (host only, no GPU): the min-p aggregate of permutation statistics ``t`` [B, P + 1] (float64, column 0 the
    observed labelling) -> dict ``p_values`` [B] (p_b = #{i : t_b(i) >= t_b(0)} / (P + 1)) and ``p_aggregated`` =
    #{j : min_b p_b(j) <= min_b p_b(0)} / (P + 1), p_b(j) the same count for labelling j."""
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64))
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 2:
        raise ValueError(f"KAD aggregate: t must be [B >= 1, P + 1 >= 2], got shape {t.shape}")
    lib = K.load_library()
    pv = np.zeros(t.shape[0])
    pa = C.c_double()
    K.check(lib.fad_kad_aggregate(t.ctypes.data, int(t.shape[0]), int(t.shape[1]), pv.ctypes.data, C.byref(pa)), "fad_kad_aggregate")
    return {"p_values": pv, "p_aggregated": float(pa.value)}


# ------------------------------------------------------------------------ precision, recall, density, coverage (k-NN manifold metrics)
PRDC_MAX_K = 16


def prdc(x, y, k: int = 5, device: int = 0, details: bool = False) -> dict:
    """``fad_prdc``: precision, recall, density and coverage of the rows of y (evaluation) against the rows of x (baseline) with k
    neighbours -> dict of the four values and n, m, k.  ``details=True`` adds the per-row arrays of ``fad_prdc_detail``:
    ``radius2_x`` [n] and ``radius2_y`` [m] (float32 squared k-NN radii), ``balls_y`` [m] and ``flags_x`` [n] (int32; bit 0 recalled,
    bit 1 covered).  Both sets are numpy arrays or both torch CUDA tensors of one dtype (float16 / bfloat16 / float32)."""
    k = int(k)
    if not 1 <= k <= PRDC_MAX_K:
        raise ValueError(f"PRDC: k must be in 1 .. {PRDC_MAX_K}, got {k}")
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"PRDC: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("PRDC: x and y must have the same dtype")
    if n <= k or m <= k:
        raise ValueError(f"PRDC with k = {k} needs more than {k} rows per set, got {n} and {m}")
    res = K.FadPrdcResult()
    det, arrays = None, {}
    if details:
        arrays = {"radius2_x": np.zeros(n, np.float32), "radius2_y": np.zeros(m, np.float32), "balls_y": np.zeros(m, np.int32),
                  "flags_x": np.zeros(n, np.int32)}
        det = K.FadPrdcDetail(*(a.ctypes.data for a in arrays.values()))
    K.check(lib.fad_prdc(px, n, ldx, py, m, ldy, d, cx, dev_x, k, C.byref(res), C.byref(det) if det is not None else None, int(device),
                         K.current_stream_ptr(device)), "fad_prdc")
    out = res.as_dict()
    out.update(arrays)
    return out


# ------------------------------------------------------------------------ nearest baseline rows and authenticity (k-NN search)
def nearest(x, y, k: int = 1, authenticity: bool = True, device: int = 0) -> dict:
    """``fad_nearest``: the k nearest rows of x (baseline) to every row of y, ascending in (float32 d^2, index) -> dict of ``index``
    [m, k] (int32), ``dist2`` [m, k] (float32 squared distances), ``nn_radius2`` [m] (float32 r1^2 of each row's nearest baseline row,
    None without authenticity), ``authenticity`` (NaN without it), ``copied`` (-1 without it), ``n``, ``m`` and ``k``.  Both sets are
    numpy arrays or both torch CUDA tensors of one dtype (float16 / bfloat16 / float32)."""
    k = int(k)
    if not 1 <= k <= PRDC_MAX_K:
        raise ValueError(f"nearest: k must be in 1 .. {PRDC_MAX_K}, got {k}")
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"nearest: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("nearest: x and y must have the same dtype")
    if n < k or m < 1 or (authenticity and n < 2):
        raise ValueError(f"nearest with k = {k}{' and authenticity' if authenticity else ''} needs at least "
                         f"{max(k, 2) if authenticity else k} baseline rows and 1 evaluation row, got {n} and {m}")
    index = np.zeros((m, k), np.int32)
    dist2 = np.zeros((m, k), np.float32)
    nn_r2 = np.zeros(m, np.float32) if authenticity else None
    res = K.FadNearestResult()
    K.check(lib.fad_nearest(px, n, ldx, py, m, ldy, d, cx, dev_x, k, int(bool(authenticity)), index.ctypes.data, dist2.ctypes.data,
                            nn_r2.ctypes.data if nn_r2 is not None else None, C.byref(res), int(device), K.current_stream_ptr(device)),
            "fad_nearest")
    out = res.as_dict()
    out.update(index=index, dist2=dist2, nn_radius2=nn_r2)
    return out


# ------------------------------------------------------------------------ leave-one-out k-NN two-sample test on the pooled rows
NN_TEST_MAX_K = 15


def nn_test_k(k, n_rows: Optional[int] = None) -> int:
    """-> k as ``fad_nn_test`` takes it: odd, 1 .. 15 and at most n_rows - 1 (when the pooled row count is given); anything else is a
    ValueError, raised before the native library is touched."""
    if isinstance(k, bool) or int(k) != k:
        raise ValueError(f"nearest-neighbour test: k must be an odd integer in 1 .. {NN_TEST_MAX_K}, got {k!r}")
    k = int(k)
    if not 1 <= k <= NN_TEST_MAX_K or k % 2 == 0:
        raise ValueError(f"nearest-neighbour test: k must be odd and in 1 .. {NN_TEST_MAX_K}, got {k}")
    if n_rows is not None and k > n_rows - 1:
        raise ValueError(f"nearest-neighbour test: k = {k} needs at least {k + 1} pooled rows, got {n_rows}")
    return k


def nn_test(x, y, labels, k: int = 1, device: int = 0, return_graph: bool = False) -> dict:
    """``fad_nn_test``: the leave-one-out k-nearest-neighbour two-sample test on the pooled rows Z = [x; y] -> dict of
    fad_nn_test_result (accuracy, accuracy_x, accuracy_y, p_value, p_value_low, correct_x, correct_y, n, m, k) and
    ``null_correct_x`` / ``null_correct_y`` [P] (int64, the correct baseline-labelled / evaluation-labelled rows under every labelling
    of ``labels``).  ``labels`` as ``kad_permutation_test`` takes them; the observed labelling is added by the library.  k is odd,
    1 .. 15, at most n + m - 1.  ``return_graph=True`` adds ``index`` [N, k] (int32, Z's row numbering) and ``dist2`` [N, k] (float32),
    every pooled row's k nearest OTHER pooled rows in ascending (d^2, index): numpy arrays for numpy rows, torch tensors on the rows'
    device for torch CUDA rows."""
    k = nn_test_k(k)
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"nearest-neighbour test: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("nearest-neighbour test: x and y must have the same dtype")
    nn_test_k(k, n + m)
    pl, P, dev_l, kl = _kad_labels(labels, n + m, device)
    if not 1 <= P <= KAD_MAX_PERMUTATIONS:
        raise ValueError(f"nearest-neighbour test takes 1 .. {KAD_MAX_PERMUTATIONS} labellings, got {P}")
    res = K.FadNnTestResult()
    null_x = np.zeros(P, np.int64)
    null_y = np.zeros(P, np.int64)
    index = dist2 = None
    pi = pd = None
    if return_graph:
        if dev_x:
            import torch
            index = torch.zeros((n + m, k), dtype=torch.int32, device=kx.device)
            dist2 = torch.zeros((n + m, k), dtype=torch.float32, device=kx.device)
            pi, pd = index.data_ptr(), dist2.data_ptr()
        else:
            index = np.zeros((n + m, k), np.int32)
            dist2 = np.zeros((n + m, k), np.float32)
            pi, pd = index.ctypes.data, dist2.ctypes.data
    K.check(lib.fad_nn_test(px, n, ldx, py, m, ldy, d, cx, dev_x, k, pl, P, dev_l, C.byref(res), null_x.ctypes.data, null_y.ctypes.data,
                            pi, pd, int(device), K.current_stream_ptr(device)), "fad_nn_test")
    out = res.as_dict()
    out.update(null_correct_x=null_x, null_correct_y=null_y)
    if return_graph:
        out.update(index=index, dist2=dist2)
    return out


# ------------------------------------------------------------------------ kernel distance with the polynomial kernel (KID)
def kid_params(degree=3, gamma=None, coef0=1.0):
    """-> (degree, gamma, coef0) as the C ABI takes them: degree 1 .. 4, gamma None -> 0 (the library's 1 / D) else a finite value > 0,
    coef0 finite.  Anything else is a ValueError, raised before the native library is touched."""
    if int(degree) != degree or not 1 <= int(degree) <= 4:
        raise ValueError(f"KID: degree must be 1 .. 4, got {degree}")
    g = 0.0 if gamma is None else float(gamma)
    if gamma is not None and not (g > 0 and np.isfinite(g)):
        raise ValueError(f"KID: gamma must be finite and > 0 (None: 1 / D), got {gamma}")
    c = float(coef0)
    if not np.isfinite(c):
        raise ValueError(f"KID: coef0 must be finite, got {coef0}")
    return int(degree), g, c


def _kid_pair(x, y, device: int):
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"KID: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("KID: x and y must have the same dtype")
    return (px, n, ldx, kx), (py, m, ldy, ky), d, cx, dev_x


def kid(x, y, degree: int = 3, gamma: Optional[float] = None, coef0: float = 1.0, device: int = 0) -> dict:
    """``fad_kid``: the unbiased MMD^2 with the polynomial kernel (gamma a.b + coef0)^degree over all rows of x and y -> dict of
    fad_kid_result (mmd2, kxx_mean, kyy_mean, kxy_mean, gamma and coef0 as used, degree, n, m).  ``gamma=None``: 1 / D.
    Both sets are numpy arrays or both torch CUDA tensors of one dtype (float16 / bfloat16 / float32)."""
    degree, g, c = kid_params(degree, gamma, coef0)
    lib = K.load_library()
    (px, n, ldx, kx), (py, m, ldy, ky), d, code, on_dev = _kid_pair(x, y, device)
    res = K.FadKidResult()
    K.check(lib.fad_kid(px, n, ldx, py, m, ldy, d, code, on_dev, degree, g, c, C.byref(res), int(device), K.current_stream_ptr(device)), "fad_kid")
    return res.as_dict()


def _kid_index(index, what: str, device: int):
    """-> (int32 [S, s] numpy array or contiguous torch CUDA tensor, on_device)"""
    if K._is_torch(index):
        import torch
        if index.dim() != 2:
            raise ValueError(f"KID: {what} must be 2-D [subsets, subset_size], got shape {tuple(index.shape)}")
        if index.is_cuda:
            return index.to(torch.int32).contiguous(), 1
        index = index.numpy()
    a = np.asarray(index)
    if a.ndim != 2:
        raise ValueError(f"KID: {what} must be 2-D [subsets, subset_size], got shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise ValueError(f"KID: {what} must hold integers, got {a.dtype}")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f"KID: {what} does not fit 32 bits")
    return np.ascontiguousarray(a, dtype=np.int32), 0


def kid_subsets(x, y, index_x, index_y, degree: int = 3, gamma: Optional[float] = None, coef0: float = 1.0, device: int = 0) -> dict:
    """``fad_kid_subsets``: the KID protocol, every subset in one fused pass.  ``index_x`` / ``index_y``: integer [S, s] row numbers of
    x / of y, subset q being x[index_x[q]] against y[index_y[q]] (both numpy, or both torch CUDA tensors used in place as int32).
    -> dict: ``mmd2`` [S] and ``terms`` [S, 3] (kxx, kyy, kxy means) as float64 numpy arrays, ``mean`` and ``std`` (population) of
    mmd2, ``subsets``, ``subset_size``."""
    degree, g, c = kid_params(degree, gamma, coef0)
    ix, dev_i = _kid_index(index_x, "index_x", device)
    iy, dev_j = _kid_index(index_y, "index_y", device)
    if tuple(ix.shape) != tuple(iy.shape):
        raise ValueError(f"KID: index_x {tuple(ix.shape)} and index_y {tuple(iy.shape)} must have one shape")
    if dev_i != dev_j:
        raise ValueError("KID: index_x and index_y must both be numpy arrays or both torch CUDA tensors")
    S, s = int(ix.shape[0]), int(ix.shape[1])
    lib = K.load_library()
    (px, n, ldx, kx), (py, m, ldy, ky), d, code, on_dev = _kid_pair(x, y, device)
    mmd2, terms = np.zeros(max(S, 1)), np.zeros((max(S, 1), 3))
    mean, std = C.c_double(), C.c_double()
    pix, piy = (ix.data_ptr(), iy.data_ptr()) if dev_i else (ix.ctypes.data, iy.ctypes.data)
    K.check(lib.fad_kid_subsets(px, n, ldx, py, m, ldy, d, code, on_dev, degree, g, c, pix, piy, S, s, dev_i, mmd2.ctypes.data,
                                terms.ctypes.data, C.byref(mean), C.byref(std), int(device), K.current_stream_ptr(device)), "fad_kid_subsets")
    return {"mmd2": mmd2[:S], "terms": terms[:S], "mean": float(mean.value), "std": float(std.value), "subsets": S, "subset_size": s}


# ------------------------------------------------------------------------ Sinkhorn divergence between the two sets of rows
SINKHORN_MAX_ITERATIONS = 100000


def sinkhorn_params(epsilon=None, iterations=100):
    """-> (epsilon, iterations) as the C ABI takes them: epsilon None -> 0 (the library's default from x's median distance) else a finite
    value > 0, iterations an integer in 1 .. 100000.  Anything else is a ValueError, raised before the native library is touched."""
    e = 0.0 if epsilon is None else float(epsilon)
    if epsilon is not None and not (e > 0 and np.isfinite(e)):
        raise ValueError(f"Sinkhorn: epsilon must be finite and > 0 (None: from the median distance of x), got {epsilon}")
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= int(iterations) <= SINKHORN_MAX_ITERATIONS:
        raise ValueError(f"Sinkhorn: iterations must be an integer in 1 .. {SINKHORN_MAX_ITERATIONS}, got {iterations!r}")
    return e, int(iterations)


def sinkhorn(x, y, epsilon: Optional[float] = None, iterations: int = 100, device: int = 0, potentials: bool = False) -> dict:
    """``fad_sinkhorn``: the debiased Sinkhorn divergence between the rows of x (baseline) and y with the cost |a - b|^2 / 2 -> dict of
    fad_sinkhorn_result (divergence, ot_xy, ot_xx, ot_yy, epsilon as used, marginal_error, marginal_error_xx, marginal_error_yy, n, m,
    iterations).  ``epsilon=None``: (0.25 x the median pairwise distance of x)^2.  ``potentials=True`` adds the float64 arrays ``f`` [n]
    and ``g`` [m] (the dual potentials of the x-y problem) and ``pot_x`` [n], ``pot_y`` [m] (the debiased ones: divergence =
    mean(pot_x) + mean(pot_y)).  Both sets are numpy arrays or both torch CUDA tensors of one dtype (float16 / bfloat16 / float32)."""
    e, iterations = sinkhorn_params(epsilon, iterations)
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _kad_pair(x, y, "y", device)
    if d != dy:
        raise ValueError(f"Sinkhorn: x has D = {d}, y has D = {dy}")
    if cx != cy:
        raise ValueError("Sinkhorn: x and y must have the same dtype")
    res = K.FadSinkhornResult()
    det, arrays = None, {}
    if potentials:
        arrays = {"f": np.zeros(n), "g": np.zeros(m), "pot_x": np.zeros(n), "pot_y": np.zeros(m)}
        det = K.FadSinkhornDetail(*(a.ctypes.data for a in arrays.values()))
    K.check(lib.fad_sinkhorn(px, n, ldx, py, m, ldy, d, cx, dev_x, e, iterations, C.byref(res), C.byref(det) if det is not None else None,
                             int(device), K.current_stream_ptr(device)), "fad_sinkhorn")
    out = res.as_dict()
    out.update(arrays)
    return out


# ------------------------------------------------------------------------ sliced Wasserstein distance between the two sets of rows
SLICED_MAX_PROJECTIONS = 65536


def sliced_directions_array(directions, d: int) -> np.ndarray:
    """-> ``directions`` as the C ABI takes them: a C-contiguous float32 [L x d] array, L in 1 .. 65536, every entry finite.  Anything
    else is a ValueError, raised before the native library is touched."""
    t = np.ascontiguousarray(np.asarray(directions), dtype=np.float32)
    if t.ndim != 2 or t.shape[1] != d:
        raise ValueError(f"sliced Wasserstein: directions must be [L x {d}], got shape {t.shape}")
    if not 1 <= t.shape[0] <= SLICED_MAX_PROJECTIONS:
        raise ValueError(f"sliced Wasserstein: {t.shape[0]} directions, outside 1 .. {SLICED_MAX_PROJECTIONS}")
    if not np.all(np.isfinite(t)):
        raise ValueError("sliced Wasserstein: a direction has an entry that is not finite")
    return t


def _sliced_rows(x, y, what: str, device: int):
    """-> (rows_view of x, rows_view of y) for the sliced entries: ``_kad_pair``, then one D and one dtype.  ``what`` names y in the
    messages: "y", or "rows" for the songs of ``sliced_individual``, which are checked only where there are any."""
    vx, vy = _kad_pair(x, y, what, device)
    has, other = ("the songs have", "the songs") if what == "rows" else ("y has", "y")
    if what != "rows" or vy[1] > 0:
        if vx[2] != vy[2]:
            raise ValueError(f"sliced Wasserstein: x has D = {vx[2]}, {has} D = {vy[2]}")
        if vx[4] != vy[4]:
            raise ValueError(f"sliced Wasserstein: x and {other} must have the same dtype")
    return vx, vy


def _sliced_detail(struct, arrays: dict):
    """-> byref of the detail ``struct`` with the address of every array asked for (its fields' names are the keys), NULL without any"""
    if not arrays:
        return None
    return C.byref(struct(*(arrays[k].ctypes.data if k in arrays else None for k, _ in struct._fields_)))


def _sliced_pair_call(entry: str, struct, x, y, directions, device: int, values: bool, sorted_projections: bool, indices: bool,
                      shares: bool) -> dict:
    """``fad_sliced_wasserstein`` / ``fad_sliced_shares`` (``entry``, with its detail ``struct``): the rows, the directions, the arrays
    asked for, the call -> dict of fad_sliced_result and those arrays."""
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _sliced_rows(x, y, "y", device)
    t = sliced_directions_array(directions, d)
    L = t.shape[0]
    res = K.FadSlicedResult()
    out = {"share_x": np.zeros(max(n, 0)), "share_y": np.zeros(max(m, 0))} if shares else {}
    arrays = {}
    if values:
        arrays["values"] = np.zeros(L)
    for on, stem, dtype in ((sorted_projections, "sorted", np.float32), (indices, "index", np.int32)):
        if on:
            arrays[stem + "_x"] = np.zeros((L, n), dtype=dtype)
            arrays[stem + "_y"] = np.zeros((L, m), dtype=dtype)
    K.check(getattr(lib, entry)(px, n, ldx, py, m, ldy, d, cx, dev_x, t.ctypes.data, L, C.byref(res), *(a.ctypes.data for a in out.values()),
                                _sliced_detail(struct, arrays), int(device), K.current_stream_ptr(device)), entry)
    return {**res.as_dict(), **arrays, **out}


def sliced_wasserstein(x, y, directions, device: int = 0, values: bool = False, sorted_projections: bool = False) -> dict:
    """``fad_sliced_wasserstein``: the sliced 2-Wasserstein distance between the rows of x (baseline) and y over the float32 directions
    [L x D] (not normalised: the library divides by their squared lengths) -> dict of fad_sliced_result (sw2_squared, std_error,
    max_sliced, max_index, n, m, projections).  ``values=True`` adds the float64 array ``values`` [L] (W_l); ``sorted_projections=True``
    adds the float32 arrays ``sorted_x`` [L x n] and ``sorted_y`` [L x m].  Both sets are numpy arrays or both torch CUDA tensors of
    one dtype (float16 / bfloat16 / float32)."""
    return _sliced_pair_call("fad_sliced_wasserstein", K.FadSlicedDetail, x, y, directions, device, values, sorted_projections, False, False)


def sliced_shares(x, y, directions, device: int = 0, values: bool = False, sorted_projections: bool = False, indices: bool = False) -> dict:
    """``fad_sliced_shares``: ``sliced_wasserstein`` (the same result fields, bit for bit) plus every row's share of ``sw2_squared`` ->
    that dict with the float64 arrays ``share_x`` [n] and ``share_y`` [m], each summing to ``sw2_squared`` up to rounding.  ``values``
    and ``sorted_projections`` as there; ``indices=True`` adds the int32 arrays ``index_x`` [L x n] and ``index_y`` [L x m]: the row at
    every rank of every direction (equal projections in ascending row order)."""
    return _sliced_pair_call("fad_sliced_shares", K.FadSlicedSharesDetail, x, y, directions, device, values, sorted_projections, indices, True)


def sliced_last_plan() -> dict:
    """``fad_sliced_last_plan``: how this thread's last fad_sliced_wasserstein or fad_sliced_shares call was laid out -> dict of ``chunks``,
    ``directions_per_chunk``, ``sort_passes`` and ``share`` (W >= 1: workgroups per segment of x's sort; -G: one workgroup owns G
    segments)."""
    out = (C.c_int64 * 4)()
    K.check(K.load_library().fad_sliced_last_plan(out), "fad_sliced_last_plan")
    return dict(zip(("chunks", "directions_per_chunk", "sort_passes", "share"), map(int, out)))


def sliced_individual(x, rows, offsets: Sequence[int], directions, device: int = 0, values: bool = False, sorted: bool = False) -> dict:
    """``fad_sliced_individual``: the sliced 2-Wasserstein distance between the baseline rows x and every song s =
    rows[offsets[s]:offsets[s + 1]] over the float32 directions [L x D], bit for bit what ``sliced_wasserstein(x, song_s, directions)``
    gives -> dict of float64 arrays ``sw2_squared``, ``std_error``, ``max_sliced``, int64 ``max_index`` and int32 ``status`` [S] (NaN
    and -1 where status is FAD_ERR_TOO_FEW_ROWS or FAD_ERR_NOT_FINITE), plus ``n`` and ``projections``.  ``values=True`` adds the
    float64 array ``values`` [S x L]; ``sorted=True`` adds the float32 arrays ``sorted_x`` [L x n] and ``sorted_rows`` [L x n_rows]
    (every song's range sorted on its own).  x and rows are both numpy arrays or both torch CUDA tensors of one dtype (float16 /
    bfloat16 / float32)."""
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _sliced_rows(x, rows, "rows", device)
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if off.ndim != 1 or off.shape[0] < 2:
        raise ValueError("sliced Wasserstein: offsets must be a 1-D sequence of S + 1 row indices, S >= 1")
    S = off.shape[0] - 1
    t = sliced_directions_array(directions, d)
    L = t.shape[0]
    out = {k: np.full(S, np.nan) for k in ("sw2_squared", "std_error", "max_sliced")}
    out["max_index"] = np.full(S, -1, dtype=np.int64)
    out["status"] = np.zeros(S, dtype=np.int32)
    arrays = {}
    if values:
        arrays["values"] = np.full((S, L), np.nan)
    if sorted:
        arrays["sorted_x"] = np.zeros((L, n), dtype=np.float32)
        arrays["sorted_rows"] = np.zeros((L, m), dtype=np.float32)
    K.check(lib.fad_sliced_individual(px, n, ldx, py if m > 0 else None, m, max(ldy, d), off.ctypes.data_as(C.POINTER(C.c_int64)), S, d,
                                      cx, dev_x, t.ctypes.data, L, out["sw2_squared"].ctypes.data, out["std_error"].ctypes.data,
                                      out["max_sliced"].ctypes.data, out["max_index"].ctypes.data, out["status"].ctypes.data,
                                      _sliced_detail(K.FadSlicedIndividualDetail, arrays), int(device), K.current_stream_ptr(device)),
            "fad_sliced_individual")
    out.update(arrays)
    out.update(n=n, projections=L)
    return out


def sliced_individual_last_plan() -> dict:
    """``fad_sliced_individual_last_plan``: how this thread's last fad_sliced_individual call was laid out -> dict of ``chunks``,
    ``directions_per_chunk``, ``units`` (resident units per direction), ``long_songs`` (songs beyond the resident capacity, on the
    global sort), ``most_songs`` (in one unit) and ``capacity`` (C, keys a unit holds at most)."""
    out = (C.c_int64 * 6)()
    K.check(K.load_library().fad_sliced_individual_last_plan(out), "fad_sliced_individual_last_plan")
    return dict(zip(("chunks", "directions_per_chunk", "units", "long_songs", "most_songs", "capacity"), map(int, out)))


# ------------------------------------------------------------------------ sliced Wasserstein two-sample permutation test
def sliced_permutation_test(x, y, labels, directions, device: int = 0, per_labelling: bool = False, stages: bool = False) -> dict:
    """``fad_sliced_permutation_test``: the two-sample permutation test with the sliced 2-Wasserstein distance as its statistic, on the
    pooled rows Z = [x; y] -> dict of fad_sliced_result for the observed labelling (bit for bit ``sliced_wasserstein(x, y, directions)``),
    ``null`` and ``null_max`` [P] (the mean and the maximum over the directions under every labelling of ``labels``), ``p_value`` =
    (1 + #{null >= sw2_squared}) / (P + 1), ``p_value_max`` the same with the maxima, and ``permutations`` = P.  ``labels`` as
    ``kad_permutation_test`` takes them; the observed labelling is added by the library.  ``per_labelling=True`` adds the float64 array
    ``values`` [P + 1, L] (row 0 the observed labelling); ``stages=True`` adds ``sorted_z`` (float32) and ``index_z`` (int32) [L x N]: the
    sorted pooled projections and the pooled row at every rank."""
    lib = K.load_library()
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _sliced_rows(x, y, "y", device)
    t = sliced_directions_array(directions, d)
    L = t.shape[0]
    pl, P, dev_l, kl = _kad_labels(labels, n + m, device)
    if not 1 <= P <= KAD_MAX_PERMUTATIONS:
        raise ValueError(f"sliced Wasserstein permutation test takes 1 .. {KAD_MAX_PERMUTATIONS} labellings, got {P}")
    res = K.FadSlicedPermutationResult()
    null = np.zeros(P)
    null_max = np.zeros(P)
    arrays = {}
    if per_labelling:
        arrays["values"] = np.zeros((P + 1, L))
    if stages:
        arrays["sorted_z"] = np.zeros((L, n + m), dtype=np.float32)
        arrays["index_z"] = np.zeros((L, n + m), dtype=np.int32)
    K.check(lib.fad_sliced_permutation_test(px, n, ldx, py, m, ldy, d, cx, dev_x, t.ctypes.data, L, pl, P, dev_l, C.byref(res),
                                            null.ctypes.data, null_max.ctypes.data, _sliced_detail(K.FadSlicedPermutationDetail, arrays),
                                            int(device), K.current_stream_ptr(device)), "fad_sliced_permutation_test")
    return {**res.as_dict(), "null": null, "null_max": null_max, **arrays}


def sliced_permutation_last_plan() -> dict:
    """``fad_sliced_permutation_last_plan``: how this thread's last fad_sliced_permutation_test call was laid out -> dict of
    ``sort_chunks``, ``directions_per_sort_chunk``, ``rounds`` (pair rounds in all), ``directions_per_round``, ``words_per_round``
    (labelling words of 32) and ``share`` (as ``sliced_last_plan``, of the pooled rows)."""
    out = (C.c_int64 * 6)()
    K.check(K.load_library().fad_sliced_permutation_last_plan(out), "fad_sliced_permutation_last_plan")
    return dict(zip(("sort_chunks", "directions_per_sort_chunk", "rounds", "directions_per_round", "words_per_round", "share"), map(int, out)))


# ------------------------------------------------------------------------ sliced Wasserstein bootstrap
SLICED_MAX_REPLICATES = 65536


def sliced_bootstrap_counts_array(counts, rows: int, name: str) -> np.ndarray:
    """-> ``counts`` as the C ABI takes them: a C-contiguous uint8 [B x rows] array, B in 1 .. 65536.  Anything else is a ValueError,
    raised before the native library is touched."""
    if not isinstance(counts, np.ndarray) or counts.dtype != np.uint8 or counts.ndim != 2 or counts.shape[1] != rows:
        raise ValueError(f"sliced Wasserstein bootstrap: {name} must be a uint8 array [B x {rows}], got "
                         f"{getattr(counts, 'dtype', type(counts).__name__)} {getattr(counts, 'shape', '')}")
    if not 1 <= counts.shape[0] <= SLICED_MAX_REPLICATES:
        raise ValueError(f"sliced Wasserstein bootstrap takes 1 .. {SLICED_MAX_REPLICATES} replicates, got {counts.shape[0]}")
    return np.ascontiguousarray(counts)


def sliced_bootstrap(x, y, counts_x, counts_y, directions, device: int = 0, per_replicate: bool = False, stages: bool = False) -> dict:
    """``fad_sliced_bootstrap``: the sliced 2-Wasserstein distance on B resamples of both sets, each given as uint8 row counts
    (``counts_x`` [B x n], ``counts_y`` [B x m]) -> dict of fad_sliced_result for the sets as given (bit for bit
    ``sliced_wasserstein(x, y, directions)``), ``boot`` and ``boot_max`` [B] (the mean and the maximum over the directions on every
    resample, bit for bit ``sliced_wasserstein(np.repeat(x, counts_x[b], 0), np.repeat(y, counts_y[b], 0), directions)``) and
    ``replicates`` = B.  ``per_replicate=True`` adds the float64 array ``values`` [B + 1, L] (row 0 the sets as given) and the int64
    array ``totals`` [B + 1, 2] (the rows of x and of y every replicate takes); ``stages=True`` adds ``sorted_x``, ``sorted_y`` (float32)
    and ``index_x``, ``index_y`` (int32) as ``sliced_shares`` gives them."""
    (px, n, d, ldx, cx, dev_x, kx), (py, m, dy, ldy, cy, dev_y, ky) = _sliced_rows(x, y, "y", device)
    t = sliced_directions_array(directions, d)
    L = t.shape[0]
    ca = sliced_bootstrap_counts_array(counts_x, n, "counts_x")
    cb = sliced_bootstrap_counts_array(counts_y, m, "counts_y")
    B = ca.shape[0]
    if cb.shape[0] != B:
        raise ValueError(f"sliced Wasserstein bootstrap: counts_x has {B} replicates, counts_y has {cb.shape[0]}")
    lib = K.load_library()
    res = K.FadSlicedBootstrapResult()
    boot = np.zeros(B)
    boot_max = np.zeros(B)
    arrays = {}
    if per_replicate:
        arrays["values"] = np.zeros((B + 1, L))
        arrays["totals"] = np.zeros((B + 1, 2), dtype=np.int64)
    if stages:
        arrays["sorted_x"] = np.zeros((L, n), dtype=np.float32)
        arrays["index_x"] = np.zeros((L, n), dtype=np.int32)
        arrays["sorted_y"] = np.zeros((L, m), dtype=np.float32)
        arrays["index_y"] = np.zeros((L, m), dtype=np.int32)
    K.check(lib.fad_sliced_bootstrap(px, n, ldx, py, m, ldy, d, cx, dev_x, t.ctypes.data, L, ca.ctypes.data, cb.ctypes.data, B, C.byref(res),
                                     boot.ctypes.data, boot_max.ctypes.data, _sliced_detail(K.FadSlicedBootstrapDetail, arrays),
                                     int(device), K.current_stream_ptr(device)), "fad_sliced_bootstrap")
    return {**res.as_dict(), "boot": boot, "boot_max": boot_max, **arrays}


def sliced_bootstrap_last_plan() -> dict:
    """``fad_sliced_bootstrap_last_plan``: how this thread's last fad_sliced_bootstrap call was laid out -> dict of ``sort_chunks``,
    ``directions_per_sort_chunk``, ``rounds`` (rounds in all), ``directions_per_round``, ``words_per_round`` (replicate words) and
    ``replicates_per_word``."""
    out = (C.c_int64 * 6)()
    K.check(K.load_library().fad_sliced_bootstrap_last_plan(out), "fad_sliced_bootstrap_last_plan")
    return dict(zip(("sort_chunks", "directions_per_sort_chunk", "rounds", "directions_per_round", "words_per_round", "replicates_per_word"),
                    map(int, out)))


# ------------------------------------------------------------------------ Lloyd's k-means on the pooled rows (MAUVE, PRD curves)
KMEANS_MAX_CLUSTERS = 65536
KMEANS_MAX_SETS = 8


def kmeans_args(clusters, iterations, n_rows: Optional[int] = None):
    """-> (K, max_iter) as ``fad_kmeans`` takes them: K an integer in 1 .. min(n_rows, 65 536) (when the pooled row count is given),
    max_iter an integer >= 0.  Anything else is a ValueError, raised before the native library is touched."""
    for name, v in (("clusters", clusters), ("iterations", iterations)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"k-means: {name} must be an integer, got {v!r}")
    k, it = int(clusters), int(iterations)
    if not 1 <= k <= KMEANS_MAX_CLUSTERS:
        raise ValueError(f"k-means: clusters must be in 1 .. {KMEANS_MAX_CLUSTERS}, got {k}")
    if n_rows is not None and k > n_rows:
        raise ValueError(f"k-means: clusters = {k} needs at least {k} pooled rows, got {n_rows}")
    if not 0 <= it <= 2 ** 31 - 2:
        raise ValueError(f"k-means: iterations must be >= 0, got {it}")
    return k, it


def kmeans(sets, init, iterations: int = 100, device: int = 0, return_dist2: bool = True) -> dict:
    """``fad_kmeans``: Lloyd's k-means on the pooled rows of ``sets`` (one frame matrix or a list of 1 .. 8 of them, pooled in the
    given order without a copy; numpy arrays or torch tensors of one dtype, float16 / bfloat16 / float32, all on the host or all on
    the device) from the centroids ``init`` [K, D] (float32) -> dict of ``centroids`` [K, D] float32, ``labels`` [N] int32,
    ``counts`` [K] int64, ``dist2`` [N] float32 (``return_dist2``), ``inertia_trace`` (float64, one value per assignment made) and
    fad_kmeans_result (inertia, n, k, iterations, converged, changed_last, empty_clusters, assignments).  ``iterations=0`` is a pure
    assignment of the rows to ``init``.  The rule is fully determined (include/fad_hip.h): the same bits on every run."""
    if K._is_torch(sets) or isinstance(sets, np.ndarray):
        sets = [sets]
    sets = list(sets)
    if not 1 <= len(sets) <= KMEANS_MAX_SETS:
        raise ValueError(f"k-means takes 1 .. {KMEANS_MAX_SETS} row sets, got {len(sets)}")
    init = np.ascontiguousarray(np.asarray(init, dtype=np.float32))
    if init.ndim != 2:
        raise ValueError(f"k-means: init must be [K, D], got shape {init.shape}")
    k, max_iter = kmeans_args(init.shape[0], iterations)
    views = []
    for s, x in enumerate(sets):
        if K._is_torch(x):
            import torch
            ok = x.dtype in (torch.float16, torch.bfloat16, torch.float32)
        else:
            x = np.asarray(x)
            ok = x.dtype in (np.float16, np.float32)
        if not ok:
            raise ValueError(f"k-means takes float16, bfloat16 or float32 rows; set {s} is {x.dtype}")
        views.append(K.rows_view(x, host_bf16=True))
    d, code, dev = views[0][2], views[0][4], views[0][5]
    for s, v in enumerate(views):
        if v[2] != d:
            raise ValueError(f"k-means: set 0 has D = {d}, set {s} has D = {v[2]}")
        if v[4] != code or v[5] != dev:
            raise ValueError("k-means: every set must have the same dtype and live on the same side (host or device)")
        if v[1] < 1:
            raise ValueError(f"k-means: set {s} has no rows")
    if init.shape[1] != d:
        raise ValueError(f"k-means: init has D = {init.shape[1]}, the rows have D = {d}")
    N = sum(v[1] for v in views)
    kmeans_args(k, max_iter, N)
    if not np.isfinite(init).all():
        raise ValueError("k-means: init has a NaN/Inf entry")
    lib = K.load_library()
    S = len(views)
    ptrs = (C.c_void_p * S)(*[v[0] for v in views])
    ns = np.array([v[1] for v in views], dtype=np.int64)
    lds = np.array([v[3] for v in views], dtype=np.int64)
    centroids = np.zeros((k, d), np.float32)
    labels = np.zeros(N, np.int32)
    counts = np.zeros(k, np.int64)
    dist2 = np.zeros(N, np.float32) if return_dist2 else None
    trace = np.zeros(max_iter + 1, np.float64)
    res = K.FadKmeansResult()
    K.check(lib.fad_kmeans(ptrs, ns.ctypes.data_as(C.POINTER(C.c_int64)), lds.ctypes.data_as(C.POINTER(C.c_int64)), S, d, code, dev, k,
                           init.ctypes.data, max_iter, centroids.ctypes.data, labels.ctypes.data, counts.ctypes.data,
                           dist2.ctypes.data if return_dist2 else None, trace.ctypes.data, C.byref(res), int(device),
                           K.current_stream_ptr(device)), "fad_kmeans")
    out = res.as_dict()
    out.update(centroids=centroids, labels=labels, counts=counts, inertia_trace=trace[:out["assignments"]].copy())
    if return_dist2:
        out["dist2"] = dist2
    return out


def kmeans_last_plan() -> dict:
    """``fad_kmeans_last_plan``: how this thread's last fad_kmeans call ran -> dict of ``planes`` (of the centroid operand),
    ``assign_launches`` (of the last assignment), ``chunk_rows`` (rows per update chunk), ``max_chunks`` (most chunks one cluster took
    in the last update), ``iterations`` and ``assignments``."""
    out = (C.c_int64 * 6)()
    K.check(K.load_library().fad_kmeans_last_plan(out), "fad_kmeans_last_plan")
    return dict(zip(("planes", "assign_launches", "chunk_rows", "max_chunks", "iterations", "assignments"), map(int, out)))
