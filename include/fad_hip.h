/*
 * fad_hip.h -- C ABI of libfad_hip.so, the MI355X (gfx950) implementation of the FAD hot path.
 *
 * The reference (microsoft/fadtk v1.1.0) is pure Python and has no FFI for this path; each
 * entry point below replaces the numpy/scipy call(s) cited next to it (paths relative to the
 * reference root).  A maintainer binds these with ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns FAD_OK (0) or a negative fad_status; nothing throws across the ABI;
 *     fad_last_error() gives a thread-local message for the last failure on the calling thread.
 *   - `on_device` != 0 means the data pointers are device (HBM) pointers on the handle's GPU;
 *     0 means host pointers (the library stages them over PCIe itself).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Work is enqueued on
 *     that stream; functions that return results to HOST memory synchronise it before returning.
 *   - row-major everywhere; `ld` is the row pitch in ELEMENTS.
 *   - distinct handles are independent; handle-less functions are re-entrant; one handle must not
 *     be used from two threads at once.
 *   - there is NO CPU fallback: without a usable GPU every compute entry returns
 *     FAD_ERR_NO_DEVICE.
 */
#ifndef FAD_HIP_H
#define FAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAD_ABI_VERSION 2

typedef enum fad_status {
    FAD_OK = 0,
    FAD_ERR_INVALID = -1,       /* bad argument (NULL, negative size, unknown dtype ...)        */
    FAD_ERR_NO_DEVICE = -2,     /* no HIP device / wrong architecture                            */
    FAD_ERR_HIP = -3,           /* a HIP runtime call failed (message has the hipError string)   */
    FAD_ERR_ALLOC = -4,         /* device or host allocation failed                              */
    FAD_ERR_SHAPE = -5,         /* dimension mismatch (fad.py:78-81 AssertionError)              */
    FAD_ERR_TOO_FEW_ROWS = -6,  /* N < 2 frames (fad.py:46-47 AssertionError)                    */
    FAD_ERR_NOT_FINITE = -7,    /* NaN/Inf in the inputs or a diverged root (fad.py:102-106 ValueError) */
    FAD_ERR_NOT_CONVERGED = -8  /* iteration hit max_iter (result still written; see fad_diag_t) */
} fad_status;

typedef enum fad_dtype { FAD_F16 = 0, FAD_BF16 = 1, FAD_F32 = 2, FAD_F64 = 3 } fad_dtype;

/* ------------------------------------------------------------------ library / device */
int fad_version(void);                       /* FAD_ABI_VERSION                                   */
int fad_device_count(void);                  /* number of gfx950 devices visible (0 if none)      */
const char* fad_last_error(void);            /* thread-local, never NULL                          */
const char* fad_device_arch(int device);     /* e.g. "gfx950:sramecc+:xnack-"; "" on failure      */

/* ------------------------------------------------------------------ running moments
 * Replaces calc_embd_statistics (fadtk/fad.py:42-48), _process_file (fadtk/utils.py:13-16) and
 * the merge loop of calculate_embd_statistics_online (fadtk/utils.py:36-45).
 *
 * A handle accumulates the sufficient statistics (n, sum x, sum x x^T) of all rows fed so far,
 * in float64 in HBM, packed as [n | sum_x (D) | sum_xxT (D*D, row-major, symmetric)] =
 * 1 + D + D*D doubles.  Raw moments are sum-reducible, so merging datasets or GPUs is an
 * element-wise add of packed buffers (one RCCL all-reduce across ranks).
 */
typedef struct fad_moments fad_moments_t;

int fad_moments_create(int d, int device, fad_moments_t** out);
int fad_moments_destroy(fad_moments_t* h);
int fad_moments_reset(fad_moments_t* h, void* stream);
/* fad_moments_reset for `count` handles in one call (a scoring loop that re-feeds the accumulators of sixteen scores: one call into
 * the library instead of thirty-two). */
int fad_moments_reset_multi(int count, fad_moments_t* const* hs, void* stream);
/* The zeroing of a reset (or bind) is deferred: an update right after it overwrites the accumulator instead.  Whoever
 * reads the packed buffer BEHIND the library's back (a collective over a bound buffer) calls this first so that a
 * handle that received no rows holds zeros. */
int fad_moments_settle(fad_moments_t* h, void* stream);
/* Keep the packed statistics in the CALLER's device buffer (packed_len doubles, 16-byte aligned, same device) from
 * now on, and reset them.  The buffer then is what a collective runs over in place -- e.g. two handles bound to the
 * halves of one allocation are summed across ranks by a single all-reduce with no export/import copies (bench.py).
 * The caller keeps ownership and must outlive the handle or re-bind. */
int fad_moments_bind(fad_moments_t* h, double* device_packed);
int fad_moments_dim(const fad_moments_t* h);                 /* D, or <0 on error                */
int64_t fad_moments_packed_len(const fad_moments_t* h);      /* 1 + D + D*D                      */

/* Feed a block of `n` frames (rows) of `d` features.  n == 0 is a no-op. */
int fad_moments_update(fad_moments_t* h, const void* rows, int64_t n, int64_t ld, int dtype,
                       int on_device, void* stream);

/* Reference-order means (off by default).  The reference's np.mean(embd_lst, axis=0) (fadtk/fad.py:48) adds the rows one after the
 * other in float32 (float16 frames widened first) and divides by n in float32: for frames with a sizeable offset the float16-rounded
 * result differs from the rounded EXACT mean -- what fad_moments_finalize returns otherwise -- by one ulp in a few dimensions, worth
 * 2e-5 .. 5e-4 of a small Frechet distance.  With the switch on, every update also carries numpy's float32 running column sums (one lane
 * per column walks the rows in order, on a stream of its own beside the update's other kernels: csrc/moments_kernels.h) and
 * fad_moments_finalize returns mu = float32(float64(run) / n) (numpy's quotient) widened to double; the covariance is unchanged.  Covers plain updates
 * (fad_moments_update / _multi, host or device rows, float16 / bfloat16 / float32) in the order they are fed; statistics that were imported,
 * all-reduced or fed while the switch was off have no row order: finalize then falls back to the exact mean.  The
 * fad_frechet_from_moments* entry points take the same mean for their mean term (then rounded as `mean_dtype` asks) from a handle whose
 * running sums cover its rows, the exact one otherwise.
 * enabled = 2 ("detached"): as 1, and the caller vouches that every frame matrix it feeds is COMPLETE when the update is called and stays
 * unchanged until the handle's statistics are next read (finalize / export / merge / allreduce / fad_frechet_from_moments*): the walk
 * then neither waits for the work queued on the caller's stream nor holds that stream up -- it runs beside everything and the readers
 * wait for it.  With 1 the walk starts behind the caller's stream and the update does not return the stream before it is through. */
int fad_moments_set_reference_mean(fad_moments_t* h, int enabled);

/* Feed `count` (1..32) frame matrices to `count` DIFFERENT handles of one dimension, dtype and device with ONE
 * launch of each kernel (more than 16: one launch on the 256-column-slab route -- float16, D >= 512, no running sums asked for --
 * else sixteen at a time): rows[i] (a DEVICE pointer, n[i] frames, pitch ld[i]) goes to hs[i].  The two datasets of a
 * FAD score (fad.py:292-302 calls calc_embd_statistics / load_stats twice), the 25 resamples of score_inf
 * (fad.py:333-341) ...: the workgroup slots of the GPU are shared out over all sets in proportion to their rows,
 * so the fixed costs of a pass (one 64 KiB partial tile per workgroup, pipeline fill, launches) are paid once.
 * Results are identical to `count` separate fad_moments_update calls up to the fp64 summation order of the
 * partial tiles.  Sets with n[i] == 0 are skipped. */
int fad_moments_update_multi(int count, fad_moments_t* const* hs, const void* const* rows, const int64_t* n,
                             const int64_t* ld, int dtype, void* stream);

/* fad_moments_update_multi over GATHERED rows: set i is fed the n_idx[i] frames rows[idx[i][0]], rows[idx[i][1]], ... of ONE resident
 * matrix `rows` [n_src x ld] (device; idx[i]: device, int32, 0 <= idx < n_src), in that order -- the resamples with replacement of
 * score_inf (fad.py:333-337: np.random.choice + fancy indexing, 1.3 GB of copies at config 3) without materialising them: for float16
 * frames of D >= 512 the gather rides on the row offsets of the slab kernel's LDS-DMA loads and of the running-sum walk; other inputs
 * are gathered into the handles' staging areas first.  Results as fad_moments_update_multi on the materialised matrices (count <= 16). */
int fad_moments_update_multi_indexed(int count, fad_moments_t* const* hs, const void* rows, int64_t n_src, int64_t ld, int dtype,
                                     const int32_t* const* idx, const int64_t* n_idx, void* stream);

/* Same, for `n_segments` files/songs stored back to back: segment s owns rows
 * [offsets[s], offsets[s+1]) (offsets is a HOST array of n_segments+1 entries).  If
 * seg_sums != NULL it receives the per-segment column sums, [n_segments x D] float64 (host or
 * device per on_device): the per-file means of utils.py:16 and the per-song means of
 * fad.py:377 are seg_sums / segment length. */
int fad_moments_update_segmented(fad_moments_t* h, const void* rows, int64_t n, int64_t ld, int dtype,
                                 const int64_t* offsets, int64_t n_segments, double* seg_sums,
                                 int on_device, void* stream);

/* The per-file mean terms of the online statistics.  fadtk merges per-file (mean, scatter, n) triplets
 * (utils.py:13-16, 36-40) and np.mean of a float16 file is float16, so the dataset covariance it returns is
 *   (sum xx^T - sum_f n_f m_f m_f^T  +  sum_f n_f m~_f m~_f^T - N mu~ mu~^T) / (N - 1),  mu~ = sum_f n_f m~_f / N
 * with m_f the exact and m~_f the dtype-rounded mean of file f.  Given the per-file column sums (seg_sums
 * [n_files x D] float64, from fad_moments_update_segmented) and sizes (int64 [n_files]) -- on_device bit 0: seg_sums is
 * a device pointer, bit 1: sizes is (the usual call has the sums in HBM and the sizes on the host: on_device = 1) --
 * this accumulates the rows sqrt(n_f) m_f into `exact`, sqrt(n_f) m~_f into `rounded` and n_f m~_f into
 * `weighted` (three distinct handles of dimension D): afterwards sum_xxT(exact) and sum_xxT(rounded) are the two
 * D x D terms and sum_x(weighted) = N mu~ -- all sum-reducible across batches and ranks.  Empty files add nothing. */
int fad_moments_update_file_means(fad_moments_t* exact, fad_moments_t* rounded, fad_moments_t* weighted,
                                  const double* seg_sums, const int64_t* sizes, int64_t n_files, int dtype,
                                  int on_device, void* stream);

/* The two calls above with the reference's OWN per-file means.  np.mean of a float16 (float32) file (utils.py:16; per song fad.py:377)
 * adds the file's rows one after the other in float32 and rounds the quotient to the file's dtype: for a file of a few thousand frames
 * with an offset that differs from the rounded exact mean -- what fad_moments_update_file_means forms from seg_sums -- by one ulp in
 * ~0.3 % of the columns.  fad_moments_update_segmented_ref additionally returns those float32 running column sums per segment
 * (seg_runsums [n_segments x D] float32, host or device like seg_sums; NULL = none; float16 / bfloat16 / float32 rows: for float64
 * rows numpy's sum is the exact one) -- a second walk over rows the tile kernel has just read.  fad_moments_update_file_means_ref takes
 * them (on_device bit 2: seg_runsums is a device pointer; NULL = the rounded exact means) and forms m~_f = round(float32(run_f / n_f)). */
int fad_moments_update_segmented_ref(fad_moments_t* h, const void* rows, int64_t n, int64_t ld, int dtype,
                                     const int64_t* offsets, int64_t n_segments, double* seg_sums, float* seg_runsums,
                                     int on_device, void* stream);
int fad_moments_update_file_means_ref(fad_moments_t* exact, fad_moments_t* rounded, fad_moments_t* weighted,
                                      const double* seg_sums, const float* seg_runsums, const int64_t* sizes, int64_t n_files, int dtype,
                                      int on_device, void* stream);

/* dst += src.  (Rows from another handle have no place in dst's row order: a handle with fad_moments_set_reference_mean on falls back
 * to the exact mean afterwards, as after import / allreduce.) */
int fad_moments_merge(fad_moments_t* dst, const fad_moments_t* src, void* stream);
/* Copy the packed float64 statistics out / in (the buffer an RCCL all-reduce runs over). */
int fad_moments_export(const fad_moments_t* h, double* packed, int on_device, void* stream);
int fad_moments_import(fad_moments_t* h, const double* packed, int on_device, void* stream);
int fad_moments_count(const fad_moments_t* h, int64_t* n, void* stream);

/* Sum the packed statistics of all ranks IN PLACE with one collective (the only
 * exchange of the data-parallel path; replaces the pickled per-file (mean, scatter, n) tuples of
 * utils.py:19-46 / the process pool of fad_batch.py:43-48).  `rccl_comm` is the caller's ncclComm_t;
 * ncclAllReduce(count = 1 + D + D*D, ncclFloat64, ncclSum) is looked up in the RCCL library the host
 * process already has loaded (else librccl.so.1), so the library adds no second RCCL to the process.
 * FAD_ERR_INVALID when no RCCL can be found, FAD_ERR_HIP when the collective reports an error.
 * (torch.distributed does not hand out its communicator: the Python host reduces the same buffer through
 * torch.distributed.all_reduce instead, fadtk_amd/dist.py.) */
int fad_moments_allreduce(fad_moments_t* h, void* rccl_comm, void* stream);

/* mu = sum_x / n ; cov = (sum_xxT - n mu mu^T) / (n - ddof)   (np.mean / np.cov, fad.py:48).
 * mu [D], cov [D*D] float64.  n < 2 -> FAD_ERR_TOO_FEW_ROWS (fad.py:46-47). */
int fad_moments_finalize(const fad_moments_t* h, int ddof, double* mu, double* cov, int64_t* n,
                         int on_device, void* stream);

/* ------------------------------------------------------------------ Frechet distance
 * Replaces calc_frechet_distance (fadtk/fad.py:51-120):
 *   ||mu1-mu2||^2 + tr C1 + tr C2 - 2 tr sqrt(C1 C2)
 * tr sqrt(C1 C2) = sum_i sqrt(lambda_i(C1 C2)) -- the value the reference returns through
 * scipy.linalg.eig (fad.py:91-92) -- is computed with a coupled Newton-Schulz iteration on MFMA tiles: for
 * well-conditioned products (and d a multiple of 64) the iterations run in low precision (float32 on the f32 MFMA; for
 * d = 256 / 512 / 768 / 1024 split float16 on the f16 MFMA with the two products that need it formed EXACTLY through
 * base-128 digit planes on the int8 MFMA) and one float64-accurate correction restores float64 accuracy; otherwise (or
 * when max_iter / tol are given) everything runs in float64.
 * eps: added to both diagonals for a retry when the first attempt diverges (fad.py:94-99).
 * max_iter <= 0 -> default (64); tol <= 0 -> default.
 */
typedef struct fad_diag {
    int32_t iters;          /* Newton-Schulz iterations executed                                 */
    int32_t converged;      /* 1: residual < tol, 2: trace stagnated / divergence guard (rank-deficient or near-singular
                               product), 3: float32 iterations + float64 correction accepted, 0: max_iter */
    int32_t used_eps;       /* 1 if the eps-regularised retry produced the result                */
    int32_t route;          /* with converged == 3: 1 = float32 iterations on the f32 MFMA, 2 = split-float16 iterations + exact
                               int8-MFMA products (d = 256 / 384 / 512 / 768 / 1024); 0 otherwise (all-float64 iteration)  */
    double residual;        /* ||I - Z Y||_F at the last iteration                               */
    double scale;           /* c with Y0 = C1 C2 / c                                             */
    double mean_term;       /* ||mu1 - mu2||^2 in float64                                        */
    double tr1, tr2;        /* tr C1, tr C2                                                      */
    double tr_sqrt;         /* tr sqrt(C1 C2)                                                    */
    int32_t verified;       /* route 2 only: 1 = accepted on the MEASURED verification record (1/2 tr(EP) added, 4 x 1/8 |tr(ZPP)| +
                               ||E||^2 ||P|| as the error estimate: csrc/frechet.hip) where the norm bound says nothing (decaying
                               spectra); 0 = accepted on the norm bound, or another route                                  */
    int32_t reserved;
} fad_diag_t;

int fad_frechet(int d, const double* mu1, const double* cov1, const double* mu2, const double* cov2,
                double eps, int max_iter, double tol, int on_device, int device, void* stream,
                double* out_fad, fad_diag_t* diag);

/* Same, straight from two moment handles (no host round trip of mu/cov).
 * mean_dtype: how ||mu1 - mu2||^2 is formed.  FAD_F16 / FAD_BF16 / FAD_F32 = as the reference does for embeddings
 * of that dtype: np.mean keeps the dtype (fad.py:48 on the float16 arrays of model_loader.py:47-48), so the means are
 * rounded to it, subtracted in it, and diff.dot(diff) (fad.py:83, 119) is accumulated in float32 and rounded to it
 * (float16: bit for bit what numpy returns).  Anything else (FAD_F64, -1): float64 means.
 * FAD_MEAN_SECOND_ONLY | dtype: only the mean of the SECOND handle is rounded to the dtype, difference and dot product stay in
 * float64 -- score_inf's case (fad.py:333-341): a float64 baseline mean from the statistics cache against np.mean of resampled
 * float16 frames. */
#define FAD_MEAN_SECOND_ONLY 16
int fad_frechet_from_moments(const fad_moments_t* h1, const fad_moments_t* h2, int ddof, double eps,
                             int max_iter, double tol, int mean_dtype, void* stream, double* out_fad, fad_diag_t* diag);

/* Several scores in flight.  The square-root chain of ONE score is a dozen dependent launches of small kernels: it is
 * bound by launch latency.  begin() puts (mu, Sigma) of both handles and the whole chain on `stream` and returns at once;
 * end() waits for it and delivers the same result (and the same errors) as fad_frechet_from_moments -- topping the
 * iteration up or falling back to the float64 iteration when the device says so.  A caller that begins score k+1 before it
 * ends score k never leaves the device waiting between scores (bench.py: +10 % scores/s on ONE stream); with one stream
 * per score the chains and moments passes of consecutive scores overlap as well (another +20 %: bench.py's timed layout).
 * The handles may be reset / fed again ON `stream` as soon as begin() has returned (their statistics were copied out in
 * stream order); on another stream only after end().  A job must be ended (or cancelled) by the host thread that began it:
 * the slots are thread-local, 8 per thread and device.  cancel() gives the slot back without a result. */
typedef struct fad_frechet_job fad_frechet_job_t;
int fad_frechet_from_moments_begin(const fad_moments_t* h1, const fad_moments_t* h2, int ddof, double eps, int mean_dtype,
                                   void* stream, fad_frechet_job_t** job);
int fad_frechet_end(fad_frechet_job_t* job, double* out_fad, fad_diag_t* diag);
int fad_frechet_cancel(fad_frechet_job_t* job);

/* `count` (1..FAD_MULTI_MAX_PAIRS) independent scores in ONE job: pair b = (h1[b], h2[b]).  The eight launches of the square-root chain carry all
 * pairs (each launch costs ~4 us before it does anything and its workgroups are latency-bound: B chains as one batch take little
 * longer than one); multi_end() delivers out_fad[b] (and diag[b], or diag == NULL) exactly as fad_frechet_from_moments would for
 * that pair -- a pair the batch does not finish or accept goes through that very entry point.  Same stream / thread rules as
 * begin() / end(); one slot per job.  Used by bench.py for the scores it keeps in flight and by score_inf (fad.py:304-351: 25
 * independent scores against one baseline). */
#define FAD_MULTI_MAX_PAIRS 32   /* (8 until round 5; 16 pairs put a workgroup of the batched kernels on every CU, 32 two) */
int fad_frechet_from_moments_multi_begin(int count, const fad_moments_t* const* h1, const fad_moments_t* const* h2, int ddof,
                                         double eps, int mean_dtype, void* stream, fad_frechet_job_t** job);
int fad_frechet_multi_end(fad_frechet_job_t* job, int count, double* out_fad, fad_diag_t* diag);

/* ------------------------------------------------------------------ per-song FAD (--indiv)
 * Replaces the loop of score_individual (fadtk/fad.py:373-387): for every song s (rows
 * [offsets[s], offsets[s+1]) of `rows`), FAD between the baseline (mu_b, cov_b) and that song's
 * own (mu_s, cov_s).  Songs with fewer than 2 frames get status FAD_ERR_TOO_FEW_ROWS and a NaN
 * score (the reference drops them, fad.py:380-391).  A song with a NaN or infinite frame, and every song of two or more frames when
 * cov_b holds a non-finite entry, gets status FAD_ERR_NOT_FINITE and a NaN score, in every route; the other songs of the call keep
 * the bits they have without it (the reference's eig raises on such a song and score_individual drops it).  No song comes back with
 * a non-finite score and status FAD_OK or FAD_ERR_NOT_CONVERGED.
 * mean_mode: 0 = song mean in float64; 1 = round the song mean to the input dtype first, as
 * np.mean does for float16 (model_loader.py:47-48 + fad.py:48).
 * on_device = 1: rows, mu_b and cov_b are DEVICE pointers (a caller scoring many batches against one baseline uploads it
 * once); offsets, out_scores and out_status are host pointers either way.  cov_b is read as (cov_b + cov_b^T)/2.
 * Routes, chosen per song by its frame count n (the result does not depend on the route beyond ~1e-8 of a score):
 *   n = 2: closed form; n - 1 < D: the Gram form on the n - 1 non-zero eigenvalues; n >= D + 1 and D in {128, 256, 384, 512, 768,
 *   1024}: the low-precision chain of the single pair, batched over the songs (exact int8-MFMA products, split-float16
 *   Newton-Schulz, one float64-accurate correction, accepted per song on a bound of what the correction neglects), with
 *   float16 frames also the covariances on the float16 matrix pipe; whatever that chain does not accept -- and every other D --
 *   the float64 Newton-Schulz routes.  Environment switches (tests, diagnosis): FAD_SONG_FAST=0 (float64 routes only),
 *   FAD_SONG_BIG=<smallest batch on 128 x 128 tiles>, FAD_SONG_RES=0, FAD_FAST_TRACE=1.
 */
int fad_frechet_batched_vs_baseline(int d, const double* mu_b, const double* cov_b,
                                    const void* rows, int64_t n_rows, int64_t ld, int dtype,
                                    const int64_t* offsets, int64_t n_songs, int mean_mode,
                                    int on_device, int device, void* stream,
                                    double* out_scores, int32_t* out_status);

/* ------------------------------------------------------------------ log-mel front ends
 * Replace the third-party feature extraction that runs inside ModelLoader._get_embedding
 * (fadtk/model_loader.py:99,108 VGGish / torchvggish mel_features; :661,666 Whisper /
 * transformers WhisperFeatureExtractor; :385,406 CLAP-HTSAT / torchlibrosa).
 * wav: float32 mono samples of n_clips clips stored back to back, clip c = wav[offsets[c] ..
 * offsets[c+1]) (offsets: HOST array of n_clips+1).  wav/out are host or device per on_device.
 *
 * VGGish  (16 kHz): periodic-Hann 400 / hop 160 / FFT 512 magnitude, 64 HTK mels 125-7500 Hz,
 *          log(mel + 0.01), non-overlapping examples of 96 frames, incomplete tail dropped.
 *          out [total_examples][96][64]; example_offsets (host, n_clips+1, may be NULL) receives the
 *          first example of each clip.
 * Whisper (16 kHz): clip zero-padded / cut to 480000 samples, centred reflect STFT 400 / hop 160,
 *          power, n_mels (80 or 128) Slaney mels 0-8 kHz, log10(max(.,1e-10)), clamp to
 *          (clip max - 8), (x + 4) / 4.   out [n_clips][n_mels][3000].
 * HTSAT   (48 kHz): centred reflect STFT 1024 / hop 480, power, 64 Slaney mels 50-14000 Hz,
 *          10 log10(max(.,1e-10)).  Every clip must give n_frames_out = 1 + n_samples/480 frames.
 *          Clips of 512 samples or fewer -> FAD_ERR_SHAPE: the 512-sample reflect pad must be shorter
 *          than the clip (torch.stft's rule on the reference's path).  out [n_clips][n_frames_out][64].
 */
int64_t fad_logmel_vggish_num_examples(int64_t n_samples);
int fad_logmel_vggish(const float* wav, const int64_t* offsets, int64_t n_clips, float* out,
                      int64_t out_capacity_examples, int64_t* example_offsets, int on_device, int device,
                      void* stream);
int fad_logmel_whisper(const float* wav, const int64_t* offsets, int64_t n_clips, int n_mels, float* out,
                       int on_device, int device, void* stream);
int fad_logmel_htsat(const float* wav, const int64_t* offsets, int64_t n_clips, int64_t n_frames_out,
                     float* out, int on_device, int device, void* stream);

/* ------------------------------------------------------------------ audio normalisation
 * Replaces the resampler of FrechetAudioDistance.load_audio (fadtk/fad.py:151-159):
 *   torchaudio.transforms.Resample(fs, model_sr, lowpass_filter_width=64, rolloff=0.9475937167399596,
 *                                  resampling_method="sinc_interp_kaiser", beta=14.769656459379492)
 * on a mono float32 signal (the mono mix of fad.py:150 is the caller's), output length
 * ceil(new_sr * n / orig_sr) = fad_resample_num_samples().  quantize_pcm16 != 0 also applies the 16-bit round
 * trip the reference makes through its cache file (fad.py:160 saves PCM_S 16, model_loader.py:64 reads int16 /
 * 32768): out = clamp(rint(y * 32768), -32768, 32767) / 32768.
 * Rates whose ratio needs a filter table above 256 MiB (nearly coprime rates) are refused with FAD_ERR_INVALID. */
int64_t fad_resample_num_samples(int64_t n, int orig_sr, int new_sr);
int fad_resample_kaiser(const float* wav, int64_t n, int orig_sr, int new_sr, int quantize_pcm16, float* out,
                        int64_t out_capacity, int on_device, int device, void* stream);

/* ------------------------------------------------------------------ Kernel Audio Distance (KAD)
 * Not in the reference: the unbiased Gaussian-kernel MMD^2 of Chung et al. 2025 ("KAD: No More FAD!") between the rows x [n x d] and
 * y [m x d] that FAD would reduce to (mu, Sigma):
 *   k(a, b) = exp(-|a - b|^2 / (2 sigma^2)),   MMD^2 = Kxx + Kyy - 2 Kxy,
 *   Kxx = sum_{i != j} k(x_i, x_j) / (n (n - 1)),  Kyy likewise,  Kxy = sum_{i, j} k(x_i, y_j) / (n m).
 * The score may be negative (the estimator is unbiased).  Rows are float16, bfloat16 or float32 (FAD_F64 -> FAD_ERR_INVALID:
 * cast), 1 <= d <= 2048, ld >= d; dot products in float32 on the matrix cores, sums in float64, the same bits on every run.
 * n or m < 2 -> FAD_ERR_TOO_FEW_ROWS; a NaN/Inf row norm -> FAD_ERR_NOT_FINITE.  Work goes on `stream`; both calls synchronise it. */
typedef struct fad_kad_result {
    double mmd2, kxx_mean, kyy_mean, kxy_mean, bandwidth;   /* bandwidth: the sigma used */
    int64_t n, m;
} fad_kad_result_t;
/* median pairwise Euclidean distance within one set (the default bandwidth): np.median(scipy.spatial.distance.pdist(x)),
 * the mean of the two middle distances when n (n - 1) / 2 is even; exact selection on the float32 squared distances */
int fad_kad_median_distance(const void* x, int64_t n, int64_t ld, int64_t d, int dtype, int on_device,
                            double* sigma, int device, void* stream);
/* unbiased Gaussian-kernel MMD^2; bandwidth <= 0: the median distance of x (a median of 0 -> FAD_ERR_INVALID).  d^2 is formed as
 * |a|^2 + |b|^2 - 2 a.b in float32, so equal rows give exactly 0 only when their products sum exactly (e.g. integer-valued rows);
 * otherwise a rounding residue may leave a tiny positive median, which is used as the bandwidth. */
int fad_kad(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
            int on_device, double bandwidth, fad_kad_result_t* out, int device, void* stream);
/* ------------------------------------------------------------------ KAD kernels
 * The _k entry points below take the kernel as the KAD toolkit does, one bandwidth convention for all, gamma = 1 / (2 sigma^2):
 *   FAD_KAD_GAUSSIAN   k(a, b) = exp(-gamma |a - b|^2)
 *   FAD_KAD_IQ         k(a, b) = 1 / (1 + gamma |a - b|^2)          (inverse quadratic)
 *   FAD_KAD_IMQ        k(a, b) = 1 / sqrt(1 + gamma |a - b|^2)      (inverse multiquadric)
 * The toolkit forms gamma = 1 / (2 sigma^2 + eps) with eps = 1e-8; this library adds no eps, for any kernel (a median of 0 is an error
 * instead).  That is the only difference.  Each _k function is its parent with `kernel` after `bandwidth`: the same arguments, results,
 * errors and default bandwidth (a median distance, whatever the kernel); the parent is the _k function with FAD_KAD_GAUSSIAN, bit for
 * bit.  Any other value of `kernel` -> FAD_ERR_INVALID.  The heavy-tailed kernels are evaluated in float32 as 1 / max(1 + t, 1) (its
 * square root for imq), t = gamma |a - b|^2; the permutation test's c0 under the default sigma is k at t = 1/2: 2/3 and 1 / sqrt(1.5). */
typedef enum fad_kad_kernel { FAD_KAD_GAUSSIAN = 0, FAD_KAD_IQ = 1, FAD_KAD_IMQ = 2 } fad_kad_kernel;
int fad_kad_k(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
              int on_device, double bandwidth, int kernel, fad_kad_result_t* out, int device, void* stream);
int fad_kad_individual_k(const void* x, int64_t n, int64_t ldx, const void* rows, int64_t n_rows, int64_t ldy,
                         const int64_t* offsets, int64_t n_songs, int64_t d, int dtype, int on_device, double bandwidth, int kernel,
                         fad_kad_result_t* base, double* out_mmd2, double* out_kyy_mean, double* out_kxy_mean,
                         int32_t* out_status, int device, void* stream);
int fad_kad_uncertainty_k(const void* x, int64_t n, int64_t ldx, const void* const* ys, const int64_t* ms, const int64_t* ldys,
                          int n_sets, int64_t d, int dtype, int on_device, double bandwidth, int kernel,
                          fad_kad_result_t* out /* [n_sets] */, double* cov /* [n_sets * n_sets] */,
                          double* proj_x /* [n_sets * n] or NULL */, double* proj_y /* [sum m_s] or NULL */, int device, void* stream);
int fad_kad_permutation_test_k(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                               int on_device, double bandwidth, int kernel, const uint32_t* labels, int64_t n_perm,
                               int labels_on_device, fad_kad_result_t* observed, double* null /* [n_perm] host */, double* p_value,
                               int device, void* stream);
/* ------------------------------------------------------------------ KAD at several bandwidths (bandwidth sweep)
 * fad_kad_k at n_bw bandwidths (1 .. FAD_KAD_MAX_BANDWIDTHS) in one call: both sets are packed once, and each of the three passes forms
 * a tile's dot products once for up to 8 bandwidths, whose kernel values go into sums of their own.  relative == 0: bandwidths[b] is
 * sigma_b itself and no median is computed; relative != 0: bandwidths[b] is a factor, sigma_b = bandwidths[b] * the median pairwise
 * distance of x (found once; a median of 0 -> FAD_ERR_INVALID), so the factor 1.0 gives fad_kad_k's default result, bandwidth included.
 * Every entry must be finite and > 0 in both modes ("<= 0 means the median" does not exist here: ask for the factor 1); duplicates and
 * any order are allowed.  out[b] is fad_kad_k's result for sigma_b, in the caller's order -- bit for bit whenever the two calls cut
 * their passes into the same launches (always when a pass fits one launch of both: 16-bit rows up to D = 512 at n = m = 100 000, for
 * one; past that the float32 partial sums are still the same and only the float64 order of adding them differs).  The mean of the
 * n_bw mmd2 is MMD^2 under the mixture kernel (1 / n_bw) sum_b k_b, exactly, by linearity.  Argument errors come before any device
 * call, with fad_kad_k's codes: NULL pointers, n_bw outside 1 .. 32, an entry that is not finite and > 0, an unknown kernel, dtype, d,
 * ld < d, n or m < 2 -> FAD_ERR_TOO_FEW_ROWS.
 * A NaN/Inf row norm -> FAD_ERR_NOT_FINITE; a sigma_b whose kernel constant leaves float32 -> FAD_ERR_INVALID, the message naming b.
 * Any refusal fails the whole call and leaves `out` untouched.  No float atomics: the same bits on every run.  Synchronises `stream`. */
#define FAD_KAD_MAX_BANDWIDTHS 32
int fad_kad_sweep(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                  const double* bandwidths, int n_bw, int relative, int kernel, fad_kad_result_t* out /* [n_bw] */, int device,
                  void* stream);
/* ------------------------------------------------------------------ per-song KAD (--indiv)
 * For every song s (rows [offsets[s], offsets[s+1]) of `rows` [n_rows x d]), KAD between the baseline x [n x d] and that song alone,
 * with one sigma for all songs: what fad_kad(x, song_s, bandwidth = sigma) gives, in one call that packs the baseline, finds sigma
 * (bandwidth <= 0: the median distance of x) and sums its Kxx once:
 *   mmd2[s] = Kxx + Kyy(s) - 2 Kxy(s),  Kyy(s) = sum_{i != j in s} k / (m_s (m_s - 1)),  Kxy(s) = sum_{x, j in s} k / (n m_s).
 * `base` receives kxx_mean, bandwidth and n -- bit for bit what fad_kad and fad_kad_median_distance give on the same x -- with
 * m = n_rows and NaN in its other fields.  Songs with fewer than 2 frames get status FAD_ERR_TOO_FEW_ROWS, songs with a NaN/Inf row
 * norm FAD_ERR_NOT_FINITE, both with NaN outputs; the other songs do not depend on them.  Rows and x are host or device per on_device
 * (one dtype: float16, bfloat16 or float32); offsets [n_songs + 1] and the outputs [n_songs] are host pointers either way.  Argument
 * errors (offsets that do not run from 0 to n_rows or that decrease, dtype, d, ld, n < 2 -> FAD_ERR_TOO_FEW_ROWS) come before any
 * device call.  n_rows < 2^31 - 128.  The same bits on every run; synchronises `stream`. */
int fad_kad_individual(const void* x, int64_t n, int64_t ldx, const void* rows, int64_t n_rows, int64_t ldy,
                       const int64_t* offsets, int64_t n_songs, int64_t d, int dtype, int on_device, double bandwidth,
                       fad_kad_result_t* base, double* out_mmd2, double* out_kyy_mean, double* out_kxy_mean,
                       int32_t* out_status, int device, void* stream);
/* ------------------------------------------------------------------ KAD standard errors, paired comparison of sets
 * One baseline x [n x d] and S evaluation sets ys[s] [ms[s] x ldys[s]] (1 <= S <= 64), one sigma for all (bandwidth <= 0: the median
 * distance of x, as fad_kad resolves it).  With k as above, for every row i of x and row l of set s:
 *   mxx(i) = sum_{j != i} k(x_i, x_j) / (n - 1)          mxs(i) = sum_l k(x_i, y^s_l) / m_s
 *   mss(l) = sum_{l' != l} k(y^s_l, y^s_l') / (m_s - 1)   msx(l) = sum_i k(x_i, y^s_l) / n
 *   a^s_i = mxx(i) - mxs(i)                               b^s_l = mss(l) - msx(l)
 *   MMD^2_s   = mean_i a^s_i + mean_l b^s_l     (= Kxx + Kyy - 2 Kxy: the quantity fad_kad returns)
 *   cov[s][t] = 4 / (n (n - 1)) sum_i (a^s_i - mean a^s)(a^t_i - mean a^t)  +  [s = t] 4 / (m_s (m_s - 1)) sum_l (b^s_l - mean b^s)^2
 *   stderr_s  = sqrt(cov[s][s])
 * cov is the FIRST-ORDER (Hoeffding-projection) covariance of the S unbiased estimates, which share x and are otherwise independent
 * (the covariance of the relative-similarity test of Bounliphone et al., ICLR 2016).  A paired comparison of sets s and t is
 * z = (MMD^2_s - MMD^2_t) / sqrt(cov_ss + cov_tt - 2 cov_st), two-sided p = erfc(|z| / sqrt 2).  The estimate is meaningful when the
 * sets differ from the baseline (any generative model).  When a set has x's distribution the U-statistic is degenerate and the
 * estimate understates the spread: this is NOT a test of "same distribution".  m_s >= 2 is all that is required; small sets simply
 * get a poor estimate.
 * out[s]: mmd2, kxx_mean (the same bits in every out[s]: one fixed-order sum), kyy_mean, kxy_mean, bandwidth, n and m = m_s.  cov
 * [S x S] row-major; proj_x [S x n] a^s_i and proj_y [sum m_s] b^s_l (set after set) when not NULL.  All outputs are host pointers;
 * rows are host or device per on_device, one dtype (float16, bfloat16 or float32), 1 <= d <= 2048.  Argument errors come before any
 * device call: dtype, d, ld < d, n or m_s < 2 -> FAD_ERR_TOO_FEW_ROWS, S outside 1 .. 64, a non-finite bandwidth; a NaN/Inf row norm
 * -> FAD_ERR_NOT_FINITE.  Float64 sums in a fixed order, no float atomics: the same bits on every run.  Synchronises `stream`. */
int fad_kad_uncertainty(const void* x, int64_t n, int64_t ldx, const void* const* ys, const int64_t* ms, const int64_t* ldys,
                        int n_sets, int64_t d, int dtype, int on_device, double bandwidth, fad_kad_result_t* out /* [n_sets] */,
                        double* cov /* [n_sets * n_sets] */, double* proj_x /* [n_sets * n] or NULL */,
                        double* proj_y /* [sum m_s] or NULL */, int device, void* stream);

/* ------------------------------------------------------------------ KAD two-sample permutation test
 * Is y distinguishable from x at all?  Z = [x; y] pooled (N = n + m rows), K' = the Gaussian kernel matrix of Z with a zero diagonal,
 * r = K'1, T = 1'r.  A labelling is a 0/1 vector u over Z's rows with exactly n ones (the "baseline" group):
 *   q(u) = u'K'u,  R(u) = u'r,  Sxx = q,  Sxy = R - q,  Syy = T - 2R + q
 *   t(u) = Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m)        (fad_kad's MMD^2 when u is x's own labelling)
 * Labelling 0 is the observed one (Z's first n rows), added by the library; `labels` holds the n_perm random ones as packed bits,
 * [n_perm x ceil(N / 32)] uint32 row-major, bit (i & 31) of word i >> 5 is row i of Z; every labelling has exactly n ones and no bit at
 * or past N.  null[p] = t(u_{p+1}) (host, n_perm entries); p_value = (1 + #{p : null[p] >= t_0}) / (n_perm + 1), compared in float64.
 * observed: mmd2 = t_0, its kxx / kyy / kxy means, sigma, n and m.
 * Bandwidth <= 0: sigma = the median pairwise distance of Z, bit for bit fad_kad_median_distance on the concatenated rows -- a function of
 * the pooled rows alone, so the test is exact.  A given sigma is used as is; KAD's baseline median (fad_kad's default) depends on the
 * labelling and makes the test approximate.  Every labelling goes through the same kernels, so the p-value is exact under
 * exchangeability whatever the rounding: q is summed on the matrix cores from f16(k - c0) (c0 = e^-1/2 under the default sigma, the
 * mean off-diagonal kernel value of Z under a given one), R and T from float32 kernel values, all in float64 past one tile.
 * Rows host or device per on_device, labels per labels_on_device.  Argument errors come before any device call: dtype, d outside
 * 1 .. 2048, ld < d, n or m < 2 -> FAD_ERR_TOO_FEW_ROWS, n_perm outside 1 .. 65536, N >= 2^31 - 128, a non-finite bandwidth, host
 * labels with a wrong count -> FAD_ERR_INVALID.  Device labels with a wrong count -> FAD_ERR_INVALID (checked on the device); a NaN/Inf
 * row norm -> FAD_ERR_NOT_FINITE.  Workspace (kept per thread and device): Z's image, about 3 (n_perm + 33) N / 8 bytes of label words,
 * the row-sum pass's slots (128 float64 per unit, about 16 384 units), and at most 512 x 1024 float64 slots per group of 1024 labellings.  No float atomics: the
 * same bits on every run.  Synchronises `stream`. */
int fad_kad_permutation_test(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                             int on_device, double bandwidth, const uint32_t* labels, int64_t n_perm, int labels_on_device,
                             fad_kad_result_t* observed, double* null /* [n_perm] host */, double* p_value, int device, void* stream);
/* ------------------------------------------------------------------ KAD permutation test at several bandwidths, aggregated
 * fad_kad_permutation_test_k at n_bw bandwidths (1 .. FAD_KAD_PERM_MAX_BANDWIDTHS) on the same labellings in one call, and one p-value
 * over all of them.  A test at one sigma is blind to differences that live at another scale; the aggregate does not depend on having
 * picked the right one.  Z is packed once, the labellings and their two bit layouts are prepared once, the row-sum pass forms a tile's
 * dot products once for up to 4 bandwidths, and a triangle walk of the permutation pass carries up to 4 bandwidths wherever their
 * labelling words fit its 32 partial sums per lane together (4 bandwidths x 8 words of 32 labellings, 2 x 16, or 1 x 32: as few walks as
 * that allows, about n_bw (n_perm + 1) / 1024 of them).
 * relative == 0: bandwidths[b] is sigma_b.  relative != 0: bandwidths[b] is a factor of the median pairwise distance of the POOLED rows
 * (found once; a median of 0 -> FAD_ERR_INVALID): sigma_b is then a function of the pooled rows alone and every test stays exact; the
 * factor 1.0 gives the single test's default sigma bit for bit.  Every entry must be finite and > 0; duplicates and any order are
 * allowed.  The shift c0_b is always the mean off-diagonal kernel value of Z under sigma_b, which is what the single call uses under
 * a given sigma.  observed[b], null[b * n_perm + p] and p_values[b] are fad_kad_permutation_test_k(bandwidth = sigma_b)'s, in the
 * caller's order -- bit for bit whenever both calls run the permutation pass over Z's triangle as one launch (the row sums agree at any
 * size); past that the per-tile float32 sums are the same and only the float64 order of adding them differs.
 * Aggregation (fad_kad_aggregate: host, float64, pure counting; the sweep calls it on its own statistics).  t is [n_bw][n_lab]
 * row-major, labelling 0 the observed one (n_lab = n_perm + 1 >= 2):
 *   p_b(j) = #{i : t_b(i) >= t_b(j)} / n_lab        p_values[b] = p_b(0), the single test's p-value
 *   m(j)   = min_b p_b(j)                           p_aggregated = #{j : m(j) <= m(0)} / n_lab
 * the single-step min-p correction on the same labellings with uniform weights over the bandwidths (the weights of MMDAgg, Schrab et
 * al. 2023).  It is exact under exchangeability, because the observed labelling goes through the same code as every other.  With one
 * bandwidth p_aggregated == p_values[0]; a bandwidth given twice changes nothing.
 * Argument errors come before any device call, with the single test's codes: NULL pointers, n_bw outside 1 .. 16, an entry that is not
 * finite and > 0, an unknown kernel, and everything fad_kad_permutation_test_k refuses about rows and labellings.  A sigma_b whose
 * kernel constant leaves float32 -> FAD_ERR_INVALID, the message naming b.  Any refusal fails the whole call and leaves every output
 * untouched.  No float atomics: the same bits on every run.  Synchronises `stream`. */
#define FAD_KAD_PERM_MAX_BANDWIDTHS 16
int fad_kad_permutation_sweep(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                              int on_device, const double* bandwidths, int n_bw, int relative, int kernel, const uint32_t* labels,
                              int64_t n_perm, int labels_on_device, fad_kad_result_t* observed /* [n_bw] */,
                              double* null /* [n_bw][n_perm] host */, double* p_values /* [n_bw] */, double* p_aggregated, int device,
                              void* stream);
int fad_kad_aggregate(const double* t /* [n_bw][n_lab], labelling 0 observed */, int n_bw, int64_t n_lab,
                      double* p_values /* [n_bw] */, double* p_aggregated);

/* ------------------------------------------------------------------ precision, recall, density, coverage (k-NN manifold metrics)
 * Not in the reference: Kynkaanniemi et al. 2019 (precision, recall) and Naeem et al. 2020 (density, coverage) between the baseline
 * ("real") rows x [n x d] and the evaluation ("fake") rows y [m x d], with k neighbours, Euclidean distances compared squared:
 *   r_X(i) = the k-th smallest distance from x_i to the OTHER rows of x (self excluded by index, so a duplicate row is a neighbour at
 *            distance 0); r_Y(j) likewise within y;
 *   precision = #{j : some i has d(x_i, y_j) < r_X(i)} / m        recall   = #{i : some j has d(x_i, y_j) < r_Y(j)} / n
 *   density   = sum_j #{i : d(x_i, y_j) < r_X(i)} / (k m)          coverage = #{i : some j has d(x_i, y_j) < r_X(i)} / n
 * All comparisons strict, as in the authors' `prdc` package (its radius is the (k+1)-th smallest of a row holding self at 0).  Every
 * decision is taken on the float32 d^2 = |a|^2 + |b|^2 - 2 a.b (products on the matrix cores, clamped at 0), so a pair within rounding of
 * a radius may fall the other way from a float64 evaluation; integer-valued rows are exact.  Rows are float16, bfloat16 or float32,
 * host or device per on_device, 1 <= d <= 2048, ld >= d.  k outside 1 .. 16 or an unknown dtype -> FAD_ERR_INVALID; n <= k or m <= k ->
 * FAD_ERR_TOO_FEW_ROWS (argument errors come before any device call); a NaN/Inf row norm -> FAD_ERR_NOT_FINITE.  n, m < 2^31 - 128.
 * Integer counts: the same result on every run.  Work goes on `stream`; the call synchronises it. */
typedef struct fad_prdc_result {
    double precision, recall, density, coverage;
    int64_t n, m, k;
} fad_prdc_result_t;
/* optional per-row outputs on the host, any of them NULL */
typedef struct fad_prdc_detail {
    float* radius2_x;   /* [n] r_X(i)^2 as the comparisons used it (float32) */
    float* radius2_y;   /* [m] */
    int32_t* balls_y;   /* [m] #{i : d^2(x_i, y_j) < r_X(i)^2} */
    int32_t* flags_x;   /* [n] bit 0: recalled (P2 for some j), bit 1: covered (P1 for some j) */
} fad_prdc_detail_t;
int fad_prdc(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
             int on_device, int k, fad_prdc_result_t* out, fad_prdc_detail_t* detail /* may be NULL */, int device, void* stream);

/* ------------------------------------------------------------------ nearest baseline rows and authenticity (k-NN search)
 * Not in the reference.  For every evaluation row y_j (y [m x d]) its k nearest rows of the baseline x [n x d], 1 <= k <= 16, in
 * ascending order of the key (d^2, i): d^2 is the float32 max(-2 S', 0) that fad_prdc's passes form (|x_i|^2 + |y_j|^2 - 2 x_i.y_j,
 * products on the matrix cores), and equal d^2 are ordered by the smaller index i.  The result is fully determined: the same bits on
 * every run.  index [m x k] (int32) and dist2 [m x k] (float32) are host arrays, row j holding y_j's list.
 * Authenticity (Alaa et al. 2022, "How Faithful is your Synthetic Data?"), when `authenticity` is nonzero: nn(j) is index[j * k],
 * r1^2(i) the squared distance from x_i to its nearest OTHER row of x (fad_prdc's radius with k = 1: self excluded by index, so a
 * duplicate row gives 0); y_j is COPIED when dist2[j * k] <= r1^2(nn(j)).  The test is NON-strict, unlike fad_prdc's strict tests, so
 * an exact copy of a baseline row always counts.  out->copied = the number of copied rows, out->authenticity = 1 - copied / m, and
 * nn_radius2 [m] (host, may be NULL) = r1^2(nn(j)).  Without it the radius pass is skipped, authenticity is NaN, copied is -1 and
 * nn_radius2 is not written.  Rows are float16, bfloat16 or float32, host or device per on_device, 1 <= d <= 2048, ld >= d,
 * n, m < 2^31 - 128.  Argument errors come before any device call: k outside 1 .. 16, a NULL output or an unknown dtype ->
 * FAD_ERR_INVALID; n < k, m < 1, or n < 2 with authenticity -> FAD_ERR_TOO_FEW_ROWS.  A NaN/Inf row norm -> FAD_ERR_NOT_FINITE.
 * Work goes on `stream`; the call synchronises it. */
typedef struct fad_nearest_result {
    double authenticity;
    int64_t n, m, k, copied;
} fad_nearest_result_t;
int fad_nearest(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                int k, int authenticity, int32_t* index, float* dist2, float* nn_radius2 /* may be NULL */, fad_nearest_result_t* out,
                int device, void* stream);

/* ------------------------------------------------------------------ leave-one-out k-NN two-sample test on the pooled rows
 * Not in the reference.  Is y distinguishable from x at all, with no bandwidth to choose?  (Schilling 1986, Henze 1988; the classifier
 * two-sample test of Lopez-Paz & Oquab 2017 with a k-NN classifier.)  Z = [x; y] pooled, N = n + m rows; k odd, 1 <= k <= 15,
 * k <= N - 1.  For every row j of Z, nn(j, 0 .. k-1) are the k rows i != j of Z in ascending order of the key (d^2, i): d^2 is the
 * float32 max(-2 S', 0) that fad_nearest forms, equal d^2 go to the smaller index, and self is excluded by index (a duplicate row is a
 * neighbour at d^2 = 0).  The graph is fully determined and a function of the pooled rows alone.
 * A labelling u is what fad_kad_permutation_test takes: packed bits [n_perm x ceil(N / 32)], exactly n ones, no bit at or past N;
 * labelling 0 is the observed one (Z's first n rows), added by the library.  Under u, row j is PREDICTED BASELINE when more than k / 2
 * of u[nn(j, .)] are 1, and CORRECT when the prediction equals u[j]:
 *   correct_x(u) = #{j correct : u[j] = 1}    correct_y(u) = #{j correct : u[j] = 0}    c(u) = correct_x(u) + correct_y(u)
 *   accuracy = c(u_0) / N      accuracy_x = correct_x(u_0) / n      accuracy_y = correct_y(u_0) / m
 *   p_value     = (1 + #{p : c(u_p) >= c(u_0)}) / (n_perm + 1)      upper tail: distinguishable (accuracy above chance)
 *   p_value_low = (1 + #{p : c(u_p) <= c(u_0)}) / (n_perm + 1)      lower tail: memorised (evaluation rows sit on baseline rows)
 * The counts are compared as integers; both p-values are exact under exchangeability because the graph never sees a label.
 * accuracy_y near 1 with a low accuracy_x: mode collapse; both low: memorisation.  null_correct_x[p] / null_correct_y[p] (host,
 * n_perm entries each) = correct_x / correct_y of the caller's labelling p.  index [N x k] (int32) and dist2 [N x k] (float32), each
 * NULL or an array on the side of the rows (host or device per on_device), hold the graph in ascending key order with Z's row
 * numbering (y_j is row n + j).
 * One pass of fad_nearest's kernel over Z x Z (the full square) finds the graph; all labellings are then classified by one bit-parallel
 * kernel, 32 labellings per word (csrc/nn_vote.h).  Argument errors come before any device call: everything
 * fad_kad_permutation_test refuses about rows and labellings with its codes (n or m < 2 -> FAD_ERR_TOO_FEW_ROWS); k even, outside
 * 1 .. 15 or > N - 1, a NULL out or null array -> FAD_ERR_INVALID.  Device labels with a wrong count -> FAD_ERR_INVALID; a NaN/Inf row
 * norm -> FAD_ERR_NOT_FINITE.  Any refusal leaves every output untouched.  Integers and float32 bits only: the same bits on every run.
 * Workspace: Z's image, the labelling words, N k (4 + 4) bytes of graph and 8 k bytes of keys per row and row range.  Synchronises
 * `stream`. */
typedef struct fad_nn_test_result {
    double accuracy, accuracy_x, accuracy_y, p_value, p_value_low;
    int64_t correct_x, correct_y, n, m;
    int k;
} fad_nn_test_result_t;
int fad_nn_test(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                int k, const uint32_t* labels, int64_t n_perm, int labels_on_device, fad_nn_test_result_t* out,
                int64_t* null_correct_x /* [n_perm] host */, int64_t* null_correct_y /* [n_perm] host */,
                int32_t* index /* [N * k] or NULL */, float* dist2 /* [N * k] or NULL */, int device, void* stream);

/* ------------------------------------------------------------------ kernel distance with the polynomial kernel (KID protocol)
 * Not in the reference.  The unbiased MMD^2 with k(a, b) = (gamma a.b + coef0)^degree -- "KID" / "KD" of the audio evaluation suites
 * at degree 3, gamma = 1 / D, coef0 = 1 (Binkowski et al. 2018) -- over the whole sets (fad_kid) or averaged over many random subsets
 * (fad_kid_subsets: usually 100 subsets of 1000 rows, reported as mean +- std).  degree is 1 .. 4; gamma <= 0 means 1 / d; gamma and
 * coef0 are used as their float32 roundings, and fad_kid's result reports the values actually used.
 *   kxx_mean = sum_{i != j} k(x_i, x_j) / (n (n - 1))    kyy_mean likewise    kxy_mean = sum_{i, j} k(x_i, y_j) / (n m)
 *   mmd2 = kxx_mean + kyy_mean - 2 kxy_mean              (the diagonal of kxx / kyy excluded by index, as fad_kad)
 * Subset q is the rows index_x[q s .. q s + s) of x and index_y[q s .. q s + s) of y (s = subset_size), and
 *   mmd2[q] = Sxx / (s (s - 1)) + Syy / (s (s - 1)) - 2 Sxy / s^2,   Sxx, Syy over i != j, Sxy over all s^2 pairs, its diagonal included
 * -- the usual "unbiased" KID estimator; terms[3 q .. 3 q + 3) = the three means; *mean and *std = the mean and the population
 * standard deviation (ddof = 0; 0 for one subset) of mmd2[].  Repeated indices inside a subset are the caller's business: they are
 * neither checked nor refused (a repeated row pairs with its copy like with any other row).
 * Rows are float16 / bfloat16 / float32 as for fad_kad; the dot products run on the matrix cores into float32, u = fma(S, gamma, coef0)
 * and u^degree in float32, the sums per lane in float32 over one 128 x 128 tile and in float64 from there, in a fixed order: the same
 * bits on every run, and for fad_kid_subsets independent of how the subsets are grouped through the workspace (groups of subsets whose
 * gathered images stay under 128 MiB).  Errors: everything fad_kad_k refuses about rows, with its codes; degree outside 1 .. 4, gamma or
 * coef0 not finite (or outside float32), a NULL output or index, n_subsets < 1, subset_size > min(n, m) -> FAD_ERR_INVALID;
 * subset_size < 2 -> FAD_ERR_TOO_FEW_ROWS; an index outside [0, n) / [0, m) -> FAD_ERR_INVALID (checked on the device before any row
 * is read through it); a kernel sum that is not finite -- NaN/Inf rows, a row whose squared norm overflows float32, or u^degree
 * beyond float32 -- -> FAD_ERR_NOT_FINITE.  Any refusal leaves every output untouched.  Synchronises `stream`. */
typedef struct fad_kid_result {
    double mmd2, kxx_mean, kyy_mean, kxy_mean;
    double gamma, coef0;
    int degree;
    int64_t n, m;
} fad_kid_result_t;
int fad_kid(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
            int degree, double gamma, double coef0, fad_kid_result_t* out, int device, void* stream);
int fad_kid_subsets(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                    int degree, double gamma, double coef0, const int32_t* index_x, const int32_t* index_y,
                    int64_t n_subsets, int64_t subset_size, int index_on_device,
                    double* mmd2 /* [n_subsets] host */, double* terms /* [n_subsets][3]: kxx, kyy, kxy means; may be NULL */,
                    double* mean, double* std /* population, ddof = 0; 0 for one subset */, int device, void* stream);

/* ------------------------------------------------------------------ Sinkhorn divergence between the two sets of rows
 * Not in the reference.  The debiased entropic transport cost between the empirical measures of x [n x d] and y [m x d] (uniform
 * weights 1 / n and 1 / m; Genevay et al. 2018, Feydy et al. 2019), cost C_ij = |x_i - y_j|^2 / 2, regularisation epsilon > 0:
 * non-negative, zero only for equal measures, -> W_2^2 / 2 as epsilon -> 0 and -> |mean x - mean y|^2 / 2 as epsilon -> infinity.
 * One problem OT_eps(x, y) starts from f = 0 [n], g = 0 [m] and runs `iterations` times, in this order (g takes the new f),
 *   f_i <- -eps (LSE_j((g_j - C_ij) / eps) - log m)        g_j <- -eps (LSE_i((f_i - C_ij) / eps) - log n)
 * and its value is mean(f) + mean(g) (after a g step the column marginal holds exactly, so the dual has no correction term).
 *   divergence = ot_xy - ot_xx / 2 - ot_yy / 2       the self problems run the same iteration on (x, x) and (y, y), i = j included
 *   marginal_error = mean_i |exp((f_i - f'_i) / eps) - 1|, f' one more f step that is not adopted: the L1 error of the row marginal
 *                    (marginal_error_xx / _yy: the self problems').  The count is fixed: no early stop; a large value means more
 *                    iterations or a larger epsilon are needed.
 *   detail (may be NULL; each array NULL or host float64): f [n] and g [m] of the (x, y) problem, and the debiased potentials
 *     pot_x[i] = f_i - (f^xx_i + g^xx_i) / 2,  pot_y[j] = g_j - (f^yy_j + g^yy_j) / 2, so that divergence = mean(pot_x) + mean(pot_y):
 *     the mean of pot_y over a song's rows, times its share of the rows, is what that song adds to the divergence.
 * epsilon <= 0 takes (FAD_SINKHORN_BLUR_FACTOR x fad_kad_median_distance(x))^2 (needs n >= 2; a median of 0 -> FAD_ERR_INVALID); the
 * result reports the epsilon used.  Every half-step is one pass of fad_kad_individual's cross kernel over the n x m pair rectangle with
 * a (max, sum of exponentials) epilogue per column, the row potential added to the rows' -|row|^2 / 2: dot products on the matrix cores
 * into float32, the cost matrix never stored, both sets packed once for all iterations of the three problems, potentials kept in
 * float32 between steps and merged in float64, every merge in a fixed order: the same bits on every run, and divergence == 0 exactly
 * for sets of identical bits.  C is formed in float32 from norms and dot products as KAD's d^2 is, so a potential carries an error of
 * about 2^-24 (|x|^2 + |y|^2): rows far from the origin lose digits (centre them first).
 * Rows are float16 / bfloat16 / float32; FAD_F64 -> FAD_ERR_INVALID (cast).  d outside 1 .. 2048, a row pitch < d, iterations outside
 * 1 .. 100000, an epsilon that is NaN / Inf or outside float32, a NULL out -> FAD_ERR_INVALID; n or m < 1 -> FAD_ERR_TOO_FEW_ROWS; a
 * NaN/Inf row norm -> FAD_ERR_NOT_FINITE.  Argument errors come before any device call; any refusal leaves every output untouched.
 * Workspace: the two images; per problem 20 bytes per row of its first set and 12 per row of its second (f, f', g and the two float32
 * vectors); 8 bytes per column and row range of the largest pass.  Synchronises `stream`. */
#define FAD_SINKHORN_BLUR_FACTOR 0.25
typedef struct fad_sinkhorn_result {
    double divergence, ot_xy, ot_xx, ot_yy;
    double epsilon;
    double marginal_error, marginal_error_xx, marginal_error_yy;
    int64_t n, m;
    int iterations;
} fad_sinkhorn_result_t;
typedef struct fad_sinkhorn_detail {
    double* f;        /* [n] */
    double* g;        /* [m] */
    double* pot_x;    /* [n] */
    double* pot_y;    /* [m] */
} fad_sinkhorn_detail_t;
int fad_sinkhorn(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                 double epsilon, int iterations, fad_sinkhorn_result_t* out, fad_sinkhorn_detail_t* detail /* may be NULL */,
                 int device, void* stream);

/* ------------------------------------------------------------------ sliced 2-Wasserstein distance between the two sets of rows
 * Not in the reference.  The transport distance between the empirical measures of x [n x d] and y [m x d] (uniform weights), averaged
 * over L = `projections` one-dimensional projections (Rabin et al. 2011; Bonneel et al. 2015): no blur, no iterations, O((n + m) log)
 * per direction on all rows.  `directions` [L x d] is host float32 and is NOT normalised by the caller or the library: the library
 * rounds it to the rows' dtype (round to nearest even) when it packs it, so that for 16-bit rows every product is exact in float32,
 * and q_l = sum_c theta_lc^2 comes from the rounded values in float64, in index order.  Per direction l, with a = sort(x theta_l),
 * b = sort(y theta_l) and the step quantile functions of the two,
 *   W_l = (1 / q_l) int_0^1 (Fa^-1(t) - Fb^-1(t))^2 dt = S_l / (n m q_l),
 *   S_l = sum over the overlapping (i, j) of w_ij (a_(i) - b_(j))^2,  w_ij = min((i + 1) m, (j + 1) n) - max(i m, j n) > 0, an integer
 * (n == m: S_l = n sum_i (a_(i) - b_(i))^2).
 *   sw2_squared = mean_l W_l;  std_error = std(W_l, ddof = 1) / sqrt(L), NaN for L = 1;  max_sliced = max_l W_l at max_index (the first).
 *   D x sw2_squared reads beside FAD's mean term: a pure translation delta and directions uniform on the sphere give E W_l = |delta|^2 / D.
 *   detail (may be NULL; each array NULL or host): values [L] = W_l; sorted_x [L x n], sorted_y [L x m]: the sorted float32 projections.
 * Arithmetic: projections in float32 on the matrix cores (KAD's main loop, the directions as a third image); a segmented radix sort of
 * the float32 keys (csrc/sliced_sort.h: exact, stable, the same passes whatever the keys, -0 before +0); the difference a - b, its
 * square, the product with the integer weight and every sum in float64, each operation rounded once (no fused multiply-add).  S_l is
 * summed in a fixed order: per element i of the larger set (x when n == m) over its j ascending, then blocks of 256 consecutive i by a
 * halving tree (i += i + 128, i += i + 64, ...), then the blocks in index order.  W_l is one division S_l / ((double)(n m) q_l); the mean
 * (a running sum over l, divided by L), sqrt(sum_l (W_l - mean)^2 / (L - 1)) / sqrt(L) and the maximum are taken on the host in index
 * order.  So: the same bits on every run, whatever the chunking, and for swapped arguments; exactly 0 for sets of identical bits.
 * Rows are float16 / bfloat16 / float32; FAD_F64 -> FAD_ERR_INVALID (cast).  d outside 1 .. 2048, a row pitch < d, projections outside
 * 1 .. 65536, a NULL out or directions, a direction with an entry that is not finite or whose rounded q_l is 0 or not finite,
 * n m >= 2^53 -> FAD_ERR_INVALID; n or m < 1 -> FAD_ERR_TOO_FEW_ROWS; a NaN/Inf row norm or a projection that is not finite in float32
 * -> FAD_ERR_NOT_FINITE.  Argument errors come before any device call; any refusal leaves every output untouched.
 * Workspace: the two images and the directions' ((L rounded up to 128) + 128 rows); then, per direction of a chunk, 4 bytes per padded
 * row of x, of y and of the larger of the two (the sort's second buffer), 1 KiB per 2048 rows of the larger set (counts) and 8 bytes per
 * 256 of them.  Directions are processed in chunks so that this second part stays within 1 GiB (a chunk holds at least one direction).
 * The environment variable FAD_SLICED_WORKSPACE (bytes, read at the start of every call) replaces the 1 GiB: it exists for tests, which
 * force several chunks at small shapes with it.  sorted_x / sorted_y are staged in host memory until the call succeeds.
 * Synchronises `stream`. */
typedef struct fad_sliced_result {
    double sw2_squared, std_error, max_sliced;
    int64_t max_index, n, m;
    int projections;
} fad_sliced_result_t;
typedef struct fad_sliced_detail {
    double* values;      /* [L]      W_l, may be NULL */
    float* sorted_x;     /* [L x n]  may be NULL */
    float* sorted_y;     /* [L x m]  may be NULL */
} fad_sliced_detail_t;
int fad_sliced_wasserstein(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                           int on_device, const float* directions /* host, [L x d] */, int projections,
                           fad_sliced_result_t* out, fad_sliced_detail_t* detail /* may be NULL */, int device, void* stream);

/* ------------------------------------------------------------------ per-song sliced 2-Wasserstein distance against a baseline
 * Not in the reference.  Every song s = rows[offsets[s] .. offsets[s + 1]) (m_s rows) against the baseline x [n x d], in one call: song
 * s gets, bit for bit, what fad_sliced_wasserstein(x, song_s) returns with the same directions -- W_l^s (detail->values, song-major
 * [n_songs x L]), out_sw2, out_std_error, out_max_sliced and out_max_index -- on every run, for any chunking of the directions,
 * wherever the song sits among the rows and whatever its neighbours are.  The same directions, rounding, q_l, float32 projections and
 * float64 match in the same fixed order (the larger of x and song s leads, x at m_s = n; per leading element over its j ascending;
 * blocks of 256 leading elements by the halving tree; the blocks in index order; one division S / ((double)(n m_s) q_l)); the
 * statistics over l in index order on the host.  No floating-point atomics.
 * The baseline is packed once and its projections are sorted once per direction; all song rows are packed once and projected in one
 * launch per chunk; every song of at most C = 4096 rows is sorted inside one workgroup's LDS (csrc/sliced_song_sort.h: units of
 * consecutive songs, at most C keys and 256 songs each, one coalesced read and one coalesced write); longer songs go through
 * csrc/sliced_sort.h's global sort one by one; one workgroup per (direction, song) matches.  The match walks the whole sorted baseline
 * for every song: O(L sum_s max(n, m_s)).
 *   detail (may be NULL; each array NULL or host): values [n_songs x L]; sorted_x [L x n]; sorted_rows [L x n_rows], every song's
 *   range of every direction sorted on its own.
 * out_status[s]: FAD_OK; FAD_ERR_TOO_FEW_ROWS for a song without rows; FAD_ERR_NOT_FINITE for a song with a NaN/Inf row norm or a
 * projection that is not finite in float32 -- both with NaN outputs (values included) and max_index = -1; the other songs do not
 * depend on them.  m_s = 1 is a valid song.
 * Refusals: dtype, d, pitches, projections and directions as fad_sliced_wasserstein; NULL x, offsets, directions or per-song output,
 * NULL rows with n_rows > 0, n_songs < 1, n_rows < 0 or > 2^31 - 129, offsets that do not start at 0, end at n_rows or that decrease,
 * n m_s >= 2^53 for a song -> FAD_ERR_INVALID; n < 1 -> FAD_ERR_TOO_FEW_ROWS; a NaN/Inf baseline row norm or a baseline projection that
 * is not finite -> FAD_ERR_NOT_FINITE.  Argument errors come before any device call; any refusal leaves every output untouched
 * (results are staged in host memory until the call succeeds).
 * Workspace: the two images and the directions'; the song table; then, per direction of a chunk,
 *   4 (n_pad + r_pad + t_pad) + 4 (count_words + 256) + 8 n_songs  bytes,
 * n_pad and r_pad the baseline's and the song rows' counts rounded up to 128, t_pad (the global sort's second buffer) = n_pad, or the
 * larger of n_pad and r_pad when a song has more than C rows, count_words = 256 per 2048 rows of the baseline or of the longest such
 * song, whichever is larger.  Directions go in chunks so that this stays within 1 GiB, or within FAD_SLICED_WORKSPACE bytes (read at
 * the start of every call; for tests); a chunk holds at least one direction.  Synchronises `stream`. */
typedef struct fad_sliced_individual_detail {
    double* values;      /* [n_songs x L]   W_l^s, may be NULL */
    float* sorted_x;     /* [L x n]         may be NULL */
    float* sorted_rows;  /* [L x n_rows]    may be NULL */
} fad_sliced_individual_detail_t;
int fad_sliced_individual(const void* x, int64_t n, int64_t ldx, const void* rows, int64_t n_rows, int64_t ldy,
                          const int64_t* offsets, int64_t n_songs, int64_t d, int dtype, int on_device,
                          const float* directions /* host, [L x d] */, int projections,
                          double* out_sw2, double* out_std_error, double* out_max_sliced, int64_t* out_max_index,
                          int32_t* out_status /* each [n_songs], host */,
                          fad_sliced_individual_detail_t* detail /* may be NULL */, int device, void* stream);

/* ------------------------------------------------------------------ sliced 2-Wasserstein distance: every row's share
 * Not in the reference.  fad_sliced_wasserstein on the same arguments -- the same rounding of the directions, q_l, float32 projections,
 * stable ascending sort (-0 before +0), weights, order of every sum; `out` and detail->values, sorted_x, sorted_y get the bits of that
 * call -- and, for every row of x and of y, its share of sw2_squared: where the distance comes from, on both sides.
 * Per direction l, a = sorted x theta_l, b = sorted y theta_l, rx_l[r] / ry_l[r] = the row of x / y at rank r; equal keys (equal float32
 * bits) stand in ascending row order: the sort is stable, and the tie rule is part of the definition (two rows with equal projections
 * swap partners, so shares are discontinuous at ties).  "Lead" is the larger set (x at n == m), A [na]; the other is B [nb].
 *   lead element at rank i:   c(i) = sum_{j = j0 .. j1} w_ij (A_i - B_j)^2,  j0 = floor(i nb / na), j1 = floor(((i + 1) nb - 1) / na), j ascending
 *                             (the per-element sum of fad_sliced_wasserstein, before its tree)
 *   other element at rank j:  c(j) = sum_{i = i0 .. i1} w_ij (A_i - B_j)^2,  i0 = floor(j na / nb), i1 = floor(((j + 1) na - 1) / nb), i ascending
 *   w_ij = min((i + 1) nb, (j + 1) na) - max(i nb, j na); difference, square, product with the weight and sums in float64, each rounded
 *   once (no fused multiply-add).
 *   t_l(row) = c / ((double)(n m) q_l): one division, by the denominator of W_l.
 *   share[row] = (sum_l t_l(row), l ascending, one running float64 sum carried across the chunks of directions) / L.
 * So sum_rows share_x = sum_rows share_y = sw2_squared up to summation rounding, and n share_x[row] is the row's mean squared
 * one-dimensional displacement.  The same bits on every run and for any chunking; swapped arguments swap the shares; sets of identical
 * bits give shares of exactly 0.  No floating-point atomics: every (direction, row) cost is stored once, and a row's sum has one owner.
 *   share_x [n], share_y [m]: host, required.
 *   detail (may be NULL; each array NULL or host): values, sorted_x, sorted_y as fad_sliced_detail; index_x [L x n], index_y [L x m]:
 *   rx_l and ry_l, so that sorted_x[l][r] is the projection of row index_x[l][r] of x.
 * Refusals: as fad_sliced_wasserstein, and a NULL share_x or share_y -> FAD_ERR_INVALID; any refusal leaves every output untouched
 * (everything is staged in host memory until the call succeeds).
 * Workspace: fad_sliced_wasserstein's and, per direction of a chunk, 4 more bytes per padded row of x, of y and of the larger of the
 * two (the rows at every rank, and the index sort's second buffer: csrc/sliced_sort_pairs.h) and 8 per padded row of x and of y (the
 * costs); chunked under the same 1 GiB or FAD_SLICED_WORKSPACE.  Beside the chunks: 8 bytes per row and per direction.
 * fad_sliced_last_plan reports this call's plan too.  Synchronises `stream`. */
typedef struct fad_sliced_shares_detail {
    double* values;      /* [L]      W_l, may be NULL */
    float* sorted_x;     /* [L x n]  may be NULL */
    float* sorted_y;     /* [L x m]  may be NULL */
    int32_t* index_x;    /* [L x n]  may be NULL */
    int32_t* index_y;    /* [L x m]  may be NULL */
} fad_sliced_shares_detail_t;
int fad_sliced_shares(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                      const float* directions /* host, [L x d] */, int projections, fad_sliced_result_t* out,
                      double* share_x /* host, [n] */, double* share_y /* host, [m] */,
                      fad_sliced_shares_detail_t* detail /* may be NULL */, int device, void* stream);

/* ------------------------------------------------------------------ sliced 2-Wasserstein two-sample permutation test
 * Not in the reference.  "Is y distinguishable from x at all", with the sliced distance as the statistic: no bandwidth, no pair pass.
 * Rows, directions, their rounding to the rows' dtype, q_l and the float32 projections are fad_sliced_wasserstein's.  Z = [x; y],
 * N = n + m.  A labelling u is a 0/1 vector over Z's rows with exactly n ones, given as packed bits in fad_kad_permutation_test's
 * layout (labels [n_perm x ceil(N / 32)] uint32, bit j % 32 of word j / 32 = row j; host or device); the library puts the observed
 * labelling (the first n rows) in front: NL = n_perm + 1 labellings, u_0 the observed one.
 * Per direction l and labelling u: a = the sorted projections of the rows with u = 1, b = those with u = 0,
 *   W_l(u) = S_l(a, b) / ((double)(n m) q_l),
 * S_l exactly as fad_sliced_wasserstein forms it: the same integer weights, float64 with every operation rounded once and no fused
 * multiply-add; the larger group leads (the label-1 group at n == m); per leading element over its j ascending, blocks of 256 by the
 * halving tree, the blocks in index order, one division.  Per labelling, over l in index order as fad_sliced_wasserstein's statistics:
 *   T(u) = mean_l W_l(u)      M(u) = max_l W_l(u)
 *   observed = the fad_sliced_result_t of u_0;  null[p] = T(u_{p+1}),  null_max[p] = M(u_{p+1})   (host, [n_perm], required)
 *   p_value = (1 + #{p : null[p] >= T(u_0)}) / (n_perm + 1);  p_value_max the same with M -- the max-sliced test, sensitive to a
 *   difference that lives in few directions.  Both counts compare float64 values on the host; ties count (>=).
 *   detail (may be NULL; each array NULL or host): values [NL x L], labelling-major, row 0 the observed labelling; sorted_z [L x N] and
 *   index_z [L x N]: the sorted pooled projections and the pooled row at every rank (equal keys in ascending row order).
 * How: the pooled rows are projected and sorted once per direction (csrc/sliced_sort_pairs.h).  A labelling splits that one sorted array
 * into its two sorted groups by a stable compaction (csrc/sliced_split.h: the place of a key is a function of its rank alone), 32
 * labellings per gathered label word; fad_sliced_wasserstein's match and finish kernels then run over the (direction, labelling) pairs
 * as if they were directions.  No sort per labelling.
 * Exactness: the sorted pooled projections and the row indices never see a label, and every labelling, the observed one included, goes
 * through the same kernels.  So under exchangeability of the pooled rows both p-values are exact, whatever float32 rounding did to the
 * projections.
 * Contract: observed and values[0] have the bits of fad_sliced_wasserstein(x, y, directions); values[p] has the bits of
 * fad_sliced_wasserstein(Z[u_p], Z[~u_p], directions), rows taken in ascending pooled order; the same bits on every run, for any
 * chunking of directions and of labelling words, and for swapped arguments with complemented labellings.  No floating-point atomics.
 * Refusals: everything fad_sliced_wasserstein refuses about rows and directions, with its codes; n or m < 1 -> FAD_ERR_TOO_FEW_ROWS;
 * N >= 2^31 - 128, a NULL out, null, null_max or labels, n_perm outside 1 .. 65536, a host labelling whose count of ones is not n or
 * that has a bit at or past N -> FAD_ERR_INVALID, all before any device call; device labellings are checked on the device, with the
 * same code; a NaN/Inf row norm or a projection that is not finite in float32 -> FAD_ERR_NOT_FINITE.  Any refusal leaves every output
 * untouched (results are staged in host memory until the call succeeds).
 * Workspace: Z's image, the directions' and the labellings with their words as fad_kad_permutation_test keeps them; then, per
 * direction of a sort chunk, 16 bytes per padded pooled row (keys, rows, their second buffers) and the sort's counts; per (direction,
 * labelling) pair of a round 4 (n_pad + m_pad) bytes of split keys, 8 per 256 rows of the larger set and 4 per 2048 pooled rows; and
 * 8 L NL bytes of sums.  Sort chunks take a quarter of 1 GiB (or of FAD_SLICED_WORKSPACE), rounds of (directions of the chunk) x
 * (labelling words) the rest; never less than one direction per chunk nor than one direction x one word per round.
 * Synchronises `stream`. */
typedef struct fad_sliced_permutation_result {
    fad_sliced_result_t observed;
    double p_value, p_value_max;
    int64_t permutations;
} fad_sliced_permutation_result_t;
typedef struct fad_sliced_permutation_detail {
    double* values;      /* [NL x L]  W_l(u), labelling-major, may be NULL */
    float* sorted_z;     /* [L x N]   may be NULL */
    int32_t* index_z;    /* [L x N]   may be NULL */
} fad_sliced_permutation_detail_t;
int fad_sliced_permutation_test(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype,
                                int on_device, const float* directions /* host, [L x d] */, int projections,
                                const uint32_t* labels /* [n_perm x ceil(N / 32)] */, int64_t n_perm, int labels_on_device,
                                fad_sliced_permutation_result_t* out, double* null /* [n_perm] host */,
                                double* null_max /* [n_perm] host */, fad_sliced_permutation_detail_t* detail /* may be NULL */,
                                int device, void* stream);

/* ------------------------------------------------------------------ sliced 2-Wasserstein bootstrap
 * Not in the reference.  "How certain is the number": the sliced distance recomputed on resamples of both sets, for an interval on the
 * distance and, with one baseline resampled alike against several sets, on the difference of two distances.  Rows, directions, their
 * rounding to the rows' dtype, q_l and the float32 projections are fad_sliced_wasserstein's.
 * A resample of a set is the set with an integer multiplicity per row: counts_x [n_boot x n] and counts_y [n_boot x m], uint8, host,
 * replicate-major (row counts of a replicate contiguous).  Who draws them decides the resampling unit: rows one by one, or all rows
 * of a file together.  The library puts the all-ones replicate in front: NB = n_boot + 1 replicates, replicate 0 the sets as given.
 * n_b and m_b are the totals of replicate b over x and over y; they differ from replicate to replicate when files are the unit.
 * Per direction l and replicate b: a = the sorted projections of x with the projection of row i taken counts_x[b][i] times, b the same
 * of y,
 *   W_l(b) = S_l(a, b) / ((double)(n_b m_b) q_l),
 * S_l exactly as fad_sliced_wasserstein forms it on sets of n_b and m_b rows: the same integer weights, float64 with every operation
 * rounded once and no fused multiply-add; the larger set leads (x at n_b == m_b); per leading element over its j ascending, blocks
 * of 256 by the halving tree, the blocks in index order, one division.  Per replicate, over l in index order as
 * fad_sliced_wasserstein's statistics:
 *   observed = the fad_sliced_result_t of replicate 0;  boot[b] = mean_l W_l(b + 1),  boot_max[b] = max_l W_l(b + 1)   (host, [n_boot],
 *   required);  replicates = n_boot.  Intervals are the caller's to take from boot (fadtk_amd/sliced.py).
 *   detail (may be NULL; each array NULL or host): values [NB x L], replicate-major, row 0 the sets as given; sorted_x, sorted_y, index_x,
 *   index_y as fad_sliced_shares_detail; totals [NB x 2] int64: n_b, m_b.
 * How: x and y are each projected and sorted once per direction, with the row at every rank (csrc/sliced_sort_pairs.h).  The sorted
 * projections of a resample are that one sorted array with the key at rank r repeated by the count of its row: a stable expansion
 * (csrc/sliced_expand.h: the key at rank r goes to the exclusive prefix sum of the counts over the lower ranks and the places behind
 * it, a function of the rank alone), 4 replicates per gathered word of byte counts.  A match with per-pair sizes then runs over the
 * (direction, replicate) pairs.  No sort per replicate, no gather of rows.
 * Contract: observed and values[0] have the bits of fad_sliced_wasserstein(x, y, directions); values[b] has the bits of
 * fad_sliced_wasserstein(repeat(x, counts_x[b - 1]), repeat(y, counts_y[b - 1]), directions), repeat as numpy.repeat along the rows (rows
 * in ascending order, copies adjacent); the same bits on every run, for any chunking of directions and of replicate words, and for
 * swapped arguments with swapped counts; sets of identical bits with identical counts give exactly 0.  No floating-point atomics.
 * Refusals: everything fad_sliced_wasserstein refuses about rows and directions, with its codes; n or m < 1 -> FAD_ERR_TOO_FEW_ROWS;
 * a NULL counts_x, counts_y, out, boot or boot_max, n_boot outside 1 .. 65536, a replicate whose total over x or over y is 0 or above
 * 2^31 - 129, n_b m_b >= 2^53 for a replicate -> FAD_ERR_INVALID, all before any device call; a NaN/Inf row norm or a projection that
 * is not finite in float32 -> FAD_ERR_NOT_FINITE.  Any refusal leaves every output untouched (results are staged in host memory until
 * the call succeeds).
 * Workspace: the two images and the directions'; 4 bytes per padded row and word of 4 replicates (the count words); then, per direction
 * of a sort chunk, 8 bytes per padded row of x, of y and of the larger of the two (keys, rows, their second buffers) and the sort's
 * counts; per (direction, replicate) pair of a round 4 (xp + yp) bytes of expanded keys, xp and yp the largest n_b and m_b rounded up
 * to 128, 8 per 256 rows of the largest replicate and 4 per 2048 rows of the larger set; and 8 L NB bytes of sums.  Sort chunks take a
 * quarter of 1 GiB (or of FAD_SLICED_WORKSPACE), rounds of (directions of the chunk) x (replicate words) the rest; never less than one
 * direction per chunk nor than one direction x one word per round.  Synchronises `stream`. */
typedef struct fad_sliced_bootstrap_result {
    fad_sliced_result_t observed;
    int64_t replicates;
} fad_sliced_bootstrap_result_t;
typedef struct fad_sliced_bootstrap_detail {
    double* values;      /* [NB x L]  W_l(b), replicate-major, may be NULL */
    float* sorted_x;     /* [L x n]   may be NULL */
    int32_t* index_x;    /* [L x n]   may be NULL */
    float* sorted_y;     /* [L x m]   may be NULL */
    int32_t* index_y;    /* [L x m]   may be NULL */
    int64_t* totals;     /* [NB x 2]  n_b, m_b, may be NULL */
} fad_sliced_bootstrap_detail_t;
int fad_sliced_bootstrap(const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int64_t d, int dtype, int on_device,
                         const float* directions /* host, [L x d] */, int projections,
                         const uint8_t* counts_x /* host, [n_boot x n] */, const uint8_t* counts_y /* host, [n_boot x m] */,
                         int64_t n_boot, fad_sliced_bootstrap_result_t* out, double* boot /* [n_boot] host */,
                         double* boot_max /* [n_boot] host */, fad_sliced_bootstrap_detail_t* detail /* may be NULL */,
                         int device, void* stream);

/* ------------------------------------------------------------------ diagnostics (NOT part of the drop-in surface)
 * Nothing in fadtk corresponds to these two calls and no binding of the reference needs them: they exist for bench.py's
 * roofline object (HIP events around the tile kernel on the stream it is launched on) and for the GPU tests that check
 * which kernel variant ran.
 *
 * Opt-in HIP-event timing (bench.py's roofline): while enabled every update records events around
 * its tile kernel on the caller's stream (no synchronisation); last_timing() returns the AVERAGE
 * duration in ms of the tile kernel and of the reduce kernels over the updates recorded since the
 * last query (at most 256), and which tile kernel ran (0 = fp16/bf16 MFMA on 128 x 128 tiles, 1 = generic fp64,
 * 2 = fp16 MFMA on 256-column slabs, D >= 512).
 * A fad_moments_update_multi call is ONE update recorded on hs[0]: its tile-kernel time covers all sets.
 * enabled = 2 records the two events around the tile kernel only (ms_reduce comes back 0): an event record between two
 * kernels costs the stream a few microseconds, and the one behind the reduce sits in front of whatever the caller
 * enqueues next. */
/* Give back the handle's host-input staging area (and scratch) when it holds more than `keep_bytes`: a handle cached between calls
 * (fadtk_amd/fad.py keeps one per thread) otherwise pins up to 1 GiB of HBM for the life of its thread.  Synchronises the device. */
int fad_moments_trim(fad_moments_t* h, int64_t keep_bytes);
int fad_moments_set_timing(fad_moments_t* h, int enabled);
int fad_moments_last_timing(fad_moments_t* h, float* ms_main_kernel, float* ms_reduce_kernel,
                            int* kernel_variant);

/* Diagnostic: how the last KAD-family call of this thread (fad_kad*, fad_prdc, fad_nearest, fad_nn_test, fad_kid*, fad_sinkhorn) cut its passes into
 * launches (fad_sinkhorn plans each direction of each problem once, 6 passes, and runs that plan at every iteration).  out = { passes planned, launches planned, fewest launches of one pass, most launches of one pass, most slots one
 * workgroup of a launch walks }; all 0 when the call was refused before it planned a pass.  A pass is one walk of a pair space (the
 * median's three histogram rounds share one plan and count once; every word group of a permutation pass is one).  The environment
 * variable FAD_KAD_LAUNCH_BUDGET (cost units per launch, default 2^30, read at the start of every such call; a launch never holds
 * fewer than 64 tiles) exists for tests, which cut small passes into several launches with it. */
int fad_kad_last_plan(int64_t out[5]);

/* Diagnostic: how the last fad_sliced_wasserstein or fad_sliced_shares call of this thread was laid out.  out = { chunks, directions per chunk, sort passes,
 * share }; all 0 when the call was refused before it planned.  share describes the sort of x's segments in a full chunk: W >= 1 when a
 * segment of n keys takes W workgroups (2048 keys each), -G when n <= 256 and one workgroup owns G > 1 segments.  The chunking follows
 * FAD_SLICED_WORKSPACE (above), as fad_kad_last_plan's launch cut follows FAD_KAD_LAUNCH_BUDGET. */
int fad_sliced_last_plan(int64_t out[4]);

/* Diagnostic: how the last fad_sliced_individual call of this thread was laid out.  out = { chunks, directions per chunk, resident
 * units per direction, songs on the long path (more than C rows), most songs in one unit, C }; all 0 when the call was refused
 * before it planned. */
int fad_sliced_individual_last_plan(int64_t out[6]);

/* Diagnostic: how the last fad_sliced_permutation_test call of this thread was laid out.  out = { sort chunks, directions per sort
 * chunk, pair rounds in all, directions per round, labelling words per round, share }; all 0 when the call was refused before it
 * planned.  share is fad_sliced_last_plan's, of the pooled rows' segments in a full sort chunk. */
int fad_sliced_permutation_last_plan(int64_t out[6]);

/* Diagnostic: how the last fad_sliced_bootstrap call of this thread was laid out.  out = { sort chunks, directions per sort chunk,
 * rounds in all, directions per round, replicate words per round, replicates per word }; all 0 when the call was refused before it
 * planned. */
int fad_sliced_bootstrap_last_plan(int64_t out[6]);

/* Lloyd's k-means on the pooled rows of 1 .. 8 row sets, the quantisation under MAUVE and PRD curves
 * (fadtk_amd/mauve.py).  xs / ns / lds: the sets' rows, row counts and row pitches (the list form of fad_kad_uncertainty), all of one
 * dtype (float16, bfloat16 or float32), all host or all device; they are pooled in the given order, N rows in all, 1 <= D <= 2048,
 * ld >= D.  1 <= K <= min(N, 65536).  init [K x D] float32 (host, required: seeding is the caller's), max_iter >= 0.
 *   Assignment A(C): row i takes the centroid with the smallest key (d^2, index): d^2 is fad_nearest's float32 max(-2 S', 0), formed
 *     against the float32 centroid (16-bit rows: the centroid enters the main loop as 2 (float16) or 3 (bfloat16) planes of the rows'
 *     dtype whose sum is the float32 value; h_c = -|c|^2 / 2 from the float32 values); equal d^2 go to the smaller index.
 *   Update M(A): c_k = float32(sum of the rows of cluster k in float64 / count_k); a cluster without rows keeps its centroid.
 *   Loop, t = 1 .. max_iter: A_t = A(C_{t-1}); if t > 1 and A_t = A_{t-1}, stop with converged = 1; else C_t = M(A_t).  If the loop
 *     runs out (and for max_iter = 0, a pure assignment against init) the labels are one more assignment against the last centroids,
 *     so labels, dist2, counts and inertia always belong to the returned centroids.
 * Outputs (host): centroids [K x D] float32, labels [N] int32 in pooled order, counts [K] int64, dist2 [N] float32 (may be NULL),
 * inertia_trace [max_iter + 1] (may be NULL): the float64 sum of dist2 in a fixed order after every assignment made, `assignments`
 * values.  iterations: the t at which the loop stopped (max_iter when it ran out); changed_last: the labels that differed at the
 * last comparison of two assignments (-1 when none was made); empty_clusters: the clusters without a row under the returned labels.
 * No floating-point atomics: the same bits on every run and under every launch cut.  Refusals (outputs untouched): FAD_ERR_INVALID
 * for bad shapes, K or max_iter, FAD_ERR_TOO_FEW_ROWS for an empty set, FAD_ERR_NOT_FINITE for a row or an init centroid that is not
 * finite (a float32 init entry past the range of float16 rows included). */
typedef struct fad_kmeans_result {
    double inertia;
    int64_t n, k, iterations, converged, changed_last, empty_clusters, assignments;
} fad_kmeans_result_t;
int fad_kmeans(const void* const* xs, const int64_t* ns, const int64_t* lds, int n_sets, int64_t d, int dtype, int on_device, int64_t k,
               const float* init, int max_iter, float* centroids, int32_t* labels, int64_t* counts, float* dist2, double* inertia_trace,
               fad_kmeans_result_t* out, int device, void* stream);

/* Diagnostic: how the last fad_kmeans call of this thread ran.  out = { planes of the centroid operand, launches of the last
 * assignment, rows per update chunk, most chunks one cluster took in the last update, iterations, assignments made }; all 0 when the
 * call was refused before it ran. */
int fad_kmeans_last_plan(int64_t out[6]);

/* A HIP stream confined to a subset of the device's CUs (hipExtStreamCreateWithCUMask; `mask` = `words` x 32 bits, bit i = CU i in
 * the runtime's numbering, which on this 8-XCD part walks the XCDs first: bit i -> XCD i % 8).  bench.py's --chain-cus layout
 * experiment puts the square-root chains and the moments kernels on disjoint CU sets with it; nothing in the library uses it.
 * The stream is the caller's (destroy with fad_stream_destroy); `*stream` is a hipStream_t. */
int fad_stream_create_cu_mask(int device, const uint32_t* mask, int words, void** stream);
int fad_stream_destroy(int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FAD_HIP_H */
