// Running (n, sum x, sum x x^T) of frame matrices E[N x D]  -- gfx950 / CDNA4 only.
//
// Replaces np.mean + np.cov of fadtk/fad.py:48 and the per-file np.cov + merge loop of
// fadtk/utils.py:13-45 by ONE pass over E that accumulates raw moments (sum-reducible).
//
// Kernels
//   moments_tile_h16_tr    fp16/bf16 rows -> fp32 partial tiles of E^T E with v_mfma_f32_32x32x16_{f16,bf16}
//                          (fp16 x fp16 products are exact in fp32; each workgroup sums a bounded run of rows in
//                          fp32, the partials are combined in fp64).  Only upper-triangular 128x128 tiles are
//                          computed (E^T E is symmetric); column sums ride along on the diagonal tiles.
//                          ONE launch serves up to kMaxSets frame matrices ("sets": the two datasets of a FAD
//                          score, the resamples of score_inf ...): the workgroup slots of the chip are shared
//                          out over all sets, so every workgroup sums a longer run of rows and the per-workgroup
//                          costs (a 64 KiB partial tile written and re-read, pipeline fill, launch) are paid once
//                          for all of them.
//   moments_tile_f64       any dtype / any alignment -> fp64 partial tiles with v_mfma_f64_16x16x4_f64
//                          (products and sums in fp64, like np.cov); also the exact redo of the shift guard.
//   moments_reduce         partials (fp32|fp64) -> += packed fp64 accumulator, mirrored; all sets in one launch.
//   moments_finalize       (n, sum, sumsq) -> mu, cov with ddof.
// (Earlier generations of the tile kernel, and the one-tile-per-wave kernel shipped through round 2:
//  scripts/probes/moments_generations.hip.)
//
// Data layout in HBM
//   E            row-major [N x ld], one frame per row (the layout of fadtk's .npy files)
//   accumulator  packed fp64 [ n | sum_x[D] | sum_xxT[D*D] ]
//   partials     [split][tile][BT][BT]   (BT = 128 fp32 | 64 fp64), fragment-major inside a 128x128 tile
//   colpart      [split][nt*BT] fp64
#include "fad_common.h"
#include <hip/hip_ext.h>
#include "moments_kernels.h"
#include "moments_tile256.h"
#include <dlfcn.h>
#include <vector>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>

// ==========================================================================================
// handle + host side
// ==========================================================================================
struct fad_moments {
    int d = 0, device = 0;
    double* acc = nullptr;                 // packed [1 + d + d*d]
    bool owns_acc = true;                  // false after fad_moments_bind: the caller's buffer
    fad::DevBuf partials, colpart, stage, seg_tab, seg_piece, seg_out, scratch;
    fad::DevBuf partials64, colpart64;     // exact fp64 redo of a block flagged by the shift guard
    fad::DevBuf cvec;                      // float16 rows: per-split column shifts for the guard's second pass
    fad::DevBuf presum, presum_col;        // stage-1 output of the two-level reduce
    fad::DevBuf blocktab;                  // 256-column-slab kernel: where every 32 x 32 block's partial sums sit (tile256_roles.h)
    int blocktab_nsb = 0;
    bool ref_mean = false;                 // fad_moments_set_reference_mean: keep numpy's float32 running column sums beside the exact ones
    fad::DevBuf runsum;                         // ... [d] floats
    bool runsum_covers = true;             // ... they cover exactly the rows the accumulator holds (an empty handle: trivially)
    bool runsum_live = false;              // ... a running-sum kernel has written them since the handle was created / reset
    fad::DevBuf seg_run, seg_off, seg_jobs;   // per-file running sums (fad_moments_update_segmented_ref), the offsets they are walked by, the walk's job table
    hipEvent_t rs_fork = nullptr, rs_join = nullptr;   // ... the walk runs on the device's side stream between these two (running_sums)
    hipStream_t cp_st = nullptr;           // host rows in pieces: the copies run on this stream, ahead of the caller's (update_any)
    hipEvent_t cp_enter = nullptr, cp_ev[8] = {};
    bool ref_detached = false;             // fad_moments_set_reference_mean(h, 2): the walk neither waits for the caller's stream nor holds it up
    hipEvent_t rs_pending = nullptr;       // ... the library's event behind the handle's last detached walk: settle() makes a reader's stream wait for it
    hipEvent_t rs_reader = nullptr;        // ... and the handle's own event behind its last ASYNCHRONOUS reader (moments_mark_read): the next detached walk,
    bool rs_reader_set = false;            //     which rewrites the running sums on the side stream, waits for it
    hipEvent_t rs_caller = nullptr;        // ... and the handle's own event behind its last walk on the CALLER's stream (unaligned rows, bfloat16, float32):
    bool rs_caller_set = false;            //     the next detached walk continues that walk's carry, so it waits for it as well
    bool staged_input = false;             // update_any is feeding host rows through the staging area: no detached walk over those
    int tile256 = 1;                       // 0: FAD_MOMENTS_TILE256=0 (read at creation) keeps D >= 512 on the 128 x 128 kernel
    // the segment tables of the last fused update_segmented call, kept on the host: a caller feeding groups of the SAME file sizes
    // (30-second clips: every file 2250 frames) finds them on the device already -- no H2D copy in front of the tile kernel
    std::vector<int64_t> seg_cached_offsets; int64_t seg_cached_n = -1; int seg_cached_S = 0; int64_t seg_cached_runs = 0, seg_cached_max = 0;
    size_t seg_cached_bytes_runs = 0, seg_cached_bytes_first = 0;
    std::vector<int64_t> sizes_cached; const void* sizes_cached_at = nullptr;      // ... and the sizes of update_file_means (in `scratch`)
    void* tab_host = nullptr; size_t tab_host_cap = 0;     // pinned staging of the segment tables of update_segmented
    hipEvent_t tab_ev = nullptr;           // recorded behind the upload of tab_host: the next call waits before rewriting it
    int* shift_flag = nullptr;             // device int[2], ping-pong between updates
    unsigned update_seq = 0;
    int guard = 1;                         // 0 disables the guard (FAD_MOMENTS_SHIFT_GUARD=0, read at creation)
    bool force_generic = false;            // FAD_MOMENTS_FORCE_GENERIC=1 (read at creation): always the fp64 kernel
    bool fresh = false;                    // reset since the last update: the next reduce stores instead of adding
    // opt-in HIP-event timing: a ring of (before tile kernel, after tile kernel, after reduce) triplets,
    // recorded on the caller's stream and only read back by fad_moments_last_timing (no sync in update)
    static constexpr int kRing = 256;
    int timing = 0;                        // 0 off, 1 all three events, 2 tile kernel only (no event behind the reduce)
    hipEvent_t* ev = nullptr;              // [kRing][3]
    int ev_count = 0;                      // entries recorded since the last query
    int last_variant = -1;                 // 0: h16 MFMA 128 x 128 tile kernel, 1: generic fp64 kernel, 2: h16 MFMA 256-column-slab kernel
    int last_sets = 1;                     // frame matrices the last timed launch covered
    int n_cu = 256;
};

namespace fad {

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return FAD_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 4;
    if (hipMalloc(&p, want) != hipSuccess) {
        p = nullptr;
        return set_error(FAD_ERR_ALLOC, "hipMalloc of %zu bytes failed", want);
    }
    cap = want;
    return FAD_OK;
}
void DevBuf::release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }

static int64_t packed_len(int d) { return 1 + (int64_t)d + (int64_t)d * d; }

// The dynamic-LDS limit of the fp16 tile kernels is a per-device function attribute: set it once per device,
// under a lock (two host threads may make their first update on different GPUs at the same time).
typedef void (*tile_kernel_t)(TileLaunch);
static tile_kernel_t tr_kernel_shift(bool fast) {          // second pass of the shift guard (float16 rows only)
    return fast ? &moments_tile_h16_tr<FAD_F16, H_NST, true, true> : &moments_tile_h16_tr<FAD_F16, 2 * H_NST, false, true>;
}
static tile_kernel_t tr_kernel_walk(int dtype, bool fast) {  // first pass + the per-file float32 running sums (file-aligned splits, one run per file)
    if (dtype == FAD_F16) return fast ? &moments_tile_h16_tr<FAD_F16, H_NST, true, false, true> : &moments_tile_h16_tr<FAD_F16, 2 * H_NST, false, false, true>;
    return fast ? &moments_tile_h16_tr<FAD_BF16, H_NST, true, false, true> : &moments_tile_h16_tr<FAD_BF16, 2 * H_NST, false, false, true>;
}
static tile_kernel_t tr_kernel(int dtype, bool fast) {       // multi-tile: 4 stages of 16 KiB; single tile: 8 stages of 8 KiB
    if (dtype == FAD_F16) return fast ? &moments_tile_h16_tr<FAD_F16, H_NST, true> : &moments_tile_h16_tr<FAD_F16, 2 * H_NST, false>;
    return fast ? &moments_tile_h16_tr<FAD_BF16, H_NST, true> : &moments_tile_h16_tr<FAD_BF16, 2 * H_NST, false>;
}
constexpr size_t kTrLds = (size_t)H_NST * 2 * H_KB * 16 * sizeof(uint4);
static int ensure_kernel_attrs(int device) {
    static std::mutex mu;
    static bool done[64] = {false};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= 64) return set_error(FAD_ERR_INVALID, "device %d out of range", device);
    if (done[device]) return FAD_OK;
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_tile256<FAD_F16, false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kT256Lds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_tile256<FAD_F16, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kT256Lds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_tile256<FAD_F16, false, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kT256Lds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_tile256<FAD_F16, true, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kT256Lds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum_h16<16, 192, 4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRsLds));
    for (int dt : {FAD_F16, FAD_BF16}) {
        for (bool fast : {false, true}) {
            FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tr_kernel_walk(dt, fast)),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrLds));
            FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tr_kernel(dt, fast)),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrLds));
            if (dt == FAD_F16)
                FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tr_kernel_shift(fast)),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrLds));
        }
    }
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum_h16<16, 192, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRsLds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum<raw_f16, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum<raw_f16, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum<raw_bf16, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum<raw_bf16, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum<float, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLds));
    FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&moments_running_colsum<float, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRunLds));
    done[device] = true;
    return FAD_OK;
}

// Split plan of one launch over `count` frame matrices of n[i] rows: every workgroup sums a run of `r` rows of one
// tile of one set, the same r for all sets.  r is the SMALLEST run (multiple of kb, >= min_rows) for which the work
// items fit into R "rounds" of the resident workgroup slots (n_cu * wg_per_cu), R being the number of rounds the
// longest allowed run needs -- one, unless max_rows forces more items than slots: then the items are sized to fill R
// whole rounds instead of leaving a nearly empty last one (4 x [100k x 512]: 520 items at r = 8192 took two rounds of
// 8192 rows; 1000 items of 4000 rows take two rounds of 4000).
// max_rows bounds the run of rows one workgroup sums in fp32 (0 = unbounded): the MFMA accumulate error is systematic
// (it behaves like truncation): measured -3.5e-7 relative at 32768 rows per run, ~1e-8 per 1000 rows, so runs are
// capped at 8192 rows and long inputs simply use more splits than resident slots.
static void plan_splits(int count, const int64_t* n, int d, int bt, int kb, int n_cu, int wg_per_cu, int64_t min_rows,
                        int64_t max_rows, SplitPlan* out, int items_per_split = 0) {
    const int nt = (int)cdiv(d, bt), T = items_per_split > 0 ? items_per_split : nt * (nt + 1) / 2;
    const int64_t slots = (int64_t)n_cu * wg_per_cu;
    int64_t total = 0, longest = 1;
    for (int i = 0; i < count; ++i) { total += n[i]; if (n[i] > longest) longest = n[i]; }
    auto items = [&](int64_t r) { int64_t w = 0; for (int i = 0; i < count; ++i) w += cdiv(n[i], r); return w * T; };
    int64_t r_cap = cdiv((max_rows > 0 && max_rows < longest) ? max_rows : longest, kb) * kb;
    if (max_rows > 0 && r_cap > max_rows) r_cap = (max_rows / kb) * kb;
    if (r_cap < kb) r_cap = kb;
    const int64_t rounds = cdiv(items(r_cap), slots);
    int64_t r = cdiv(cdiv(total * T, rounds * slots), kb) * kb;
    const int64_t r_min = cdiv(min_rows, kb) * kb;
    if (r < r_min) r = r_min;
    while (r < r_cap && items(r) > rounds * slots) r += kb;
    if (r > r_cap) r = r_cap;
    for (int i = 0; i < count; ++i) {
        out[i].nt = nt; out[i].T = T;
        out[i].rows_per_split = r;
        out[i].S = (int)cdiv(n[i], r);
        if (out[i].S < 1) out[i].S = 1;
    }
}

static int timing_events(fad_moments* h, hipEvent_t** ev) {
    *ev = nullptr;
    if (!h->timing) return FAD_OK;
    if (!h->ev) {
        h->ev = new (std::nothrow) hipEvent_t[fad_moments::kRing * 3]();
        if (!h->ev) return set_error(FAD_ERR_ALLOC, "out of host memory");
        for (int i = 0; i < fad_moments::kRing * 3; ++i) FAD_HIP_TRY(hipEventCreate(&h->ev[i]));
    }
    *ev = h->ev + 3 * (h->ev_count % fad_moments::kRing);
    h->ev_count++;
    return FAD_OK;
}

template <typename TIn>
static void launch_generic(const TileLaunch& L, int max_items, hipStream_t st) {
    hipLaunchKernelGGL((moments_tile_f64<TIn>), dim3((unsigned)max_items, (unsigned)L.nsets), dim3(256), 0, st, L);
}
static int launch_generic_dtype(const TileLaunch& L, int max_items, int dtype, hipStream_t st) {
    switch (dtype) {
        case FAD_F16: launch_generic<raw_f16>(L, max_items, st); break;
        case FAD_BF16: launch_generic<raw_bf16>(L, max_items, st); break;
        case FAD_F32: launch_generic<float>(L, max_items, st); break;
        case FAD_F64: launch_generic<double>(L, max_items, st); break;
        default: return set_error(FAD_ERR_INVALID, "unknown dtype %d", dtype);
    }
    return FAD_OK;
}

// Segment-aligned splits of ONE set (fad_moments_update_segmented on long files): device tables + counts.
struct SegPlan {
    const SegRun* runs; const int* split_first_run;   // device
    int n_runs, S;
    int64_t max_split_rows;
    float* seg_runsum = nullptr;                      // device [n_segments][d]: the tile kernel walks numpy's per-file running sums as well
};

// Pinned host staging for the small tables update_segmented uploads (no pageable copy, no stream sync): the buffer is
// reused by the next call, which first waits for the event recorded behind this call's upload.
static int stage_tables(fad_moments* h, size_t bytes, char** host) {
    if (!h->tab_ev) FAD_HIP_TRY(hipEventCreateWithFlags(&h->tab_ev, hipEventDisableTiming));
    else FAD_HIP_TRY(hipEventSynchronize(h->tab_ev));
    if (bytes > h->tab_host_cap) {
        if (h->tab_host) (void)hipHostFree(h->tab_host);
        h->tab_host = nullptr; h->tab_host_cap = 0;
        FAD_HIP_TRY(hipHostMalloc(&h->tab_host, bytes + bytes / 4 + 4096, hipHostMallocDefault));
        h->tab_host_cap = bytes + bytes / 4 + 4096;
    }
    *host = static_cast<char*>(h->tab_host);
    return FAD_OK;
}


// ------------------------------------------------------------------------------------------
// D >= 512, float16 rows: the 256-column-slab kernel (moments_tile256.h).  Same three launches as the 128 x 128 path -- tile
// kernel, gated second pass of the shift guard, reduce -- with ONE workgroup per CU and work items of 64-72 blocks.
// ------------------------------------------------------------------------------------------
static int block_table(fad_moments* h, int nsb, hipStream_t st) {
    if (h->blocktab_nsb == nsb) return FAD_OK;
    // host copies live for the life of the process: the upload below reads them asynchronously
    static std::mutex mu;
    static std::vector<t256::BlockSrc>* cache[t256::MAX_SB + 1] = {nullptr};
    const std::vector<t256::BlockSrc>* tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!cache[nsb]) {
            auto* v = new (std::nothrow) std::vector<t256::BlockSrc>((size_t)t256::n_blocks(t256::NFR * nsb));
            if (!v) return set_error(FAD_ERR_ALLOC, "out of host memory");
            if (!t256::build_block_table(nsb, v->data())) { delete v; return set_error(FAD_ERR_INVALID, "block table of %d superblocks is inconsistent", nsb); }
            cache[nsb] = v;
        }
        tab = cache[nsb];
    }
    const size_t bytes = tab->size() * sizeof(t256::BlockSrc);
    FAD_TRY(h->blocktab.reserve(bytes));
    FAD_HIP_TRY(hipMemcpyAsync(h->blocktab.p, tab->data(), bytes, hipMemcpyHostToDevice, st));
    h->blocktab_nsb = nsb;
    return FAD_OK;
}

static bool tile256_eligible(const fad_moments* h0, int count, const int64_t* n, const int64_t* ld, int dtype, bool aligned, bool seg) {
    const int d = h0->d;
    if (!h0->tile256 || !aligned || seg || dtype != FAD_F16 || h0->force_generic) return false;
    if (d < 2 * t256::SB || d > t256::MAX_SB * t256::SB) return false;
    for (int i = 0; i < count; ++i) if (n[i] < 16 * (int64_t)d) return false;      // (what the guard's second pass asks for as well)
    // the kernel addresses the rows of a split (<= 8192 + 64) through a buffer resource with 32-bit offsets below 2^31
    for (int i = 0; i < count; ++i) if (ld[i] >= ((int64_t)1 << 16)) return false;
    return true;
}

static int update_tile256(int count, fad_moments* const* hs, const void* const* rows, const int64_t* n, const int64_t* ld,
                          hipStream_t st, hipEvent_t* ev, const int32_t* const* idx = nullptr, int64_t n_src = 0) {
    fad_moments* h0 = hs[0];
    const int d = h0->d, nsb = (int)cdiv(d, t256::SB), dpad = nsb * t256::SB;
    FAD_TRY(ensure_kernel_attrs(h0->device));
    T256Launch L;
    memset(&L, 0, sizeof(L));
    L.nsets = count; L.d = d; L.nsb = nsb;
    L.NT = t256::item_types(nsb, L.type, L.sa, L.sb);
    const bool has_z = (nsb & 1) != 0;
    const size_t lds_bytes = kT256Lds;
    SplitPlan plan[kMaxSets256];
    plan_splits(count, n, d, t256::SB, has_z ? 2 * T2_KB : T2_KB, h0->n_cu, 1, 256, 8192, plan, L.NT);
    FAD_TRY(block_table(h0, nsb, st));
    R256Launch R;
    memset(&R, 0, sizeof(R));
    R.table = static_cast<const t256::BlockSrc*>(h0->blocktab.p);
    R.d = d; R.nsb = nsb; R.NT = L.NT; R.nblk = t256::n_blocks(t256::NFR * nsb);
    R.two_mask = (nsb & 1) ? (1u << (nsb - 1)) : 0u;
    int item = 0, max_s = 0;
    bool any_guard = false;
    for (int i = 0; i < count; ++i) {
        fad_moments* h = hs[i];
        const SplitPlan& p = plan[i];
        FAD_TRY(h->partials.reserve((size_t)p.S * L.NT * t256::ITEM_STRIDE * sizeof(float)));
        FAD_TRY(h->colpart.reserve((size_t)p.S * 2 * dpad * sizeof(double)));
        T256Set& s = L.set[i];
        s.E = rows[i]; s.n = n[i]; s.ld = ld[i]; s.rows_per_split = p.rows_per_split; s.S = p.S; s.item0 = item;
        s.partials = static_cast<float*>(h->partials.p); s.colpart = static_cast<double*>(h->colpart.p);
        s.flag = nullptr; s.cvec = nullptr;
        s.idx = idx ? idx[i] : nullptr; s.n_src = n_src;
        R256Job& j = R.job[i];
        if (h->guard) {
            FAD_TRY(h->cvec.reserve((size_t)p.S * dpad * sizeof(uint16_t)));
            s.cvec = static_cast<uint16_t*>(h->cvec.p);
            s.flag = h->shift_flag + (h->update_seq & 1u);
            j.clear_flag = h->shift_flag + ((h->update_seq + 1u) & 1u);
            h->update_seq++;
            j.gate = s.flag; j.cvec = s.cvec;
            any_guard = true;
        }
        j.partials = s.partials; j.colpart = s.colpart;
        j.acc = h->acc; j.n_add = (double)n[i]; j.overwrite = h->fresh ? 1 : 0;
        j.S = p.S; j.rows_per_split = p.rows_per_split; j.n_rows = n[i];
        if (p.S > max_s) max_s = p.S;
        item += p.S * L.NT;
        h->last_variant = 2;
    }
    L.total = item;
    // timing: the two events take the dispatch's OWN begin / end stamps (what rocprofv3 reports for the kernel), not the stream's
    // idle-to-idle interval -- with several streams in flight an event recorded ahead of the launch also counts the time the
    // dispatch waits for another stream's workgroups to leave the CUs
    if (idx) {           // gathered rows (fad_moments_update_multi_indexed): the same kernels, the row of every LDS-DMA piece from the index
        if (ev) hipExtLaunchKernelGGL((moments_tile256<FAD_F16, false, true>), dim3((unsigned)L.total), dim3(512), (uint32_t)lds_bytes, st, ev[0], ev[1], 0u, L);
        else hipLaunchKernelGGL((moments_tile256<FAD_F16, false, true>), dim3((unsigned)L.total), dim3(512), lds_bytes, st, L);
        if (any_guard) hipLaunchKernelGGL((moments_tile256<FAD_F16, true, true>), dim3((unsigned)L.total), dim3(512), lds_bytes, st, L);
    } else {
    if (ev) hipExtLaunchKernelGGL((moments_tile256<FAD_F16, false>), dim3((unsigned)L.total), dim3(512), (uint32_t)lds_bytes, st, ev[0], ev[1], 0u, L);
    else hipLaunchKernelGGL((moments_tile256<FAD_F16, false>), dim3((unsigned)L.total), dim3(512), lds_bytes, st, L);
    if (any_guard)       // second pass of the shift guard: same geometry, gated per set; rewrites the flagged sets' partials and column sums
        hipLaunchKernelGGL((moments_tile256<FAD_F16, true>), dim3((unsigned)L.total), dim3(512), lds_bytes, st, L);
    }
    // split lanes per output group: one thread walks all splits of its four outputs with eight loads in flight.  Measured
    // (guard + reduce): 2 sets x 43 splits 22.2 / 22.8 / 22.3 / 23.3 / 26.1 us at 1 / 2 / 4 / 8 / 16 lanes,
    // 8 sets x 10 splits 26.5 / 28.3 / 32.3 / 37.6 / 58.9 us -- the LDS combine and the extra threads cost more than the shorter walks save.
    R.sl = (max_s > 128) ? 4 : 1;
    const int G = 256 / R.sl;
    const int blocks = (int)cdiv((int64_t)R.nblk * 256, G) + (int)cdiv(d, 64);
    // 8 KiB of dynamic LDS the kernel never touches: 10 instead of 20 of its workgroups per CU.  Measured at config 3
    // (scripts/probes/tile256_overlap.hip): tile + reduce 92 -> 84 us per update with 4-12 KiB of padding, 86 with 20 KiB;
    // D = 768 / 1024 within 1 %.
    hipLaunchKernelGGL(moments_reduce256, dim3((unsigned)blocks, (unsigned)count), dim3(256), 8192, st, R);
    if (ev && h0->timing == 1) FAD_HIP_TRY(hipEventRecord(ev[2], st));
    FAD_HIP_TRY(hipGetLastError());
    for (int i = 0; i < count; ++i) hs[i]->fresh = false;
    return FAD_OK;
}

// One pass over `count` frame matrices (DEVICE pointers), all of the handles' dimension, dtype and device:
// tile kernel (one launch for all sets) -> gated fp64 redo (one launch) -> reduce (one launch).
// `seg` (count == 1, fp16/bf16 aligned input only): segment-aligned splits; colpart then has one row per run.
// numpy's float32 running column sums (moments_kernels.h: moments_running_colsum) for the handles that asked for them: one launch for
// all of them, in front of the update's other kernels (float64 frames: numpy's sum is the exact one to 1e-16 -- nothing to do)
// The walk's stream: one per device (high priority: its 32 workgroups per matrix should be placed before the tile kernel's fill the
// chip; they fit BESIDE a tile workgroup).  nullptr if the stream cannot be created: the walk then runs on the caller's stream.
static hipStream_t runsum_side_stream(int device) {
    static std::mutex mu;
    static hipStream_t side[64] = {nullptr};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= 64) return nullptr;
    if (!side[device]) {
        // (a CU-masked stream -- hipExtStreamCreateWithCUMask -- would keep the walk off some CUs, but it is a BLOCKING stream: it would
        //  synchronise with the legacy default stream most callers launch on.  The walk leaves CUs free by its grid instead: 16 workgroups
        //  per matrix, moments_kernels.h.)
        hipStream_t st = nullptr;
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; hi = 0; }
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi) != hipSuccess) { st = nullptr; (void)hipGetLastError(); }
        side[device] = st;
    }
    return side[device];
}

// Events behind DETACHED walks: a ring per device, owned by the library for the life of the process (a handle only borrows the pointer;
// a re-recorded event stands for a LATER point of the in-order side stream, so waiting for it is still enough).
static hipEvent_t runsum_ring_event(int device) {
    static std::mutex mu;
    static hipEvent_t ring[64][32] = {{nullptr}};
    static unsigned next[64] = {0};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= 64) return nullptr;
    hipEvent_t& e = ring[device][next[device]++ & 31u];
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; (void)hipGetLastError(); }
    return e;
}

// The float16 walk (moments_kernels.h): 16 columns per workgroup.
static void launch_runsum_h16(const RunSumLaunch& L, int jobs, hipStream_t st, bool indexed = false) {
    if (indexed)
        hipLaunchKernelGGL((moments_running_colsum_h16<16, 192, 4, true>), dim3((unsigned)cdiv(L.d, 16), (unsigned)jobs), dim3(256), (RsShape<16, 192, 4>::lds), st, L);
    else
        hipLaunchKernelGGL((moments_running_colsum_h16<16, 192, 4>), dim3((unsigned)cdiv(L.d, 16), (unsigned)jobs), dim3(256), (RsShape<16, 192, 4>::lds), st, L);
}

// -> *joined: an event the caller's stream has to wait for before the update returns (the walk reads the caller's rows), or nullptr
static int running_sums(int count, fad_moments* const* hs, const void* const* rows, const int64_t* n, const int64_t* ld, int dtype,
                        hipStream_t st, hipEvent_t* joined, const int32_t* const* idx = nullptr) {
    *joined = nullptr;
    if (dtype == FAD_F64) {                                          // (numpy's float64 sum IS the exact one to 1e-16: finalize takes that)
        for (int i = 0; i < count; ++i)
            if (n[i] > 0) hs[i]->runsum_covers = false;
        return FAD_OK;
    }
    RunSumLaunch L;
    memset(&L, 0, sizeof(L));
    int m = 0;
    for (int i = 0; i < count; ++i) {
        fad_moments* h = hs[i];
        if (n[i] <= 0) continue;
        if (h->fresh) h->runsum_covers = true;                      // (reset: both are empty again)
        if (!h->ref_mean) { h->runsum_covers = false; continue; }   // rows the running sums will never see
        if (!h->runsum_covers) continue;                            // (imported / exchanged statistics: the order is lost for good)
        FAD_TRY(h->runsum.reserve((size_t)h->d * sizeof(float)));
        RunSumJob& j = L.job[m++];
        j.rows = rows[i]; j.n = n[i]; j.ld = ld[i]; j.run = static_cast<float*>(h->runsum.p);
        j.idx = idx ? idx[i] : nullptr;
        j.start_zero = (h->fresh || !h->runsum_live) ? 1 : 0;        // (a new handle is empty without having been reset: its buffer is not)
        h->runsum_live = true;
    }
    if (!m) return FAD_OK;
    fad_moments* h0 = hs[0];
    L.d = h0->d;
    FAD_TRY(ensure_kernel_attrs(h0->device));
    const dim3 grid((unsigned)cdiv(L.d, kRunCols), (unsigned)m);
    const size_t es = dtype_size(dtype);
    bool wide = (L.d % (int)(16 / es)) == 0;
    for (int i = 0; i < m && wide; ++i)
        wide = ((reinterpret_cast<uintptr_t>(L.job[i].rows) & 15u) == 0) && ((L.job[i].ld * (int64_t)es) % 16 == 0);
    // float16 rows, aligned: the form that fits beside the tile kernel, on the side stream -- behind everything the caller's stream holds
    // so far (the rows may still be on their way), and the caller's stream waits for it before the update returns
    hipStream_t run_st = st;
    if (dtype == FAD_F16 && wide) {
        // DETACHED (every handle of the call asked for it: fad_moments_set_reference_mean(h, 2)): the caller vouches that the rows are
        // complete now and stay as they are until the statistics are next read -- the walk starts at once, beside whatever the caller's
        // stream still holds, and settle() orders the readers behind it
        bool detached = true;
        for (int i = 0; i < count; ++i) if (n[i] > 0 && hs[i]->ref_mean && hs[i]->runsum_covers && (!hs[i]->ref_detached || hs[i]->staged_input)) detached = false;
        hipStream_t side = runsum_side_stream(h0->device);
        hipEvent_t pend = (side && detached) ? runsum_ring_event(h0->device) : nullptr;
        if (side && detached && pend) {
            // (it waits for nothing -- except a reader of these very running sums that is still on its way: a chain enqueued on the
            //  caller's stream before the handle was reset would otherwise see the NEXT rows' sums)
            for (int i = 0; i < count; ++i)
                if (n[i] > 0 && hs[i]->rs_reader_set) { FAD_HIP_TRY(hipStreamWaitEvent(side, hs[i]->rs_reader, 0)); hs[i]->rs_reader_set = false; }
            // (... and a walk of the same handle on the caller's stream that may not have left its sums yet: this walk starts from them)
            for (int i = 0; i < count; ++i)
                if (n[i] > 0 && hs[i]->rs_caller_set) { FAD_HIP_TRY(hipStreamWaitEvent(side, hs[i]->rs_caller, 0)); hs[i]->rs_caller_set = false; }
            run_st = side;
        } else if (side) {
            if (!h0->rs_fork) {
                FAD_HIP_TRY(hipEventCreateWithFlags(&h0->rs_fork, hipEventDisableTiming));
                FAD_HIP_TRY(hipEventCreateWithFlags(&h0->rs_join, hipEventDisableTiming));
            }
            FAD_HIP_TRY(hipEventRecord(h0->rs_fork, st));
            FAD_HIP_TRY(hipStreamWaitEvent(side, h0->rs_fork, 0));
            run_st = side;
        }
        launch_runsum_h16(L, m, run_st, idx != nullptr);
        if (run_st != st && pend) {
            FAD_HIP_TRY(hipEventRecord(pend, run_st));
            for (int i = 0; i < count; ++i) if (n[i] > 0 && hs[i]->ref_mean && hs[i]->runsum_covers) hs[i]->rs_pending = pend;
        } else if (run_st != st) {
            FAD_HIP_TRY(hipEventRecord(h0->rs_join, run_st)); *joined = h0->rs_join;
        }
    } else {
        // walks on the caller's stream continue the carry of a detached walk that may still be running on the side stream
        for (int i = 0; i < count; ++i)
            if (n[i] > 0 && hs[i]->rs_pending) FAD_HIP_TRY(hipStreamWaitEvent(st, hs[i]->rs_pending, 0));
    }
    if (dtype == FAD_F16 && wide) {
    } else if (dtype == FAD_F16) {
        hipLaunchKernelGGL((moments_running_colsum<raw_f16, false>), grid, dim3(256), kRunLds, st, L);
    } else if (dtype == FAD_BF16) {
        if (wide) hipLaunchKernelGGL((moments_running_colsum<raw_bf16, true>), grid, dim3(256), kRunLds, st, L);
        else hipLaunchKernelGGL((moments_running_colsum<raw_bf16, false>), grid, dim3(256), kRunLds, st, L);
    } else {
        if (wide) hipLaunchKernelGGL((moments_running_colsum<float, true>), grid, dim3(256), kRunLds, st, L);
        else hipLaunchKernelGGL((moments_running_colsum<float, false>), grid, dim3(256), kRunLds, st, L);
    }
    FAD_HIP_TRY(hipGetLastError());
    if (!(dtype == FAD_F16 && wide)) {
        // a detached walk waits for nothing on the caller's stream -- but it continues THIS walk's carry if the handle's next rows are
        // aligned float16: it waits for the event behind this walk (rs_caller)
        for (int i = 0; i < count; ++i) {
            fad_moments* h = hs[i];
            if (n[i] <= 0 || !h->ref_mean || !h->runsum_covers) continue;
            if (!h->rs_caller) FAD_HIP_TRY(hipEventCreateWithFlags(&h->rs_caller, hipEventDisableTiming));
            FAD_HIP_TRY(hipEventRecord(h->rs_caller, st));
            h->rs_caller_set = true;
        }
    }
    return FAD_OK;
}

static int update_device_multi_impl(int count, fad_moments* const* hs, const void* const* rows, const int64_t* n,
                                    const int64_t* ld, int dtype, hipStream_t st, const SegPlan* seg);
static int update_device_multi(int count, fad_moments* const* hs, const void* const* rows, const int64_t* n,
                               const int64_t* ld, int dtype, hipStream_t st, const SegPlan* seg = nullptr) {
    // numpy's running column sums first (on the side stream where they fit beside the tile kernel), then the update's own kernels;
    // the caller's stream leaves the update only when the walk has read the rows as well
    hipEvent_t joined = nullptr;
    FAD_TRY(running_sums(count, hs, rows, n, ld, dtype, st, &joined));
    const int rc = update_device_multi_impl(count, hs, rows, n, ld, dtype, st, seg);
    if (joined) {
        const hipError_t e = hipStreamWaitEvent(st, joined, 0);
        if (e != hipSuccess && rc == FAD_OK) return set_error(FAD_ERR_HIP, "hipStreamWaitEvent failed: %s", hipGetErrorString(e));
    }
    return rc;
}
static int update_device_multi_impl(int count, fad_moments* const* hs, const void* const* rows, const int64_t* n,
                                    const int64_t* ld, int dtype, hipStream_t st, const SegPlan* seg) {
    fad_moments* h0 = hs[0];
    const int d = h0->d;
    const bool is16 = (dtype == FAD_F16 || dtype == FAD_BF16);
    bool aligned = is16 && (d % 8 == 0);
    for (int i = 0; i < count && aligned; ++i)
        aligned = (ld[i] % 8 == 0) && ((reinterpret_cast<uintptr_t>(rows[i]) & 15u) == 0);
    // Short inputs (every set with fewer than 16 rows per column) take the exact fp64 kernel: it costs next to nothing at that
    // size, and covariances of so few rows are (nearly) rank-deficient -- the Frechet distance then moves with the SQUARE ROOT of
    // a perturbation of the moments, so float32 partial sums (1e-7) could cost parity (1e-4) there.
    int64_t n_max = 0;
    for (int i = 0; i < count; ++i) if (n[i] > n_max) n_max = n[i];
    const bool use_h16 = aligned && !h0->force_generic && (n_max >= 16 * (int64_t)d || seg);

    hipEvent_t* ev = nullptr;
    FAD_TRY(timing_events(h0, &ev));
    h0->last_sets = count;
    if (use_h16 && tile256_eligible(h0, count, n, ld, dtype, aligned, seg != nullptr)) return update_tile256(count, hs, rows, n, ld, st, ev);
    SplitPlan plan[kMaxSets];
    ReduceLaunch R;
    memset(&R, 0, sizeof(R));
    R.d = d;
    if (use_h16) {
        FAD_TRY(ensure_kernel_attrs(h0->device));
        plan_splits(count, n, d, H_BT, H_KB, h0->n_cu, 2, 256, 8192, plan);
        if (seg) { plan[0].S = seg->S; plan[0].rows_per_split = seg->max_split_rows; }
        TileLaunch L;
        memset(&L, 0, sizeof(L));
        L.nsets = count; L.d = d; L.nt = plan[0].nt; L.T = plan[0].T;
        int item = 0, max_s = 0;
        for (int i = 0; i < count; ++i) if (plan[i].S > max_s) max_s = plan[i].S;
        // What a raised guard flag leads to: float16 rows in plain (not file-aligned) splits get a SECOND PASS of the tile kernel
        // over x - c (tile_h16_tr_body, SHIFT) and are un-shifted where their partial tiles are first summed (moments_reduce,
        // or moments_presum of the two-level reduce); everything else is redone by the fp64 kernel.
        // ... Short inputs (fewer than 16 rows per column) keep the fp64 redo, which costs next to nothing there: their
        // covariances are rank-deficient, sqrt(Sigma1 Sigma2) then moves with the SQUARE ROOT of a perturbation, and only sums
        // that are exact to the last bit reproduce the reference's value to 1e-4 (the VGGish pipeline tests: 10 files x 10 frames).
        bool second_pass = dtype == FAD_F16 && !seg;
        for (int i = 0; i < count; ++i) second_pass = second_pass && n[i] >= 16 * (int64_t)d;
        for (int i = 0; i < count; ++i) {
            fad_moments* h = hs[i];
            const SplitPlan& p = plan[i];
            FAD_TRY(h->partials.reserve((size_t)p.S * p.T * H_TS * sizeof(float)));
            FAD_TRY(h->colpart.reserve((size_t)(seg ? seg->n_runs : p.S) * p.nt * H_BT * sizeof(double)));
            TileSet& s = L.set[i];
            s.E = rows[i]; s.n = n[i]; s.ld = ld[i]; s.rows_per_split = p.rows_per_split; s.S = p.S; s.item0 = item;
            if (seg) { s.runs = seg->runs; s.split_first_run = seg->split_first_run; s.seg_runsum = seg->seg_runsum; }
            s.partials = h->partials.p; s.colpart = static_cast<double*>(h->colpart.p);
            s.flag = nullptr;
            if (h->guard && second_pass) {
                FAD_TRY(h->cvec.reserve((size_t)p.S * p.nt * H_BT * sizeof(uint16_t)));
                s.cvec = static_cast<uint16_t*>(h->cvec.p);
            }
            if (h->guard) {
                s.flag = h->shift_flag + (h->update_seq & 1u);
                R.job[i].clear_flag = h->shift_flag + ((h->update_seq + 1u) & 1u);
                h->update_seq++;
            }
            item += p.S * p.T;
        }
        L.total = item;
        if (ev) FAD_HIP_TRY(hipEventRecord(ev[0], st));
        hipLaunchKernelGGL((seg && seg->seg_runsum) ? tr_kernel_walk(dtype, L.T > 1) : tr_kernel(dtype, L.T > 1), dim3((unsigned)L.total), dim3(256), kTrLds, st, L);
        if (ev) FAD_HIP_TRY(hipEventRecord(ev[1], st));

        // shift guard: exact fp64 redo of every flagged set, one gated launch for all of them
        bool any_guard = false;
        TileLaunch G;
        memset(&G, 0, sizeof(G));
        G.nsets = count; G.d = d;
        SplitPlan q[kMaxSets];
        int max_items64 = 0;
        for (int i = 0; i < count; ++i) any_guard = any_guard || (L.set[i].flag != nullptr);
        if (any_guard && second_pass) {
            // same launch geometry, gated per set by its flag; it overwrites the flagged sets' partial tiles and column partials
            hipLaunchKernelGGL(tr_kernel_shift(L.T > 1), dim3((unsigned)L.total), dim3(256), kTrLds, st, L);
            for (int i = 0; i < count; ++i) R.job[i].gate = L.set[i].flag;
        } else if (any_guard) {
            plan_splits(count, n, d, G_BT, G_KB, h0->n_cu, 2, 128, 0, q);
            G.nt = q[0].nt; G.T = q[0].T;
            for (int i = 0; i < count; ++i) {
                fad_moments* h = hs[i];
                FAD_TRY(h->partials64.reserve((size_t)q[i].S * q[i].T * G_TS * sizeof(double)));
                FAD_TRY(h->colpart64.reserve((size_t)q[i].S * q[i].nt * G_BT * sizeof(double)));
                TileSet& s = G.set[i];
                s = L.set[i];
                s.rows_per_split = q[i].rows_per_split; s.S = L.set[i].flag ? q[i].S : 0; s.item0 = 0;
                s.partials = h->partials64.p; s.colpart = static_cast<double*>(h->colpart64.p);
                if (s.S * G.T > max_items64) max_items64 = s.S * G.T;
                R.job[i].alt = reduce_src(h->partials64.p, s.colpart, q[i], G_BT, 0);
                R.job[i].gate = L.set[i].flag;
            }
            FAD_TRY(launch_generic_dtype(G, max_items64, dtype, st));
        }
        // reduce: two-level when any set made more than 128 splits (S -> ceil(S/32) fp64 partials -> accumulator)
        const bool two_level = max_s > 128;
        int max_blocks = 0;
        const int col_blocks = (int)cdiv(d, 256);
        for (int i = 0; i < count; ++i) {
            fad_moments* h = hs[i];
            const SplitPlan& p = plan[i];
            ReduceJob& j = R.job[i];
            float* part = static_cast<float*>(h->partials.p);
            double* colp = static_cast<double*>(h->colpart.p);
            if (two_level) {
                SplitPlan p2 = p;
                p2.S = (int)cdiv(p.S, PRESUM_CHUNK);
                FAD_TRY(h->presum.reserve((size_t)p2.S * p.T * (H_BT * H_BT + 32) * sizeof(double)));
                FAD_TRY(h->presum_col.reserve((size_t)p2.S * p.nt * H_BT * sizeof(double)));
                double* ps = static_cast<double*>(h->presum.p);
                double* pc = static_cast<double*>(h->presum_col.p);
                const int gb = (int)cdiv((int64_t)p.T * (H_BT * H_BT / 4), 256);
                hipLaunchKernelGGL((moments_presum<H_BT>), dim3((unsigned)(gb + cdiv(p.nt * H_BT, 256)), (unsigned)p2.S), dim3(256),
                                   0, st, part, colp, p.S, seg ? seg->n_runs : p.S, p.T, p.nt, gb, ps, pc, (const int*)L.set[i].flag,
                                   (const uint16_t*)L.set[i].cvec, (int64_t)p.rows_per_split, (int64_t)n[i]);
                j.prim = reduce_src(ps, pc, p2, H_BT, 1);
                if (second_pass && L.set[i].cvec) j.gate = nullptr;      // un-shifted already: the second stage always takes these sums
            } else {
                j.prim = reduce_src(part, colp, p, H_BT, 1);
                if (seg) j.prim.SC = seg->n_runs;
                if (second_pass && L.set[i].cvec) { j.prim.cvec = L.set[i].cvec; j.prim.rows_per_split = p.rows_per_split; j.prim.n_rows = n[i]; }
            }
            if (!j.gate) j.alt = j.prim;
            j.acc = h->acc; j.n_add = (double)n[i]; j.overwrite = h->fresh ? 1 : 0;
            int blocks = j.prim.tile_blocks + col_blocks;
            if (j.gate && j.alt.tile_blocks + col_blocks > blocks) blocks = j.alt.tile_blocks + col_blocks;
            if (blocks > max_blocks) max_blocks = blocks;
            h->last_variant = 0;
        }
        if (two_level) hipLaunchKernelGGL((moments_reduce<double, H_BT>), dim3((unsigned)max_blocks, (unsigned)count), dim3(256), 0, st, R);
        else hipLaunchKernelGGL((moments_reduce<float, H_BT>), dim3((unsigned)max_blocks, (unsigned)count), dim3(256), 0, st, R);
        if (ev && h0->timing == 1) FAD_HIP_TRY(hipEventRecord(ev[2], st));
    } else {
        plan_splits(count, n, d, G_BT, G_KB, h0->n_cu, 2, 128, 0, plan);
        TileLaunch L;
        memset(&L, 0, sizeof(L));
        L.nsets = count; L.d = d; L.nt = plan[0].nt; L.T = plan[0].T;
        int max_items = 0, max_blocks = 0;
        const int col_blocks = (int)cdiv(d, 256);
        for (int i = 0; i < count; ++i) {
            fad_moments* h = hs[i];
            const SplitPlan& p = plan[i];
            FAD_TRY(h->partials.reserve((size_t)p.S * p.T * G_TS * sizeof(double)));
            FAD_TRY(h->colpart.reserve((size_t)p.S * p.nt * G_BT * sizeof(double)));
            TileSet& s = L.set[i];
            s.E = rows[i]; s.n = n[i]; s.ld = ld[i]; s.rows_per_split = p.rows_per_split; s.S = p.S; s.item0 = 0;
            s.partials = h->partials.p; s.colpart = static_cast<double*>(h->colpart.p); s.flag = nullptr;
            if (p.S * p.T > max_items) max_items = p.S * p.T;
            ReduceJob& j = R.job[i];
            j.prim = reduce_src(s.partials, s.colpart, p, G_BT, 0);
            j.alt = j.prim;
            j.acc = h->acc; j.n_add = (double)n[i]; j.overwrite = h->fresh ? 1 : 0;
            if (j.prim.tile_blocks + col_blocks > max_blocks) max_blocks = j.prim.tile_blocks + col_blocks;
            h->last_variant = 1;
        }
        L.total = max_items;
        if (ev) FAD_HIP_TRY(hipEventRecord(ev[0], st));
        FAD_TRY(launch_generic_dtype(L, max_items, dtype, st));
        if (ev) FAD_HIP_TRY(hipEventRecord(ev[1], st));
        hipLaunchKernelGGL((moments_reduce<double, G_BT>), dim3((unsigned)max_blocks, (unsigned)count), dim3(256), 0, st, R);
        if (ev && h0->timing == 1) FAD_HIP_TRY(hipEventRecord(ev[2], st));
    }
    FAD_HIP_TRY(hipGetLastError());
    // the deferred reset is consumed only now that the reduce which stores (instead of adds) is on the stream: an error return
    // above leaves every handle "fresh", so a retry still overwrites whatever the accumulator holds
    for (int i = 0; i < count; ++i) hs[i]->fresh = false;
    return FAD_OK;
}

static int update_device(fad_moments* h, const void* rows, int64_t n, int64_t ld, int dtype, hipStream_t st) {
    return update_device_multi(1, &h, &rows, &n, &ld, dtype, st);
}

// Host rows -> HBM staging area of the handle in blocks of at most 1 GiB (hipMemcpy2DAsync from the pageable rows), then
// update_device on each block.  Nothing is synchronised: the copy of block k + 1 waits ON THE DEVICE for the kernels that
// still read block k out of the same staging area.
static int update_any(fad_moments* h, const void* rows, int64_t n, int64_t ld, int dtype, int on_device,
                      hipStream_t st) {
    if (on_device) return update_device(h, rows, n, ld, dtype, st);
    // Host rows reach the kernels through the handle's staging area, block after block: a DETACHED walk of numpy's running sums
    // (fad_moments_set_reference_mean(h, 2): "the rows are complete at the call and stay unchanged") would read that area before the
    // copy has landed and while the next block overwrites it.  The caller's promise holds for ITS rows, not for the staging area:
    // staged updates take the attached walk, which starts behind the copy and is waited for before the area is reused.
    struct StagedScope { fad_moments* h; explicit StagedScope(fad_moments* p) : h(p) { h->staged_input = true; } ~StagedScope() { h->staged_input = false; } } staged_scope(h);
    const size_t es = dtype_size(dtype);
    const int64_t row_bytes = (int64_t)h->d * es;
    int64_t chunk_rows = ((int64_t)1 << 30) / (row_bytes > 0 ? row_bytes : 1);
    if (chunk_rows < 1024) chunk_rows = 1024;
    chunk_rows = (chunk_rows / 32) * 32;
    FAD_TRY(h->stage.reserve((size_t)(n < chunk_rows ? n : chunk_rows) * row_bytes + 16));
    for (int64_t r0 = 0; r0 < n; r0 += chunk_rows) {
        const int64_t m = (n - r0 < chunk_rows) ? n - r0 : chunk_rows;
        const char* src = static_cast<const char*>(rows) + r0 * ld * es;
        // Pieces of ~24 MB, each copied and then accumulated; the copies on a stream of the handle's own, so that the copy of piece p + 1
        // (the host is inside the runtime's staged copy for its whole duration) runs while the device takes the moments -- and, for a
        // handle that carries numpy's running sums, the walk -- of piece p: only the last piece's kernels are left when the last byte has
        // crossed PCIe.  (One copy + one update: 2.04 ms of copy, then 0.07 + 0.37 ms of kernels for [100 000 x 512] float16.)
        // Measured (r05l): one piece 2.40 ms per update, 12 MB pieces 2.36, 24 MB pieces 2.24 (the copy alone: 2.04).
        constexpr int64_t kPieceBytes = (int64_t)24576 * 1024;
        int64_t piece_rows = kPieceBytes / (row_bytes > 0 ? row_bytes : 1);
        piece_rows = (piece_rows / 256) * 256;
        if (piece_rows < 16 * (int64_t)h->d) piece_rows = 16 * (int64_t)h->d;     // (a piece keeps the kernels a whole update of its rows would get: >= 16 rows per column)
        if (piece_rows < 4096 || m < 2 * piece_rows) piece_rows = m;
        if (piece_rows == m) {
            FAD_HIP_TRY(hipMemcpy2DAsync(h->stage.p, (size_t)row_bytes, src, (size_t)(ld * es), (size_t)row_bytes, (size_t)m, hipMemcpyHostToDevice, st));
            FAD_TRY(update_device(h, h->stage.p, m, h->d, dtype, st));
        } else {
            if (!h->cp_st) {
                FAD_HIP_TRY(hipStreamCreateWithFlags(&h->cp_st, hipStreamNonBlocking));
                FAD_HIP_TRY(hipEventCreateWithFlags(&h->cp_enter, hipEventDisableTiming));
                for (auto& e : h->cp_ev) FAD_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            }
            // (kernels of an earlier update may still read the staging area)
            FAD_HIP_TRY(hipEventRecord(h->cp_enter, st));
            FAD_HIP_TRY(hipStreamWaitEvent(h->cp_st, h->cp_enter, 0));
            int piece = 0;
            for (int64_t q0 = 0; q0 < m; ++piece) {
                int64_t pm = (m - q0 < piece_rows) ? m - q0 : piece_rows;
                if (m - q0 - pm < piece_rows / 2) pm = m - q0;                    // (no runt at the end)
                char* dst = static_cast<char*>(h->stage.p) + q0 * row_bytes;
                FAD_HIP_TRY(hipMemcpy2DAsync(dst, (size_t)row_bytes, src + q0 * ld * es, (size_t)(ld * es), (size_t)row_bytes, (size_t)pm, hipMemcpyHostToDevice, h->cp_st));
                FAD_HIP_TRY(hipEventRecord(h->cp_ev[piece & 7], h->cp_st));
                FAD_HIP_TRY(hipStreamWaitEvent(st, h->cp_ev[piece & 7], 0));
                FAD_TRY(update_device(h, dst, pm, h->d, dtype, st));
                q0 += pm;
            }
        }
        // inputs above 1 GiB reuse the staging area: the runtime's pageable route makes no promise to order its staging copies
        // behind the kernels that still read the previous block
        if (r0 + m < n) FAD_HIP_TRY(hipStreamSynchronize(st));
    }
    return FAD_OK;
}

// Per-segment column sums of DEVICE rows into a DEVICE buffer [n_segments x d] (offsets: host).
static int segment_sums_device(fad_moments* h, const void* rows, int64_t ld, int dtype, const int64_t* offsets,
                               int64_t n_segments, double* dout, hipStream_t st) {
    const int d = h->d;
    int64_t n_pieces = 0;
    for (int64_t s = 0; s < n_segments; ++s) n_pieces += cdiv(offsets[s + 1] - offsets[s], SEG_PIECE);
    // host table (pinned staging): [n_segments + 1] first piece of each segment, then the pieces
    const size_t tab_bytes = (size_t)(n_segments + 1) * sizeof(int64_t) + (size_t)n_pieces * sizeof(SegPiece);
    char* tab = nullptr;
    FAD_TRY(stage_tables(h, tab_bytes, &tab));
    int64_t* first = reinterpret_cast<int64_t*>(tab);
    SegPiece* pieces = reinterpret_cast<SegPiece*>(first + n_segments + 1);
    int64_t np = 0;
    for (int64_t s = 0; s < n_segments; ++s) {
        first[s] = np;
        for (int64_t r = offsets[s]; r < offsets[s + 1]; r += SEG_PIECE) {
            const int64_t m = offsets[s + 1] - r;
            pieces[np].r0 = r; pieces[np].rows = (int)(m < SEG_PIECE ? m : SEG_PIECE); pieces[np].seg = (int)s;
            ++np;
        }
    }
    first[n_segments] = np;
    FAD_TRY(h->seg_tab.reserve(tab_bytes));
    h->seg_cached_n = -1;                          // (the fused path's tables, if any, are overwritten)
    FAD_HIP_TRY(hipMemcpyAsync(h->seg_tab.p, tab, tab_bytes, hipMemcpyHostToDevice, st));
    FAD_HIP_TRY(hipEventRecord(h->tab_ev, st));
    const int64_t* dfirst = static_cast<const int64_t*>(h->seg_tab.p);
    const SegPiece* dpieces = reinterpret_cast<const SegPiece*>(dfirst + n_segments + 1);
    if (n_pieces > 0) {
        FAD_TRY(h->seg_piece.reserve((size_t)n_pieces * d * sizeof(double)));
        double* ps = static_cast<double*>(h->seg_piece.p);
        const dim3 grid((unsigned)n_pieces);
        switch (dtype) {
            case FAD_F16: hipLaunchKernelGGL((segment_piece_sums<raw_f16>), grid, dim3(256), 0, st, static_cast<const raw_f16*>(rows), ld, d, dpieces, ps); break;
            case FAD_BF16: hipLaunchKernelGGL((segment_piece_sums<raw_bf16>), grid, dim3(256), 0, st, static_cast<const raw_bf16*>(rows), ld, d, dpieces, ps); break;
            case FAD_F32: hipLaunchKernelGGL((segment_piece_sums<float>), grid, dim3(256), 0, st, static_cast<const float*>(rows), ld, d, dpieces, ps); break;
            default: hipLaunchKernelGGL((segment_piece_sums<double>), grid, dim3(256), 0, st, static_cast<const double*>(rows), ld, d, dpieces, ps); break;
        }
    }
    hipLaunchKernelGGL(segment_gather_sums, dim3((unsigned)n_segments, (unsigned)cdiv(d, 128)), dim3(128), 0, st,
                       static_cast<const double*>(h->seg_piece.p), (int64_t)d, dfirst, d, dout);
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

// numpy's float32 running column sums of every segment (device rows, device offsets) -> dout [n_segments x d] float32 (device)
hipStream_t moments_side_stream(int device) { return runsum_side_stream(device); }
int segment_running_sums_launch(const void* drows, int64_t dld, int d, int dtype, const int64_t* doff, int64_t n_segments, float* dout,
                                hipStream_t st, DevBuf* jobs, int64_t mean_rows, int device) {
    const size_t es = dtype_size(dtype);
    // float16 rows on 16-byte aligned pitches, segments of some length: the LDS-staged walk of the plain update, one workgroup per
    // (segment, 32 columns) -- the rows of a segment stream through coalesced, the adds cost ~9 cycles a row; one thread per 8 columns of
    // a segment is latency-bound per THREAD (2.4 us per 16 rows in flight: 0.23 ms for 32 songs of [1500 x 768], r05d)
    // (d >= 256: with fewer columns a row is one or two cache lines, the 16-column workgroups of a segment land on different XCDs and every
    //  line crosses the fabric once per workgroup -- config 4's files, d = 128: 1.4 ms per group of 4096 against 0.4 with a thread per 8 columns)
    if (jobs && dtype == FAD_F16 && d % 8 == 0 && d >= 256 && (dld * 2) % 16 == 0 && (reinterpret_cast<uintptr_t>(drows) & 15u) == 0 &&
        mean_rows >= 256 && n_segments <= 65535) {
        FAD_TRY(ensure_kernel_attrs(device));
        FAD_TRY(jobs->reserve((size_t)n_segments * sizeof(RunSumJob)));
        RunSumJob* table = static_cast<RunSumJob*>(jobs->p);
        hipLaunchKernelGGL(runsum_segment_jobs, dim3((unsigned)cdiv(n_segments, 256)), dim3(256), 0, st, static_cast<const uint16_t*>(drows), dld, d,
                           doff, n_segments, dout, table);
        RunSumLaunch L;
        memset(&L, 0, sizeof(L));
        L.d = d; L.table = table;
        launch_runsum_h16(L, (int)n_segments, st);
        FAD_HIP_TRY(hipGetLastError());
        return FAD_OK;
    }
    const bool wide = (dtype == FAD_F16 || dtype == FAD_BF16) && d % 8 == 0 && (dld * (int64_t)es) % 16 == 0 && (reinterpret_cast<uintptr_t>(drows) & 15u) == 0;
    const int64_t items = n_segments * (wide ? d / 8 : d);
    const dim3 grid((unsigned)cdiv(items, 256));
    switch (dtype) {
        case FAD_F16:
            if (wide) hipLaunchKernelGGL((segment_running_sums<raw_f16, true>), grid, dim3(256), 0, st, static_cast<const raw_f16*>(drows), dld, d, doff, n_segments, dout);
            else hipLaunchKernelGGL((segment_running_sums<raw_f16, false>), grid, dim3(256), 0, st, static_cast<const raw_f16*>(drows), dld, d, doff, n_segments, dout);
            break;
        case FAD_BF16:
            if (wide) hipLaunchKernelGGL((segment_running_sums<raw_bf16, true>), grid, dim3(256), 0, st, static_cast<const raw_bf16*>(drows), dld, d, doff, n_segments, dout);
            else hipLaunchKernelGGL((segment_running_sums<raw_bf16, false>), grid, dim3(256), 0, st, static_cast<const raw_bf16*>(drows), dld, d, doff, n_segments, dout);
            break;
        case FAD_F32:
            hipLaunchKernelGGL((segment_running_sums<float, false>), grid, dim3(256), 0, st, static_cast<const float*>(drows), dld, d, doff, n_segments, dout);
            break;
        default:
            return set_error(FAD_ERR_INVALID, "running sums of float64 frames are the exact sums: pass seg_runsums = NULL");
    }
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

}  // namespace fad

using namespace fad;

extern "C" {

int fad_moments_create(int d, int device, fad_moments_t** out) {
    if (!out) return set_error(FAD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || d > 16384) return set_error(FAD_ERR_INVALID, "d=%d out of range [1, 16384]", d);
    FAD_TRY(check_device(device));
    DeviceGuard g(device);
    if (!g.ok) return set_error(FAD_ERR_HIP, "cannot select device %d", device);
    fad_moments* h = new (std::nothrow) fad_moments();
    if (!h) return set_error(FAD_ERR_ALLOC, "out of host memory");
    h->d = d; h->device = device; h->n_cu = num_cus(device);
    const size_t bytes = (size_t)packed_len(d) * sizeof(double);
    if (hipMalloc(reinterpret_cast<void**>(&h->acc), bytes) != hipSuccess) {
        delete h;
        return set_error(FAD_ERR_ALLOC, "hipMalloc of %zu bytes failed", bytes);
    }
    if (hipMemset(h->acc, 0, bytes) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&h->shift_flag), 2 * sizeof(int)) != hipSuccess ||
        hipMemset(h->shift_flag, 0, 2 * sizeof(int)) != hipSuccess) {
        (void)hipFree(h->acc); delete h;
        return set_error(FAD_ERR_HIP, "hipMemset / hipMalloc failed");
    }
    // the knobs are read once, here: nothing on the update path calls getenv
    const char* gs = getenv("FAD_MOMENTS_SHIFT_GUARD");
    h->guard = !(gs && gs[0] == '0');
    const char* fg = getenv("FAD_MOMENTS_FORCE_GENERIC");
    h->force_generic = fg && fg[0] == '1';
    const char* t2 = getenv("FAD_MOMENTS_TILE256");
    h->tile256 = !(t2 && t2[0] == '0');
    const char* nc = getenv("FAD_MOMENTS_CUS");        // plan for fewer CUs than the device has (a CU-masked stream)
    if (nc && atoi(nc) >= 8 && atoi(nc) < h->n_cu) h->n_cu = atoi(nc);
    *out = h;
    return FAD_OK;
}

int fad_moments_destroy(fad_moments_t* h) {
    if (!h) return FAD_OK;
    DeviceGuard g(h->device);
    if (h->acc && h->owns_acc) (void)hipFree(h->acc);
    if (h->shift_flag) (void)hipFree(h->shift_flag);
    h->partials64.release(); h->colpart64.release(); h->cvec.release(); h->presum.release(); h->presum_col.release(); h->blocktab.release();
    h->partials.release(); h->colpart.release(); h->stage.release();
    h->seg_tab.release(); h->seg_piece.release(); h->seg_out.release(); h->scratch.release(); h->runsum.release();
    h->seg_run.release(); h->seg_off.release(); h->seg_jobs.release();
    if (h->tab_host) (void)hipHostFree(h->tab_host);
    if (h->tab_ev) (void)hipEventDestroy(h->tab_ev);
    if (h->rs_fork) (void)hipEventDestroy(h->rs_fork);
    if (h->cp_enter) (void)hipEventDestroy(h->cp_enter);
    for (auto& e : h->cp_ev) if (e) (void)hipEventDestroy(e);
    if (h->cp_st) (void)hipStreamDestroy(h->cp_st);
    if (h->rs_join) (void)hipEventDestroy(h->rs_join);
    if (h->ev) { for (int i = 0; i < fad_moments::kRing * 3; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]); delete[] h->ev; }
    if (h->rs_reader) (void)hipEventDestroy(h->rs_reader);
    if (h->rs_caller) (void)hipEventDestroy(h->rs_caller);
    delete h;
    return FAD_OK;
}

// The accumulator's memset is deferred: an update right after a reset overwrites it (saves a launch per set);
// every other reader settles the pending zeroing first.
static int settle(const fad_moments* hc, hipStream_t st) {
    fad_moments* h = const_cast<fad_moments*>(hc);
    // a detached walk of numpy's running sums: whoever reads the statistics waits for it -- EVERY reader, on whatever stream (the
    // event stays with the handle until the next walk replaces it; waiting twice costs nothing)
    if (h->rs_pending) FAD_HIP_TRY(hipStreamWaitEvent(st, h->rs_pending, 0));
    if (!h->fresh) return FAD_OK;
    FAD_HIP_TRY(hipMemsetAsync(h->acc, 0, (size_t)packed_len(h->d) * sizeof(double), st));
    h->fresh = false;
    return FAD_OK;
}

int fad_moments_reset(fad_moments_t* h, void* stream) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    (void)stream;
    h->fresh = true;
    h->runsum_live = false; h->runsum_covers = true;
    return FAD_OK;
}

int fad_moments_reset_multi(int count, fad_moments_t* const* hs, void* stream) {
    if (count < 0 || (count > 0 && !hs)) return set_error(FAD_ERR_INVALID, "bad handle list");
    for (int i = 0; i < count; ++i) FAD_TRY(fad_moments_reset(hs[i], stream));
    return FAD_OK;
}

int fad_moments_settle(fad_moments_t* h, void* stream) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    DeviceGuard g(h->device);
    return settle(h, static_cast<hipStream_t>(stream));
}

int fad_moments_bind(fad_moments_t* h, double* device_packed) {
    if (!h || !device_packed) return set_error(FAD_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(device_packed) & 15u) return set_error(FAD_ERR_INVALID, "buffer must be 16-byte aligned");
    DeviceGuard g(h->device);
    if (h->acc && h->owns_acc) FAD_HIP_TRY(hipFree(h->acc));
    h->acc = device_packed;
    h->owns_acc = false;
    h->fresh = true;                               // bind = adopt the buffer and reset
    h->runsum_live = false; h->runsum_covers = true;
    return FAD_OK;
}

int fad_moments_dim(const fad_moments_t* h) { return h ? h->d : set_error(FAD_ERR_INVALID, "handle is NULL"); }
int64_t fad_moments_packed_len(const fad_moments_t* h) {
    return h ? packed_len(h->d) : (int64_t)set_error(FAD_ERR_INVALID, "handle is NULL");
}

int fad_moments_update(fad_moments_t* h, const void* rows, int64_t n, int64_t ld, int dtype,
                       int on_device, void* stream) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    if (n < 0 || ld < h->d) return set_error(FAD_ERR_SHAPE, "n=%lld ld=%lld d=%d", (long long)n, (long long)ld, h->d);
    if (dtype_size(dtype) == 0) return set_error(FAD_ERR_INVALID, "unknown dtype %d", dtype);
    if (n == 0) return FAD_OK;
    if (!rows) return set_error(FAD_ERR_INVALID, "rows is NULL");
    DeviceGuard g(h->device);
    return update_any(h, rows, n, ld, dtype, on_device, static_cast<hipStream_t>(stream));
}

int fad_moments_update_multi(int count, fad_moments_t* const* hs, const void* const* rows, const int64_t* n,
                             const int64_t* ld, int dtype, void* stream) {
    if (count < 1 || count > kMaxSets256) return set_error(FAD_ERR_INVALID, "count=%d out of range [1, %d]", count, kMaxSets256);
    if (!hs || !rows || !n || !ld) return set_error(FAD_ERR_INVALID, "NULL argument");
    if (dtype_size(dtype) == 0) return set_error(FAD_ERR_INVALID, "unknown dtype %d", dtype);
    fad_moments* live_h[kMaxSets256]; const void* live_rows[kMaxSets256]; int64_t live_n[kMaxSets256], live_ld[kMaxSets256];
    int m = 0;
    for (int i = 0; i < count; ++i) {
        if (!hs[i]) return set_error(FAD_ERR_INVALID, "handle %d is NULL", i);
        if (hs[i]->d != hs[0]->d || hs[i]->device != hs[0]->device)
            return set_error(FAD_ERR_SHAPE, "handle %d: d=%d device=%d, handle 0: d=%d device=%d", i, hs[i]->d, hs[i]->device,
                             hs[0]->d, hs[0]->device);
        for (int k = 0; k < i; ++k)
            if (hs[k] == hs[i]) return set_error(FAD_ERR_INVALID, "handle %d appears twice", i);
        if (n[i] < 0 || ld[i] < hs[i]->d)
            return set_error(FAD_ERR_SHAPE, "set %d: n=%lld ld=%lld d=%d", i, (long long)n[i], (long long)ld[i], hs[i]->d);
        if (n[i] == 0) continue;
        if (!rows[i]) return set_error(FAD_ERR_INVALID, "rows[%d] is NULL", i);
        live_h[m] = hs[i]; live_rows[m] = rows[i]; live_n[m] = n[i]; live_ld[m] = ld[i]; ++m;
    }
    if (m == 0) return FAD_OK;
    DeviceGuard g(live_h[0]->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m > kMaxSets) {
        // More than sixteen matrices share ONE launch of each kernel only on the 256-column-slab route (whose launch tables are that
        // long) and only when no handle wants numpy's running sums beside it (the walk's tables are not); everything else goes
        // sixteen at a time -- the same kernels, the same results, one more launch of each.
        bool one = dtype == FAD_F16 && live_h[0]->d % 8 == 0;
        for (int i = 0; i < m && one; ++i)
            one = !live_h[i]->ref_mean && (live_ld[i] % 8 == 0) && ((reinterpret_cast<uintptr_t>(live_rows[i]) & 15u) == 0);
        one = one && tile256_eligible(live_h[0], m, live_n, live_ld, dtype, true, false);
        if (!one) {
            for (int i0 = 0; i0 < m; i0 += kMaxSets) {
                const int c = (m - i0 < kMaxSets) ? m - i0 : kMaxSets;
                FAD_TRY(update_device_multi(c, live_h + i0, live_rows + i0, live_n + i0, live_ld + i0, dtype, st));
            }
            return FAD_OK;
        }
    }
    return update_device_multi(m, live_h, live_rows, live_n, live_ld, dtype, st);
}

// rows[idx[r]] -> a dense matrix: the fallback of fad_moments_update_multi_indexed (16-byte chunks when everything is aligned, else bytes)
__global__ void gather_rows_kernel(const char* __restrict__ src, int64_t src_pitch, const int32_t* __restrict__ idx, int64_t n, char* __restrict__ dst,
                                   int row_bytes, int wide) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wide) {
        const int per = row_bytes / 16;
        if (t >= n * per) return;
        const int64_t r = t / per; const int c = (int)(t - r * per);
        reinterpret_cast<uint4*>(dst + r * row_bytes)[c] = reinterpret_cast<const uint4*>(src + (int64_t)idx[r] * src_pitch)[c];
    } else {
        if (t >= n * row_bytes) return;
        const int64_t r = t / row_bytes; const int c = (int)(t - r * row_bytes);
        dst[r * row_bytes + c] = src[(int64_t)idx[r] * src_pitch + c];
    }
}

int fad_moments_update_multi_indexed(int count, fad_moments_t* const* hs, const void* rows, int64_t n_src, int64_t ld, int dtype,
                                     const int32_t* const* idx, const int64_t* n_idx, void* stream) {
    if (count < 1 || count > kMaxSets) return set_error(FAD_ERR_INVALID, "count=%d out of range [1, %d]", count, kMaxSets);
    if (!hs || !rows || !idx || !n_idx) return set_error(FAD_ERR_INVALID, "NULL argument");
    const size_t es = dtype_size(dtype);
    if (es == 0) return set_error(FAD_ERR_INVALID, "unknown dtype %d", dtype);
    if (n_src < 1 || n_src > INT32_MAX) return set_error(FAD_ERR_SHAPE, "n_src=%lld", (long long)n_src);
    fad_moments* live_h[kMaxSets]; const int32_t* live_idx[kMaxSets]; int64_t live_n[kMaxSets], live_ld[kMaxSets]; const void* live_rows[kMaxSets];
    int m = 0;
    for (int i = 0; i < count; ++i) {
        if (!hs[i]) return set_error(FAD_ERR_INVALID, "handle %d is NULL", i);
        if (hs[i]->d != hs[0]->d || hs[i]->device != hs[0]->device) return set_error(FAD_ERR_SHAPE, "handle %d: another dimension or device than handle 0", i);
        for (int k = 0; k < i; ++k)
            if (hs[k] == hs[i]) return set_error(FAD_ERR_INVALID, "handle %d appears twice", i);
        if (n_idx[i] < 0 || ld < hs[i]->d) return set_error(FAD_ERR_SHAPE, "set %d: n=%lld ld=%lld d=%d", i, (long long)n_idx[i], (long long)ld, hs[i]->d);
        if (n_idx[i] == 0) continue;
        if (!idx[i]) return set_error(FAD_ERR_INVALID, "idx[%d] is NULL", i);
        live_h[m] = hs[i]; live_idx[m] = idx[i]; live_n[m] = n_idx[i]; live_ld[m] = ld; live_rows[m] = rows; ++m;
    }
    if (m == 0) return FAD_OK;
    fad_moments* h0 = live_h[0];
    DeviceGuard g(h0->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int d = h0->d;
    const bool aligned = dtype == FAD_F16 && d % 8 == 0 && ld % 8 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15u) == 0;
    // the gather rides on the slab kernel's row offsets (32-bit, range-checked against the WHOLE source: below 2^31 bytes) and on the
    // walk's loads; everything else gathers into the handles' staging areas first and takes the ordinary route
    if (aligned && !h0->force_generic && tile256_eligible(h0, m, live_n, live_ld, dtype, true, false) && n_src * ld * 2 < ((int64_t)1 << 31)) {
        hipEvent_t joined = nullptr;
        FAD_TRY(running_sums(m, live_h, live_rows, live_n, live_ld, dtype, st, &joined, live_idx));
        hipEvent_t* ev = nullptr;
        FAD_TRY(timing_events(h0, &ev));
        h0->last_sets = m;
        const int rc = update_tile256(m, live_h, live_rows, live_n, live_ld, st, ev, live_idx, n_src);
        if (joined) {
            const hipError_t e = hipStreamWaitEvent(st, joined, 0);
            if (e != hipSuccess && rc == FAD_OK) return set_error(FAD_ERR_HIP, "hipStreamWaitEvent failed: %s", hipGetErrorString(e));
        }
        return rc;
    }
    const int row_bytes = (int)((size_t)d * es);
    const int wide = (row_bytes % 16 == 0) && ((ld * (int64_t)es) % 16 == 0) && ((reinterpret_cast<uintptr_t>(rows) & 15u) == 0);
    for (int i = 0; i < m; ++i) {
        fad_moments* h = live_h[i];
        FAD_TRY(h->stage.reserve((size_t)live_n[i] * row_bytes + 16));
        const int64_t items = wide ? live_n[i] * (row_bytes / 16) : live_n[i] * row_bytes;
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv(items, 256)), dim3(256), 0, st, static_cast<const char*>(rows), ld * (int64_t)es,
                           live_idx[i], live_n[i], static_cast<char*>(h->stage.p), row_bytes, wide);
        live_rows[i] = h->stage.p; live_ld[i] = d;
    }
    FAD_HIP_TRY(hipGetLastError());
    for (int i = 0; i < m; ++i) live_h[i]->staged_input = true;     // (the gathered copies are on their way: no detached walk over them)
    const int rc = update_device_multi(m, live_h, live_rows, live_n, live_ld, dtype, st);
    for (int i = 0; i < m; ++i) live_h[i]->staged_input = false;
    return rc;
}

static int segment_running_sums_device(fad_moments* h, const void* drows, int64_t dld, int dtype, const int64_t* offsets, int64_t n_segments,
                                       float* dout, hipStream_t st) {
    FAD_TRY(h->seg_off.reserve((size_t)(n_segments + 1) * sizeof(int64_t)));
    // through the handle's pinned table area like every other table of this file (stage_tables waits for the previous upload's event;
    // a pageable source would lean on the runtime staging it before the call returns -- the caller frees `offsets` right after)
    char* pinned = nullptr;
    const size_t off_bytes = (size_t)(n_segments + 1) * sizeof(int64_t);
    FAD_TRY(stage_tables(h, off_bytes, &pinned));
    memcpy(pinned, offsets, off_bytes);
    FAD_HIP_TRY(hipMemcpyAsync(h->seg_off.p, pinned, off_bytes, hipMemcpyHostToDevice, st));
    FAD_HIP_TRY(hipEventRecord(h->tab_ev, st));
    const int64_t total = n_segments > 0 ? offsets[n_segments] - offsets[0] : 0;
    return segment_running_sums_launch(drows, dld, h->d, dtype, static_cast<const int64_t*>(h->seg_off.p), n_segments, dout, st, &h->seg_jobs,
                                       n_segments > 0 ? total / n_segments : 0, h->device);
}

static int update_segmented_impl(fad_moments_t* h, const void* rows, int64_t n, int64_t ld, int dtype,
                                 const int64_t* offsets, int64_t n_segments, double* seg_sums, float* seg_runsums,
                                 int on_device, void* stream) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    if (n < 0 || ld < h->d) return set_error(FAD_ERR_SHAPE, "n=%lld ld=%lld d=%d", (long long)n, (long long)ld, h->d);
    if (dtype_size(dtype) == 0) return set_error(FAD_ERR_INVALID, "unknown dtype %d", dtype);
    if (n_segments < 0 || (n_segments > 0 && !offsets)) return set_error(FAD_ERR_INVALID, "bad segment list");
    for (int64_t s = 0; s < n_segments; ++s)
        if (offsets[s] > offsets[s + 1] || offsets[s] < 0 || offsets[s + 1] > n)
            return set_error(FAD_ERR_INVALID, "offsets must be non-decreasing within [0, n]");
    if (n == 0) return FAD_OK;
    if (!rows) return set_error(FAD_ERR_INVALID, "rows is NULL");
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t es = dtype_size(dtype);
    const void* drows = rows;
    int64_t dld = ld;
    struct StagedScope { fad_moments* h; bool on; StagedScope(fad_moments* p, bool o) : h(p), on(o) { if (on) h->staged_input = true; } ~StagedScope() { if (on) h->staged_input = false; } } staged_scope(h, !on_device);
    if (!on_device) {      // one staged copy serves both kernels (bounded by caller: host blocks are per-batch)
        const int64_t row_bytes = (int64_t)h->d * es;
        FAD_TRY(h->stage.reserve((size_t)n * row_bytes + 16));
        FAD_HIP_TRY(hipMemcpy2DAsync(h->stage.p, (size_t)row_bytes, rows, (size_t)(ld * es), (size_t)row_bytes, (size_t)n, hipMemcpyHostToDevice, st));
        drows = h->stage.p; dld = h->d;
    }
    double* dout = seg_sums;
    const bool want_sums = seg_sums && n_segments > 0;
    if (want_sums && !on_device) {
        FAD_TRY(h->seg_out.reserve((size_t)n_segments * h->d * sizeof(double)));
        dout = static_cast<double*>(h->seg_out.p);
    }
    // Long files of aligned fp16/bf16 frames (config 4: 2250 frames per file): splits aligned to the files, so that the
    // column sums every diagonal-tile workgroup holds anyway ARE the per-file sums -- no second pass over E.  Short
    // segments (a few frames per song) would make one pipeline fill per segment: they keep the two-stage kernel.
    const int d = h->d;
    const bool is16 = (dtype == FAD_F16 || dtype == FAD_BF16);
    const bool aligned = is16 && (d % 8 == 0) && (dld % 8 == 0) && ((reinterpret_cast<uintptr_t>(drows) & 15u) == 0) && !h->force_generic;
    bool fused = false, walked = false;
    if (want_sums && aligned) {
        constexpr int64_t kCap = 8192;             // rows one workgroup may sum in fp32 (see plan_splits)
        int64_t n_runs = 0, covered = 0;
        for (int64_t sg = 0; sg < n_segments; ++sg) { const int64_t len = offsets[sg + 1] - offsets[sg]; n_runs += len > 0 ? cdiv(len, kCap) : 1; covered += len; }
        fused = covered == n && offsets[0] == 0 && n_runs > 0 && covered / n_runs >= 256 && n_runs < (1 << 30);
        const bool same_tables = fused && h->seg_cached_n == n && (int64_t)h->seg_cached_offsets.size() == n_segments + 1 && h->seg_tab.p &&
                                 memcmp(h->seg_cached_offsets.data(), offsets, (size_t)(n_segments + 1) * sizeof(int64_t)) == 0;
        SegPlan sp;
        char* dev = nullptr;
        size_t bytes_runs = 0, bytes_first = 0;
        if (same_tables) {
            // the very segment list of the previous call: its tables are on the device already
            bytes_runs = h->seg_cached_bytes_runs; bytes_first = h->seg_cached_bytes_first;
            dev = static_cast<char*>(h->seg_tab.p);
            sp.runs = reinterpret_cast<const SegRun*>(dev);
            sp.split_first_run = reinterpret_cast<const int*>(dev + bytes_runs + bytes_first);
            sp.n_runs = (int)h->seg_cached_runs; sp.S = h->seg_cached_S; sp.max_split_rows = h->seg_cached_max;
        } else if (fused) {
            // target rows per split: what the uniform planner would choose, but never above the fp32 cap
            SplitPlan up;
            plan_splits(1, &n, d, H_BT, H_KB, h->n_cu, 2, 256, kCap, &up);
            const int64_t target = up.rows_per_split;
            // host tables: runs | seg_first_run (int64) | split_first_run (int32)
            bytes_runs = (size_t)n_runs * sizeof(SegRun); bytes_first = (size_t)(n_segments + 1) * sizeof(int64_t);
            const size_t bytes_split = (size_t)(n_runs + 1) * sizeof(int);
            char* host = nullptr;
            FAD_TRY(stage_tables(h, bytes_runs + bytes_first + bytes_split, &host));
            SegRun* runs = reinterpret_cast<SegRun*>(host);
            int64_t* seg_first = reinterpret_cast<int64_t*>(host + bytes_runs);
            int* split_first = reinterpret_cast<int*>(host + bytes_runs + bytes_first);
            int64_t nr = 0;
            for (int64_t sg = 0; sg < n_segments; ++sg) {
                seg_first[sg] = nr;
                const int64_t len = offsets[sg + 1] - offsets[sg];
                const int64_t parts = len > 0 ? cdiv(len, kCap) : 1;
                const int64_t per = len > 0 ? cdiv(cdiv(len, parts), H_KB) * H_KB : 0;
                for (int64_t q = 0; q < parts; ++q) {
                    const int64_t r0 = offsets[sg] + q * per;
                    int64_t m = offsets[sg + 1] - r0; if (m > per) m = per; if (m < 0) m = 0;
                    runs[nr].r0 = r0; runs[nr].rows = (int32_t)m; runs[nr].seg = (int32_t)sg; ++nr;
                }
            }
            seg_first[n_segments] = nr;
            int S = 0; int64_t acc_rows = 0, max_rows = 0;
            split_first[0] = 0;
            for (int64_t r = 0; r < nr; ++r) {          // greedy: consecutive runs until the target (or the cap) would be passed
                if (acc_rows > 0 && (acc_rows + runs[r].rows > target || acc_rows + runs[r].rows > kCap)) {
                    if (acc_rows > max_rows) max_rows = acc_rows;
                    split_first[++S] = (int)r; acc_rows = 0;
                }
                acc_rows += runs[r].rows;
            }
            if (acc_rows > max_rows) max_rows = acc_rows;
            split_first[++S] = (int)nr;
            FAD_TRY(h->seg_tab.reserve(bytes_runs + bytes_first + bytes_split));
            FAD_HIP_TRY(hipMemcpyAsync(h->seg_tab.p, host, bytes_runs + bytes_first + (size_t)(S + 1) * sizeof(int), hipMemcpyHostToDevice, st));
            FAD_HIP_TRY(hipEventRecord(h->tab_ev, st));
            dev = static_cast<char*>(h->seg_tab.p);
            sp.runs = reinterpret_cast<const SegRun*>(dev);
            sp.split_first_run = reinterpret_cast<const int*>(dev + bytes_runs + bytes_first);
            sp.n_runs = (int)nr; sp.S = S; sp.max_split_rows = max_rows > 0 ? max_rows : H_KB;
            h->seg_cached_offsets.assign(offsets, offsets + n_segments + 1);
            h->seg_cached_n = n; h->seg_cached_S = S; h->seg_cached_runs = nr; h->seg_cached_max = sp.max_split_rows;
            h->seg_cached_bytes_runs = bytes_runs; h->seg_cached_bytes_first = bytes_first;
        }
        if (fused) {
            fad_moments* hh = h;
            // every file one run (<= 8192 frames: config 4's 2250): the tile kernel's diagonal workgroups see a file's rows in order and
            // walk numpy's float32 running sums beside their MFMAs -- the frames cross HBM once (round 5: a second pass, 4.1 instead of 2.3 ms)
            if (seg_runsums && n_segments > 0 && sp.n_runs == n_segments && (dtype == FAD_F16 || dtype == FAD_BF16)) {
                float* drun = seg_runsums;
                if (!on_device) {
                    FAD_TRY(h->seg_run.reserve((size_t)n_segments * h->d * sizeof(float)));
                    drun = static_cast<float*>(h->seg_run.p);
                }
                sp.seg_runsum = drun;
                walked = true;
            }
            FAD_TRY(update_device_multi(1, &hh, &drows, &n, &dld, dtype, st, &sp));
            const int nt = (int)cdiv(d, H_BT);
            hipLaunchKernelGGL(segment_gather_sums, dim3((unsigned)n_segments, (unsigned)cdiv(d, 128)), dim3(128), 0, st,
                               static_cast<const double*>(h->colpart.p), (int64_t)nt * H_BT,
                               reinterpret_cast<const int64_t*>(dev + bytes_runs), d, dout);
            FAD_HIP_TRY(hipGetLastError());
        }
    }
    if (!fused) FAD_TRY(update_device(h, drows, n, dld, dtype, st));
    if (want_sums) {
        if (!fused) FAD_TRY(segment_sums_device(h, drows, dld, dtype, offsets, n_segments, dout, st));
        if (!on_device) {
            FAD_HIP_TRY(hipMemcpyAsync(seg_sums, dout, (size_t)n_segments * h->d * sizeof(double),
                                       hipMemcpyDeviceToHost, st));
        }
    }
    if (seg_runsums && n_segments > 0) {
        // (files of more than one run, short segments, float32 frames:) the second walk over the rows the reference's per-file np.mean
        // asks for (utils.py:16): they have just been read by the tile kernel -- a group of files that fits the Infinity Cache is served from there
        float* drun = seg_runsums;
        if (!on_device) {
            FAD_TRY(h->seg_run.reserve((size_t)n_segments * h->d * sizeof(float)));
            drun = static_cast<float*>(h->seg_run.p);
        }
        if (!walked) FAD_TRY(segment_running_sums_device(h, drows, dld, dtype, offsets, n_segments, drun, st));
        if (!on_device)
            FAD_HIP_TRY(hipMemcpyAsync(seg_runsums, drun, (size_t)n_segments * h->d * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (!on_device) FAD_HIP_TRY(hipStreamSynchronize(st));
    return FAD_OK;
}

int fad_moments_update_segmented(fad_moments_t* h, const void* rows, int64_t n, int64_t ld, int dtype,
                                 const int64_t* offsets, int64_t n_segments, double* seg_sums,
                                 int on_device, void* stream) {
    return update_segmented_impl(h, rows, n, ld, dtype, offsets, n_segments, seg_sums, nullptr, on_device, stream);
}

int fad_moments_update_segmented_ref(fad_moments_t* h, const void* rows, int64_t n, int64_t ld, int dtype,
                                     const int64_t* offsets, int64_t n_segments, double* seg_sums, float* seg_runsums,
                                     int on_device, void* stream) {
    if (seg_runsums && dtype == FAD_F64) return set_error(FAD_ERR_INVALID, "float64 frames: numpy's sum is the exact one, pass seg_runsums = NULL");
    return update_segmented_impl(h, rows, n, ld, dtype, offsets, n_segments, seg_sums, seg_runsums, on_device, stream);
}

static int update_file_means_impl(fad_moments_t* exact, fad_moments_t* rounded, fad_moments_t* weighted,
                                  const double* seg_sums, const float* seg_runsums, const int64_t* sizes, int64_t n_files, int dtype,
                                  int on_device, void* stream) {
    if (!exact || !rounded || !weighted) return set_error(FAD_ERR_INVALID, "handle is NULL");
    if (exact == rounded || exact == weighted || rounded == weighted) return set_error(FAD_ERR_INVALID, "three distinct handles are needed");
    const int d = exact->d;
    if (rounded->d != d || weighted->d != d || rounded->device != exact->device || weighted->device != exact->device)
        return set_error(FAD_ERR_SHAPE, "the three handles must share dimension and device");
    if (dtype_size(dtype) == 0) return set_error(FAD_ERR_INVALID, "unknown dtype %d", dtype);
    if (n_files < 0) return set_error(FAD_ERR_INVALID, "n_files=%lld", (long long)n_files);
    if (n_files == 0) return FAD_OK;
    if (!seg_sums || !sizes) return set_error(FAD_ERR_INVALID, "NULL argument");
    DeviceGuard g(exact->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t cells = (size_t)n_files * d;
    const bool sums_dev = (on_device & 1) != 0, sizes_dev = (on_device & 2) != 0, runs_dev = (on_device & 4) != 0;
    // numpy's per-file running sums (host array: uploaded into a buffer of their own)
    const float* druns = seg_runsums;
    if (seg_runsums && !runs_dev) {
        FAD_TRY(exact->seg_run.reserve(cells * sizeof(float)));
        FAD_HIP_TRY(hipMemcpyAsync(exact->seg_run.p, seg_runsums, cells * sizeof(float), hipMemcpyHostToDevice, st));
        druns = static_cast<const float*>(exact->seg_run.p);
    }
    // scratch of `exact`: [sums | sizes] as far as they arrive from the host, then the three row blocks
    const size_t sums_bytes = sums_dev ? 0 : cells * sizeof(double);
    const size_t sizes_bytes = sizes_dev ? 0 : (size_t)n_files * sizeof(int64_t);
    const size_t in_bytes = sums_bytes + sizes_bytes;
    FAD_TRY(exact->scratch.reserve(in_bytes + 3 * cells * sizeof(double) + 64));
    char* base = static_cast<char*>(exact->scratch.p);
    const double* dsums = seg_sums; const int64_t* dsizes = sizes;
    if (!sums_dev) {
        FAD_HIP_TRY(hipMemcpyAsync(base, seg_sums, sums_bytes, hipMemcpyHostToDevice, st));
        dsums = reinterpret_cast<const double*>(base);
    }
    if (!sizes_dev) {                              // through the handle's pinned staging: no pageable copy on the stream
        // (the same sizes as last time, still at the same place of the scratch area: nothing to upload -- groups of equally long files)
        const bool same = exact->sizes_cached_at == base + sums_bytes && (int64_t)exact->sizes_cached.size() == n_files &&
                          memcmp(exact->sizes_cached.data(), sizes, sizes_bytes) == 0;
        if (!same) {
            char* host = nullptr;
            FAD_TRY(stage_tables(exact, sizes_bytes, &host));
            memcpy(host, sizes, sizes_bytes);
            FAD_HIP_TRY(hipMemcpyAsync(base + sums_bytes, host, sizes_bytes, hipMemcpyHostToDevice, st));
            FAD_HIP_TRY(hipEventRecord(exact->tab_ev, st));
            exact->sizes_cached.assign(sizes, sizes + n_files);
            exact->sizes_cached_at = base + sums_bytes;
        } else if (exact->tab_ev) {
            FAD_HIP_TRY(hipStreamWaitEvent(st, exact->tab_ev, 0));       // (the cached copy may have been uploaded on another stream)
        }
        dsizes = reinterpret_cast<const int64_t*>(base + sums_bytes);
    } else {
        exact->sizes_cached_at = nullptr;          // (device sizes: the row blocks below start where a cached host copy would sit)
    }
    double* r_exact = reinterpret_cast<double*>(base + ((in_bytes + 15) & ~(size_t)15));
    double* r_round = r_exact + cells;
    double* r_weight = r_round + cells;
    const dim3 grid((unsigned)cdiv((int64_t)cells, 256));
    switch (dtype) {
        case FAD_F16: hipLaunchKernelGGL((file_mean_rows<FAD_F16>), grid, dim3(256), 0, st, dsums, dsizes, n_files, d, r_exact, r_round, r_weight, druns); break;
        case FAD_BF16: hipLaunchKernelGGL((file_mean_rows<FAD_BF16>), grid, dim3(256), 0, st, dsums, dsizes, n_files, d, r_exact, r_round, r_weight, druns); break;
        case FAD_F32: hipLaunchKernelGGL((file_mean_rows<FAD_F32>), grid, dim3(256), 0, st, dsums, dsizes, n_files, d, r_exact, r_round, r_weight, druns); break;
        default: hipLaunchKernelGGL((file_mean_rows<FAD_F64>), grid, dim3(256), 0, st, dsums, dsizes, n_files, d, r_exact, r_round, r_weight, (const float*)nullptr); break;
    }
    FAD_HIP_TRY(hipGetLastError());
    fad_moments* hs[3] = {exact, rounded, weighted};
    const void* rows[3] = {r_exact, r_round, r_weight};
    const int64_t ns[3] = {n_files, n_files, n_files};
    const int64_t lds[3] = {d, d, d};
    FAD_TRY(update_device_multi(3, hs, rows, ns, lds, FAD_F64, st));
    if (!sums_dev || (seg_runsums && !runs_dev)) FAD_HIP_TRY(hipStreamSynchronize(st));          // the caller's host arrays were read asynchronously
    return FAD_OK;
}

int fad_moments_update_file_means(fad_moments_t* exact, fad_moments_t* rounded, fad_moments_t* weighted,
                                  const double* seg_sums, const int64_t* sizes, int64_t n_files, int dtype,
                                  int on_device, void* stream) {
    return update_file_means_impl(exact, rounded, weighted, seg_sums, nullptr, sizes, n_files, dtype, on_device & 3, stream);
}

int fad_moments_update_file_means_ref(fad_moments_t* exact, fad_moments_t* rounded, fad_moments_t* weighted,
                                      const double* seg_sums, const float* seg_runsums, const int64_t* sizes, int64_t n_files, int dtype,
                                      int on_device, void* stream) {
    return update_file_means_impl(exact, rounded, weighted, seg_sums, seg_runsums, sizes, n_files, dtype, on_device, stream);
}

int fad_moments_merge(fad_moments_t* dst, const fad_moments_t* src, void* stream) {
    if (!dst || !src) return set_error(FAD_ERR_INVALID, "handle is NULL");
    if (dst->d != src->d) return set_error(FAD_ERR_SHAPE, "d mismatch %d vs %d", dst->d, src->d);
    if (dst->device != src->device) return set_error(FAD_ERR_INVALID, "handles live on different devices; export/import instead");
    DeviceGuard g(dst->device);
    const int64_t len = packed_len(dst->d);
    FAD_TRY(settle(dst, static_cast<hipStream_t>(stream)));
    FAD_TRY(settle(src, static_cast<hipStream_t>(stream)));
    // (rows from another handle have no place in dst's row order: numpy's running sums no longer cover what the accumulator holds --
    //  finalize and the Frechet entry points fall back to the exact mean, as after import / allreduce.  An EMPTY src changes nothing,
    //  but whether it is empty is known on the device only: any merge gives the order up.)
    dst->runsum_covers = false;
    hipLaunchKernelGGL(packed_axpy, dim3((unsigned)cdiv(len, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       dst->acc, src->acc, len);
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}

int fad_moments_export(const fad_moments_t* h, double* packed, int on_device, void* stream) {
    if (!h || !packed) return set_error(FAD_ERR_INVALID, "NULL argument");
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bytes = (size_t)packed_len(h->d) * sizeof(double);
    FAD_TRY(settle(h, st));
    FAD_HIP_TRY(hipMemcpyAsync(packed, h->acc, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (!on_device) FAD_HIP_TRY(hipStreamSynchronize(st));
    return FAD_OK;
}

int fad_moments_import(fad_moments_t* h, const double* packed, int on_device, void* stream) {
    if (!h || !packed) return set_error(FAD_ERR_INVALID, "NULL argument");
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bytes = (size_t)packed_len(h->d) * sizeof(double);
    h->fresh = false;                              // the whole accumulator is overwritten
    h->runsum_covers = false;                      // (statistics from elsewhere: no row order to follow)
    FAD_HIP_TRY(hipMemcpyAsync(h->acc, packed, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!on_device) FAD_HIP_TRY(hipStreamSynchronize(st));
    return FAD_OK;
}

int fad_moments_allreduce(fad_moments_t* h, void* rccl_comm, void* stream) {
    if (!h || !rccl_comm) return set_error(FAD_ERR_INVALID, "NULL argument");
    // ncclResult_t ncclAllReduce(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t)
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    static allreduce_fn fn = [] {
        void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");          // the RCCL the host process uses (e.g. torch's)
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            if (sym) break;
            if (void* lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) sym = dlsym(lib, "ncclAllReduce");
        }
        return reinterpret_cast<allreduce_fn>(sym);
    }();
    if (!fn) return set_error(FAD_ERR_INVALID, "no RCCL in this process (ncclAllReduce not found)");
    h->runsum_covers = false;                      // (the sum of several ranks' statistics has no row order)
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FAD_TRY(settle(h, st));
    constexpr int kNcclFloat64 = 8, kNcclSum = 0;                   // rccl.h: ncclDataType_t / ncclRedOp_t
    const int rc = fn(h->acc, h->acc, (size_t)packed_len(h->d), kNcclFloat64, kNcclSum, rccl_comm, st);
    if (rc != 0) return set_error(FAD_ERR_HIP, "ncclAllReduce failed with ncclResult_t %d", rc);
    return FAD_OK;
}

int fad_moments_count(const fad_moments_t* h, int64_t* n, void* stream) {
    if (!h || !n) return set_error(FAD_ERR_INVALID, "NULL argument");
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double v = 0.0;
    FAD_TRY(settle(h, st));
    FAD_HIP_TRY(hipMemcpyAsync(&v, h->acc, sizeof(double), hipMemcpyDeviceToHost, st));
    FAD_HIP_TRY(hipStreamSynchronize(st));
    *n = (int64_t)(v + 0.5);
    return FAD_OK;
}

int fad_moments_finalize(const fad_moments_t* h, int ddof, double* mu, double* cov, int64_t* n_out,
                         int on_device, void* stream) {
    if (!h || !cov) return set_error(FAD_ERR_INVALID, "NULL argument");
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t n = 0;
    FAD_TRY(fad_moments_count(h, &n, stream));
    if (n_out) *n_out = n;
    if (n < 2) return set_error(FAD_ERR_TOO_FEW_ROWS, "FAD requires at least two embedding window frames, you have %lld", (long long)n);
    const int d = h->d;
    fad_moments* hm = const_cast<fad_moments*>(h);
    double* dmu = mu; double* dcov = cov;
    if (!on_device) {
        FAD_TRY(hm->scratch.reserve(((size_t)d * d + d) * sizeof(double)));
        hm->sizes_cached_at = nullptr;             // (the scratch area is overwritten: a cached sizes upload is gone)
        dcov = static_cast<double*>(hm->scratch.p);
        dmu = dcov + (size_t)d * d;
    }
    hipLaunchKernelGGL(moments_finalize_kernel, dim3((unsigned)cdiv((int64_t)d * d, 256)), dim3(256), 0, st,
                       h->acc, d, ddof, dmu, dcov, (h->ref_mean && h->runsum_covers && h->runsum_live && !h->fresh) ? static_cast<const float*>(h->runsum.p) : nullptr);
    FAD_HIP_TRY(hipGetLastError());
    if (!on_device) {
        FAD_HIP_TRY(hipMemcpyAsync(cov, dcov, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, st));
        if (mu) FAD_HIP_TRY(hipMemcpyAsync(mu, dmu, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
        FAD_HIP_TRY(hipStreamSynchronize(st));
    }
    return FAD_OK;
}

int fad_moments_trim(fad_moments_t* h, int64_t keep_bytes) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    DeviceGuard g(h->device);
    if (keep_bytes < 0) keep_bytes = 0;
    if (h->stage.cap > (size_t)keep_bytes || h->scratch.cap > (size_t)keep_bytes) {
        FAD_HIP_TRY(hipDeviceSynchronize());       // nothing enqueued may still read what is freed
        if (h->stage.cap > (size_t)keep_bytes) h->stage.release();
        if (h->scratch.cap > (size_t)keep_bytes) { h->scratch.release(); h->sizes_cached_at = nullptr; }
    }
    return FAD_OK;
}

int fad_moments_set_reference_mean(fad_moments_t* h, int enabled) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    h->ref_mean = enabled != 0;
    h->ref_detached = enabled == 2;
    return FAD_OK;
}

int fad_moments_set_timing(fad_moments_t* h, int enabled) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    h->timing = (enabled == 2) ? 2 : (enabled != 0 ? 1 : 0);
    h->ev_count = 0;
    if (h->timing && !h->ev) {
        // the ring of events is created HERE, not by the first timed update: 768 hipEventCreate calls took ~0.35 ms out of
        // bench.py's timed region (round 3: the timed block read 8-10 % below the same block repeated without them)
        DeviceGuard g(h->device);
        h->ev = new (std::nothrow) hipEvent_t[fad_moments::kRing * 3]();
        if (!h->ev) return set_error(FAD_ERR_ALLOC, "out of host memory");
        for (int i = 0; i < fad_moments::kRing * 3; ++i) FAD_HIP_TRY(hipEventCreate(&h->ev[i]));
    }
    return FAD_OK;
}

// Average duration of the tile kernel and of the reduce kernels over every update recorded since
// timing was enabled / last queried (at most the last 256).  Synchronises on the newest event.
int fad_moments_last_timing(fad_moments_t* h, float* ms_main, float* ms_reduce, int* variant) {
    if (!h) return set_error(FAD_ERR_INVALID, "handle is NULL");
    if (!h->timing || !h->ev || h->ev_count == 0)
        return set_error(FAD_ERR_INVALID, "timing was not enabled before the update");
    DeviceGuard g(h->device);
    const int total = h->ev_count;
    const int m = total < fad_moments::kRing ? total : fad_moments::kRing;
    const bool with_reduce = h->timing == 1;
    FAD_HIP_TRY(hipEventSynchronize(h->ev[3 * ((total - 1) % fad_moments::kRing) + (with_reduce ? 2 : 1)]));
    double a = 0.0, b = 0.0;
    for (int i = total - m; i < total; ++i) {
        hipEvent_t* e = h->ev + 3 * (i % fad_moments::kRing);
        float x = 0.f, y = 0.f;
        FAD_HIP_TRY(hipEventElapsedTime(&x, e[0], e[1]));
        if (with_reduce) FAD_HIP_TRY(hipEventElapsedTime(&y, e[1], e[2]));
        a += x; b += y;
    }
    if (ms_main) *ms_main = (float)(a / m);
    if (ms_reduce) *ms_reduce = (float)(b / m);
    if (variant) *variant = h->last_variant;
    h->ev_count = 0;
    return FAD_OK;
}

}  // extern "C"

// accessors for the other translation units (frechet.hip)
namespace fad {
const double* moments_packed(const fad_moments* h) { return h->acc; }
int moments_settle(const fad_moments* h, hipStream_t st) { return settle(h, st); }
int moments_mark_read(const fad_moments* hc, hipStream_t st) {
    fad_moments* h = const_cast<fad_moments*>(hc);
    if (!h->ref_mean || !h->ref_detached) return FAD_OK;             // (everything else is ordered on the caller's stream already)
    if (!h->rs_reader) FAD_HIP_TRY(hipEventCreateWithFlags(&h->rs_reader, hipEventDisableTiming));
    FAD_HIP_TRY(hipEventRecord(h->rs_reader, st));
    h->rs_reader_set = true;
    return FAD_OK;
}
const float* moments_runsum(const fad_moments* h) {
    return (h->ref_mean && h->runsum_covers && h->runsum_live && !h->fresh) ? static_cast<const float*>(h->runsum.p) : nullptr;
}
int moments_device(const fad_moments* h) { return h->device; }
int moments_dim(const fad_moments* h) { return h->d; }
}

// ==========================================================================================
// Covariances of B songs of float16 frames on the tile kernels (moments_kernels.h: song_cov_*); for frechet.hip's batched per-song
// chain.  rows: 16-byte aligned, ld and d multiples of 8; mean_exact [song][d] and offsets on the device; cov_out [B][d * d].
// ==========================================================================================
namespace fad {
bool song_cov_f16_ok(const void* rows, int64_t ld, int d) {
    return d % 8 == 0 && ld % 8 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15u) == 0 && ld < ((int64_t)1 << 26);
}
int song_cov_f16_launch(const void* rows, int64_t ld, int d, const int64_t* d_offsets, const int64_t* d_song_ids, int64_t B,
                        int64_t max_frames, const double* d_mean_exact, const double* d_var_exact, double* d_cov_out, DevBuf& scratch,
                        int device, hipStream_t st) {
    if (B <= 0) return FAD_OK;
    {
        static std::mutex mu;
        static bool done[64] = {false};
        std::lock_guard<std::mutex> lk(mu);
        if (device < 0 || device >= 64) return set_error(FAD_ERR_INVALID, "device %d out of range", device);
        if (!done[device]) {
            FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&song_cov_tile<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrLds));
            FAD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&song_cov_tile<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrLds));
            done[device] = true;
        }
    }
    SongCovLaunch L;
    L.rows = static_cast<const uint16_t*>(rows); L.ld = ld; L.d = d;
    L.nt = (d + H_BT - 1) / H_BT; L.T = L.nt * (L.nt + 1) / 2;
    int64_t S = (max_frames + 4095) / 4096;
    L.S = (int)(S < 1 ? 1 : (S > 64 ? 64 : S));
    L.offsets = d_offsets; L.song_ids = d_song_ids; L.mean_exact = d_mean_exact; L.var_exact = d_var_exact; L.cov_out = d_cov_out;
    const size_t dpad = (size_t)L.nt * H_BT, runs = (size_t)B * L.S;
    const size_t b_part = (runs * L.T * H_TS * sizeof(float) + 255) & ~(size_t)255, b_col = (runs * dpad * sizeof(double) + 255) & ~(size_t)255;
    FAD_TRY(scratch.reserve(b_part + b_col + runs * dpad * sizeof(uint16_t) + 256));
    char* base = static_cast<char*>(scratch.p);
    L.partials = reinterpret_cast<float*>(base); L.colpart = reinterpret_cast<double*>(base + b_part);
    L.cvec = reinterpret_cast<uint16_t*>(base + b_part + b_col);
    hipLaunchKernelGGL(song_cov_shift, dim3((unsigned)B), dim3(256), 0, st, L);
    if (L.T > 1) hipLaunchKernelGGL(song_cov_tile<true>, dim3((unsigned)L.T, (unsigned)L.S, (unsigned)B), dim3(256), kTrLds, st, L);
    else hipLaunchKernelGGL(song_cov_tile<false>, dim3(1, (unsigned)L.S, (unsigned)B), dim3(256), kTrLds, st, L);
    hipLaunchKernelGGL(song_cov_finish, dim3((unsigned)(L.T * 16), (unsigned)B), dim3(256), 0, st, L);
    FAD_HIP_TRY(hipGetLastError());
    return FAD_OK;
}
// (first-use warm-up, common.cpp: warm_code_objects -- loading this translation unit's code object costs ~75 ms at the first launch)
const void* code_object_anchor_moments() { return reinterpret_cast<const void*>(&packed_axpy); }
}  // namespace fad
