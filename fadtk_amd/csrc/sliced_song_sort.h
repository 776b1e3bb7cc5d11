// The resident song sort of the per-song sliced Wasserstein distance (fad_sliced_individual): the projections of all
// song rows on one direction are one row of P [dirs x pitch]; the keys of song s are the columns [offsets[s], offsets[s + 1]) of every
// row, and every song's range of every row is sorted ascending on its own, in the order of sliced_sort.h's key_image (-0 before +0, any
// bit pattern sorts somewhere).  Keys only.
//
//   - units:   the host cuts the songs into units, the same for every direction (build_units).  A unit is a run of consecutive songs
//              whose keys together fit the resident capacity kCapacity = 4096 and that has at most kMaxSlots = 256 songs with keys; a
//              song that fits is never cut, songs without keys belong to no unit, and a song of more than kCapacity keys ends the run
//              before it and goes to the caller's long path (sliced_sort.h's global sort, one call per such song).
//   - sort:    one workgroup of 512 threads takes (direction, unit).  It reads the unit's keys once, coalesced, through key_image into
//              LDS, sorts them there with the four 8-bit LSD passes of sliced_sort.h between two LDS buffers, and writes them back once,
//              coalesced, through key_bits, in place.  A pass is a 256-bin histogram (integer LDS atomics), its exclusive scan, and
//              rounds of 512 keys placed by sliced_sort.h's rule: base of the digit + keys of that digit in earlier rounds + in earlier
//              waves of the round + in lower lanes of the wave (8 ballots).  The place is a function of the key's index alone: stable,
//              nothing is placed by order of arrival, the output does not depend on timing.
//   - slots:   in a unit of several songs every key carries the number of its song within the unit (a byte, found by bisection of the
//              unit's song ends when the key is read), and a fifth stable pass on that byte follows the four key passes: the keys end up
//              ordered by (song, key), and as a song's keys began in its own range they end there.  256 two-key songs cost what one
//              512-key song costs, plus that pass.
// LDS: 2 x 16 KiB of keys, 2 x 4 KiB of slot bytes, 1 KiB of song ends, 1 KiB of places, 8 KiB of wave counts = 50 KiB: three workgroups
// (24 waves) share a CU's 160 KiB, and a 2250-key song fits.  Nothing here is a template of the callers' dtype: the header stands on
// sliced_sort.h alone (tests/native/sliced_song_sort_check.hip includes only the two).
#pragma once

#include "sliced_sort.h"

#include <vector>

namespace fad {
namespace songsort {

constexpr int kThreads = 512;                  // a round: one key per thread
constexpr int kWaves = kThreads / 64;
constexpr int kCapacity = 4096;                // keys a unit holds at most (C)
constexpr int kMaxSlots = 256;                 // songs with keys per unit at most: the slot is one digit

struct Unit {
    int64_t k0;                                // the unit's first key (a column of P)
    int32_t nk;                                // its keys, 1 .. kCapacity
    int32_t e0;                                // where its songs' ends (relative to k0, ascending, the last is nk) begin in `ends`
    int32_t ns;                                // its songs with keys, 1 .. kMaxSlots
    int32_t pad;
};

struct Table {
    std::vector<Unit> units;
    std::vector<int32_t> ends;
    std::vector<int64_t> long_songs;           // songs of more than kCapacity keys, ascending
    int64_t most_songs = 0;                    // most songs with keys in one unit
};

// offsets [n_songs + 1] starts at 0 and never decreases (the caller checked)
inline Table build_units(const int64_t* offsets, int64_t n_songs) {
    Table t;
    Unit cur{0, 0, 0, 0, 0};
    auto close = [&]() {
        if (cur.ns > 0) {
            t.units.push_back(cur);
            if (cur.ns > t.most_songs) t.most_songs = cur.ns;
        }
        cur = Unit{0, 0, (int32_t)t.ends.size(), 0, 0};
    };
    for (int64_t s = 0; s < n_songs; ++s) {
        const int64_t m = offsets[s + 1] - offsets[s];
        if (m == 0) continue;
        if (m > kCapacity) { close(); t.long_songs.push_back(s); continue; }
        if (cur.ns > 0 && (cur.nk + m > kCapacity || cur.ns == kMaxSlots)) close();
        if (cur.ns == 0) cur.k0 = offsets[s];
        cur.nk += (int32_t)m;
        cur.ns += 1;
        t.ends.push_back(cur.nk);
    }
    close();
    return t;
}

#if defined(__HIPCC__)
// P [dirs x pitch]; workgroup b takes direction b / n_units, unit b % n_units
__global__ void __launch_bounds__(kThreads) sort_units_kernel(float* __restrict__ P, int64_t pitch, const Unit* __restrict__ units,
                                                              const int32_t* __restrict__ ends, int64_t n_units) {
    __shared__ uint32_t key[2][kCapacity];
    __shared__ unsigned char slot[2][kCapacity];
    __shared__ int send[kMaxSlots];
    __shared__ unsigned int place[ssort::kRadix];          // where the next key of digit d goes
    __shared__ unsigned int wcnt[kWaves][ssort::kRadix];   // this round's keys of digit d in wave w
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Unit un = units[blockIdx.x % n_units];
    uint32_t* g = reinterpret_cast<uint32_t*>(P) + (blockIdx.x / n_units) * pitch + un.k0;
    const int nk = un.nk < kCapacity ? un.nk : kCapacity;  // always un.nk; keeps a wrong table inside the buffers
    const int ns = un.ns < kMaxSlots ? un.ns : kMaxSlots;
    const bool multi = ns > 1;

    if (tid < ns) send[tid] = ends[un.e0 + tid];
    __syncthreads();
    for (int i = tid; i < nk; i += kThreads) {
        key[0][i] = ssort::key_image(g[i]);
        if (multi) {
            int lo = 0, hi = ns - 1;                       // the first song whose end is beyond i
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (send[mid] > i) hi = mid; else lo = mid + 1;
            }
            slot[0][i] = (unsigned char)lo;
        }
    }

    const int passes = multi ? ssort::kPasses + 1 : ssort::kPasses;
    for (int pass = 0; pass < passes; ++pass) {
        const int src = pass & 1, dst = src ^ 1;
        const bool by_slot = pass == ssort::kPasses;
        const int shift = 8 * pass;
        if (tid < ssort::kRadix) place[tid] = 0;
        for (int w = 0; w < kWaves; ++w)
            if (tid < ssort::kRadix) wcnt[w][tid] = 0;
        __syncthreads();                                   // also: the keys of the previous pass (or the load) are in LDS
        for (int i = tid; i < nk; i += kThreads) {
            const unsigned int d = by_slot ? slot[src][i] : (key[src][i] >> shift) & 0xffu;
            atomicAdd(&place[d], 1u);                      // integer counts: order does not matter
        }
        __syncthreads();
        const unsigned int own = tid < ssort::kRadix ? place[tid] : 0u;
        for (int off = 1; off < ssort::kRadix; off <<= 1) {                           // inclusive scan over the digits
            const unsigned int v = (tid < ssort::kRadix && tid >= off) ? place[tid - off] : 0u;
            __syncthreads();
            if (tid < ssort::kRadix) place[tid] += v;
            __syncthreads();
        }
        if (tid < ssort::kRadix) place[tid] -= own;
        __syncthreads();
        for (int i0 = 0; i0 < nk; i0 += kThreads) {        // uniform over the workgroup
            const bool live = i0 + tid < nk;
            const uint32_t k = live ? key[src][i0 + tid] : 0u;
            const unsigned int sl = (live && multi) ? slot[src][i0 + tid] : 0u;
            const unsigned int d = by_slot ? sl : (k >> shift) & 0xffu;
            unsigned long long peers = __ballot(live);     // the live lanes of the wave with this lane's digit
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const unsigned long long has = __ballot(live && bit);
                peers &= bit ? has : ~has;
            }
            const unsigned int below = (unsigned int)__popcll(peers & ((1ull << lane) - 1ull));
            if (live && below == 0) wcnt[wave][d] = (unsigned int)__popcll(peers);
            __syncthreads();
            if (live) {
                unsigned int at = place[d] + below;
                for (int w = 0; w < wave; ++w) at += wcnt[w][d];
                if (at < (unsigned int)nk) {               // always true; keeps a wrong count inside the buffers
                    key[dst][at] = k;
                    if (multi) slot[dst][at] = (unsigned char)sl;
                }
            }
            __syncthreads();
            if (tid < ssort::kRadix) {
                unsigned int add = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) { add += wcnt[w][tid]; wcnt[w][tid] = 0; }
                place[tid] += add;
            }
            __syncthreads();
        }
    }
    const int fin = passes & 1;
    for (int i = tid; i < nk; i += kThreads) g[i] = ssort::key_bits(key[fin][i]);
}

// every unit of `dirs` rows of P sorted in place; units_d / ends_d hold the table's units and ends on the device.  Enqueued on `st`.
inline hipError_t sort_units(float* P, int64_t pitch, int64_t dirs, const Unit* units_d, const int32_t* ends_d, int64_t n_units,
                             hipStream_t st) {
    if (dirs < 1 || n_units < 1) return hipSuccess;
    const int64_t per = (int64_t)0x7fffffff / n_units;     // directions per launch: the grid's x extent
    if (per < 1) return hipErrorInvalidValue;
    for (int64_t l0 = 0; l0 < dirs; l0 += per) {
        const int64_t cur = dirs - l0 < per ? dirs - l0 : per;
        sort_units_kernel<<<(unsigned int)(cur * n_units), kThreads, 0, st>>>(P + l0 * pitch, pitch, units_d, ends_d, n_units);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
#endif

}  // namespace songsort
}  // namespace fad
