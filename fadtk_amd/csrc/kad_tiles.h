// Which 128 x 128 tile of a KAD pair space a workgroup takes, and how a pass is cut into launches -- plain C++, shared by the
// device code (kad.hip), the host's launch plan and the CPU test of the coverage (tests/native_cpu/kad_tiles_cover.cpp).
//
// Two pair spaces:
//   triangle  (XX, YY, and the median's histogram passes): the tiles (I, J >= I) of a T x T block grid, numbered row-major
//             u = I*T - I*(I-1)/2 + (J - I).  A tile I < J takes all its pairs; a diagonal tile I == J only j > i.
//   rectangle (XY): the tiles (I, J) of a TI x TJ grid, u = I*TJ + J.
// A pass is cut into launches of at most `per_launch` consecutive tiles [u0, u0 + cnt).  Inside a launch workgroup slot L runs on
// XCD L % 8 and is that XCD's (L / 8)-th: XCD x takes the stretch [x*per, (x+1)*per) of the launch's tiles (per = ceil(cnt / 8)),
// so consecutive workgroups of one XCD walk consecutive tiles of a row block and its L2 fetches the A panel once for all of them.
// A persistent grid of G workgroups (G a multiple of 8) walks L = w, w + G, w + 2G, ... < 8 * per: every L stays on the XCD of w.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define KAD_HD __host__ __device__
#else
#define KAD_HD
#endif

namespace fad {
namespace kad {

constexpr int kTile = 128;         // rows of X (and of Y) per tile side
constexpr int kXcds = 8;

struct Tile { int64_t I, J; bool live; };

KAD_HD inline int64_t blocks(int64_t n) { return (n + kTile - 1) / kTile; }
KAD_HD inline int64_t tri_tiles(int64_t T) { return T * (T + 1) / 2; }
KAD_HD inline int64_t tri_row_start(int64_t I, int64_t T) { return I * T - I * (I - 1) / 2; }

// u -> (I, J >= I) of the row-major upper triangle of a T x T grid (0 <= u < tri_tiles(T))
KAD_HD inline Tile tri_tile(int64_t u, int64_t T) {
    const double b = 2.0 * (double)T + 1.0;
    int64_t I = (int64_t)((b - sqrt(b * b - 8.0 * (double)u)) * 0.5);
    if (I < 0) I = 0;
    if (I > T - 1) I = T - 1;
    while (I > 0 && tri_row_start(I, T) > u) --I;                 // the double root is off by at most one either way
    while (I + 1 < T && tri_row_start(I + 1, T) <= u) ++I;
    return Tile{I, I + (u - tri_row_start(I, T)), true};
}

KAD_HD inline Tile rect_tile(int64_t u, int64_t TJ) { return Tile{u / TJ, u % TJ, true}; }

// slots of a launch of `cnt` tiles: 8 * per of them, the last few of some XCDs idle
KAD_HD inline int64_t launch_per_xcd(int64_t cnt) { return (cnt + kXcds - 1) / kXcds; }
KAD_HD inline int64_t launch_slots(int64_t cnt) { return kXcds * launch_per_xcd(cnt); }

// the launch-local tile index of slot L (live = false: an idle slot)
KAD_HD inline int64_t slot_tile(int64_t L, int64_t cnt, bool* live) {
    const int64_t per = launch_per_xcd(cnt), x = L % kXcds, idx = L / kXcds, v = x * per + idx;
    *live = idx < per && v < cnt;
    return v;
}

// persistent workgroups of a launch: a multiple of 8, at most `cap` (itself a multiple of 8), never more than the slots
KAD_HD inline int64_t launch_grid(int64_t cnt, int64_t cap) {
    const int64_t s = launch_slots(cnt);
    return s < cap ? s : cap;
}

// host only: what kad::launches planned on this thread since the last reset_plan_tally() -- kad.hip resets it at the start of every
// public entry and reports it through fad_kad_last_plan, so a test reads the cut a call really took instead of redoing the cost formula.
// A pass is one call of launches() with total > 0 (every pass of kad.hip plans its launches once; the median's three histogram rounds
// run the same plan and count as one pass).  walk = the slots one workgroup of a launch walks, launch_slots(cnt) / grid rounded up.
struct PlanTally { int64_t passes, launches, min_launches, max_launches, max_walk; };
inline PlanTally& plan_tally() {
    static thread_local PlanTally t{0, 0, 0, 0, 0};
    return t;
}
inline void reset_plan_tally() { plan_tally() = PlanTally{0, 0, 0, 0, 0}; }

// host only: the launches of a pass of `total` tiles (or work units, kad_song_tiles.h), `per_launch` at most each, and their grids
struct Launch { int64_t u0, cnt, grid; };
inline std::vector<Launch> launches(int64_t total, int64_t per_launch, int64_t cap) {
    std::vector<Launch> out;
    PlanTally& t = plan_tally();
    for (int64_t u0 = 0; u0 < total; u0 += per_launch) {
        const int64_t cnt = per_launch < total - u0 ? per_launch : total - u0;
        out.push_back(Launch{u0, cnt, launch_grid(cnt, cap)});
        const int64_t walk = (launch_slots(cnt) + out.back().grid - 1) / out.back().grid;
        if (walk > t.max_walk) t.max_walk = walk;
    }
    if (const int64_t nl = (int64_t)out.size()) {
        t.min_launches = t.passes == 0 || nl < t.min_launches ? nl : t.min_launches;
        t.max_launches = nl > t.max_launches ? nl : t.max_launches;
        t.passes += 1;
        t.launches += nl;
    }
    return out;
}

// Tiles per launch.  A tile costs its MFMA k loop -- `depth` units, 16x that for the float32 MFMA (a sixteenth of the 16-bit rate) --
// plus its epilogue: 128 units for the sums' 16384 exponentials, 2048 for a histogram pass's 16384 range tests and LDS atomics.
// The histogram weight is set from the slowest histogram launch measured at n = 100 000 (16.5 ms over 306 k tiles at D = 128 / 512,
// about 2.3x the slowest sum pass per tile, the LDS atomics of the first pass contending on a few bins).  Longest single launches
// measured on an MI355X: n = 10^6 at D = 128 / 64, 35 ms (sums) and 17 ms (histogram); 90 % identical rows, every
// count in one bin, 28 ms (histogram) -- no launch holds the GPU anywhere near 100 ms, n = 10^6 cuts into tens of launches per pass.
// PRDC's passes weigh their own epilogues: kTopkEpilogue for the radius pass's per-column top-k (a compare and a
// wave-uniform skip per pair, a 16-step insertion where a value enters), kFlagEpilogue for the cross pass's two threshold tests, counts
// and ballots per pair.  fad_nearest's cross pass weighs kNearestEpilogue: the top-k of 64-bit keys, a permlane swap
// per two pairs and a u64 compare per pair, six VALU ops per list entry where a key enters.  The Sinkhorn half-step
// weighs kSoftminEpilogue: a maximum, a subtraction, a multiply and an exponential per pair, against the sums' three instructions.
// The budget of cost units per launch is a host-side value of the calling thread, 2^30 unless set_launch_budget changed it: kad.hip
// sets it from FAD_KAD_LAUNCH_BUDGET at the start of every public entry (for tests: a small budget cuts a small pass into several
// launches), the CPU cover programs set it directly.  The floor of 64 tiles per launch holds at any budget.  Host only, as is
// everything that derives a launch size from it.
constexpr int64_t kSumEpilogue = 128, kHistEpilogue = 2048, kTopkEpilogue = 1024, kFlagEpilogue = 512, kNearestEpilogue = 1536,
                  kSoftminEpilogue = 192;
constexpr int64_t kLaunchBudget = (int64_t)1 << 30;
inline int64_t& launch_budget_value() {
    static thread_local int64_t v = kLaunchBudget;
    return v;
}
inline int64_t launch_budget() { return launch_budget_value(); }
inline void set_launch_budget(int64_t v) { launch_budget_value() = v > 0 ? v : kLaunchBudget; }
inline int64_t tiles_per_launch_for(int64_t depth, bool f32, int64_t epilogue) {
    const int64_t cost = (f32 ? 16 * depth : depth) + epilogue;
    const int64_t t = launch_budget() / cost;
    return t < 64 ? 64 : t;
}
inline int64_t tiles_per_launch(int64_t depth, bool f32, bool hist = false) {
    return tiles_per_launch_for(depth, f32, hist ? kHistEpilogue : kSumEpilogue);
}

// the pair (i, j) of rows inside tile (I, J) at local (r, c): counted or not
KAD_HD inline bool pair_counted(bool tri, int64_t I, int64_t J, int r, int c, int64_t n_rows, int64_t n_cols) {
    const int64_t i = I * kTile + r, j = J * kTile + c;
    if (i >= n_rows || j >= n_cols) return false;
    return !tri || I < J || c > r;
}

}  // namespace kad
}  // namespace fad
