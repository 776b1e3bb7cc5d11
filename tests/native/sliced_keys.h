// What the three native checks of the sliced sorts share (sliced_sort_check, sliced_sort_pairs_check, sliced_song_sort_check): the
// HIP call check, the guard word, the pass / fail counters and the key families.  Included after the header under test.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s failed: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

static const uint32_t kGuard = 0x7fc0dead;                 // a NaN payload no generator below produces on purpose, and no valid position
static int g_checks = 0, g_fail = 0;

// one check: counted, and named where it fails
static void expect(bool ok, const char* what) {
    ++g_checks;
    if (!ok) { ++g_fail; printf("FAILED %s\n", what); }
}

// the check of one run: `bad` words differ from what they should be
static void expect_none(int bad, const char* what, int kind, int64_t a, int64_t b) {
    char text[96];
    snprintf(text, sizeof(text), "kind %d %s %lld x %lld: %d words differ", kind, what, (long long)a, (long long)b, bad);
    expect(bad == 0, text);
}

// the last lines of every check and its exit status
static int report() {
    printf("%d checks, %d failed\n", g_checks, g_fail);
    if (g_fail) printf("%d checks FAILED\n", g_fail); else printf("all checks passed\n");
    return g_fail ? 1 : 0;
}

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// kind 2: a few special values
static const float kSpecial[12] = {0.f, -0.f, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, 1.f, -1.f, INFINITY, -INFINITY, 1e-45f, -1e-45f};

// kinds 3 .. 6 before any fix-up: three bytes shared over the segment, byte (kind - 3) alone differs; the word may be a NaN pattern
static uint32_t shared_bytes_key(int kind, int64_t s, std::mt19937& rng) {
    const int b = kind - 3;
    const uint32_t u = 0x40490fdbu ^ (((uint32_t)s * 0x01010101u) & 0x7f7f7f7fu);
    return (u & ~(0xffu << (8 * b))) | ((rng() & 0xffu) << (8 * b));
}

// key set `kind` (0 .. 10) for segment s, element i of n: no NaN, which is not ordered
static uint32_t make_key(int kind, int64_t s, int64_t i, int64_t n, std::mt19937& rng) {
    switch (kind) {
        case 0: {
            uint32_t u = rng();
            if ((u & 0x7f800000u) == 0x7f800000u) u &= 0xff7fffffu;
            return u;
        }
        case 1: return (rng() & 0x807fffffu);                                         // denormals and zeros of both signs
        case 2: return bits_of(kSpecial[rng() % 12]);                                 // many ties
        case 3: case 4: case 5: case 6: {
            uint32_t u = shared_bytes_key(kind, s, rng);
            if ((u & 0x7f800000u) == 0x7f800000u) u ^= 0x00800000u;
            return u;
        }
        case 7: return bits_of(-3.5f);                                                // all equal
        case 8: return bits_of((float)(i - n / 2) * 0.25f);                           // sorted
        case 9: return bits_of((float)(n / 2 - i) * 0.25f);                           // reversed
        default: return bits_of((rng() & 1u) ? 2.0f : -0.0f);                         // two-valued
    }
}
