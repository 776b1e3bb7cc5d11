// The segmented radix sort of fadtk_amd/csrc/sliced_sort.h on its own, below fad_sliced_wasserstein: this file includes that header and
// nothing else of the library.  Every segment's output is compared bit for bit with std::sort of the mapped uint32 keys (mapped back),
// over key sets the public entry cannot produce -- denormals, -0 and +0 together, +-FLT_MAX and infinities, keys that share three of
// their four bytes (one digit alone decides, per byte position), all keys equal, sorted and reversed input -- at segment counts 1, 3 and
// 65 and segment lengths on both sides of a round (256), a workgroup's share (2048) and several workgroups per segment.  The words
// after each segment (the pitch is longer than the segment) and the guard words around the buffers must come back untouched.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/sliced_sort_check tests/native/sliced_sort_check.hip
#include "../../fadtk_amd/csrc/sliced_sort.h"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace fad;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s failed: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

static const uint32_t kGuard = 0x7fc0dead;                 // a NaN payload no generator below produces
static int g_checks = 0, g_fail = 0;

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// key set `kind` for segment s, element i of n
static uint32_t make_key(int kind, int64_t s, int64_t i, int64_t n, std::mt19937& rng) {
    switch (kind) {
        case 0: {
            uint32_t u = rng();
            if ((u & 0x7f800000u) == 0x7f800000u) u &= 0xff7fffffu;                   // no NaN: not ordered
            return u;
        }
        case 1: return (rng() & 0x807fffffu);                                         // denormals and zeros of both signs
        case 2: {                                                                     // a few special values, many ties
            static const float v[] = {0.f, -0.f, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, 1.f, -1.f, INFINITY, -INFINITY, 1e-45f, -1e-45f};
            return bits_of(v[rng() % 12]);
        }
        case 3: case 4: case 5: case 6: {                                             // three bytes shared: byte (kind - 3) alone differs
            const int b = kind - 3;
            uint32_t u = 0x40490fdbu ^ (((uint32_t)s * 0x01010101u) & 0x7f7f7f7fu);
            u = (u & ~(0xffu << (8 * b))) | ((rng() & 0xffu) << (8 * b));
            if ((u & 0x7f800000u) == 0x7f800000u) u ^= 0x00800000u;
            return u;
        }
        case 7: return bits_of(-3.5f);                                                // all equal
        case 8: return bits_of((float)(i - n / 2) * 0.25f);                           // sorted
        default: return bits_of((float)(n / 2 - i) * 0.25f);                          // reversed
    }
}

static int run(int kind, int64_t n, int64_t segs) {
    const int64_t pitch = n + 5, guard = 64;
    const int64_t total = segs * pitch + 2 * guard;
    std::mt19937 rng((uint32_t)(kind * 1000003 + n * 131 + segs));
    std::vector<uint32_t> host((size_t)total, kGuard), back((size_t)total), back_tmp((size_t)total);
    for (int64_t s = 0; s < segs; ++s)
        for (int64_t i = 0; i < n; ++i) host[(size_t)(guard + s * pitch + i)] = make_key(kind, s, i, n, rng);
    uint32_t *keys, *tmp, *counts, *bases;
    const int64_t nc = ssort::counts_elems(n, segs), nb = ssort::bases_elems(segs);
    CK(hipMalloc(&keys, (size_t)total * 4));
    CK(hipMalloc(&tmp, (size_t)total * 4));
    CK(hipMalloc(&counts, (size_t)(nc + guard) * 4));
    CK(hipMalloc(&bases, (size_t)(nb + guard) * 4));
    std::vector<uint32_t> fill((size_t)std::max<int64_t>(total, std::max(nc, nb) + guard), kGuard);
    CK(hipMemcpy(keys, host.data(), (size_t)total * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(tmp, fill.data(), (size_t)total * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(counts, fill.data(), (size_t)(nc + guard) * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(bases, fill.data(), (size_t)(nb + guard) * 4, hipMemcpyHostToDevice));
    CK(ssort::sort_segments(reinterpret_cast<float*>(keys + guard), reinterpret_cast<float*>(tmp + guard), pitch, n, segs, counts, bases, nullptr));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(back.data(), keys, (size_t)total * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(back_tmp.data(), tmp, (size_t)total * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> cg((size_t)guard), bg((size_t)guard);
    CK(hipMemcpy(cg.data(), counts + nc, (size_t)guard * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(bg.data(), bases + nb, (size_t)guard * 4, hipMemcpyDeviceToHost));
    CK(hipFree(keys)); CK(hipFree(tmp)); CK(hipFree(counts)); CK(hipFree(bases));

    int bad = 0;
    std::vector<uint32_t> want((size_t)n);
    for (int64_t s = 0; s < segs; ++s) {
        for (int64_t i = 0; i < n; ++i) want[(size_t)i] = ssort::key_image(host[(size_t)(guard + s * pitch + i)]);
        std::sort(want.begin(), want.end());
        for (int64_t i = 0; i < n; ++i) bad += back[(size_t)(guard + s * pitch + i)] != ssort::key_bits(want[(size_t)i]);
        for (int64_t i = n; i < pitch; ++i) bad += back[(size_t)(guard + s * pitch + i)] != kGuard || back_tmp[(size_t)(guard + s * pitch + i)] != kGuard;
    }
    for (int64_t i = 0; i < guard; ++i)
        bad += back[(size_t)i] != kGuard || back[(size_t)(total - 1 - i)] != kGuard || back_tmp[(size_t)i] != kGuard ||
               back_tmp[(size_t)(total - 1 - i)] != kGuard || cg[(size_t)i] != kGuard || bg[(size_t)i] != kGuard;
    ++g_checks;
    if (bad) { ++g_fail; printf("FAILED kind %d n %lld segs %lld: %d words differ\n", kind, (long long)n, (long long)segs, bad); }
    return 0;
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    // the map itself: order and round trip on the host
    {
        const float v[] = {-INFINITY, -FLT_MAX, -1.f, -FLT_MIN, -1e-45f, -0.f, 0.f, 1e-45f, FLT_MIN, 1.f, FLT_MAX, INFINITY};
        for (int i = 0; i < 12; ++i) {
            ++g_checks;
            const uint32_t k = ssort::key_image(bits_of(v[i]));
            if (ssort::key_bits(k) != bits_of(v[i]) || (i && !(ssort::key_image(bits_of(v[i - 1])) < k))) { ++g_fail; printf("FAILED map at %d\n", i); }
        }
    }
    const int64_t lengths[] = {1, 2, 63, 255, 256, 257, 2047, 2048, 2049, 4100, 10007};
    const int64_t counts[] = {1, 3, 65};
    for (int kind = 0; kind < 10; ++kind)
        for (int64_t n : lengths)
            for (int64_t segs : counts) {
                if (n > 4100 && segs > 3) continue;
                const int rc = run(kind, n, segs);
                if (rc) return rc;
            }
    printf("%d checks, %d failed\n", g_checks, g_fail);
    if (g_fail) printf("%d checks FAILED\n", g_fail); else printf("all checks passed\n");
    return g_fail ? 1 : 0;
}
