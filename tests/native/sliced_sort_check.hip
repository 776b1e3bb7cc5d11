// The segmented radix sort of fadtk_amd/csrc/sliced_sort.h on its own, below fad_sliced_wasserstein: this file includes that header and
// nothing else of the library.  Every segment's output is compared bit for bit with std::sort of the mapped uint32 keys (mapped back),
// over key sets the public entry cannot produce (sliced_keys.h, kinds 0 .. 9) -- denormals, -0 and +0 together, +-FLT_MAX and infinities, keys that share three of
// their four bytes (one digit alone decides, per byte position), all keys equal, sorted and reversed input -- at segment counts 1, 3 and
// 65 and segment lengths on both sides of a round (256), a workgroup's share (2048) and several workgroups per segment.  The words
// after each segment (the pitch is longer than the segment) and the guard words around the buffers must come back untouched.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/sliced_sort_check tests/native/sliced_sort_check.hip
#include "../../fadtk_amd/csrc/sliced_sort.h"

#include "sliced_keys.h"

using namespace fad;

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
    expect_none(bad, "keys x segments", kind, n, segs);
    return 0;
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    // the map itself: order and round trip on the host
    {
        const float v[] = {-INFINITY, -FLT_MAX, -1.f, -FLT_MIN, -1e-45f, -0.f, 0.f, 1e-45f, FLT_MIN, 1.f, FLT_MAX, INFINITY};
        for (int i = 0; i < 12; ++i) {
            const uint32_t k = ssort::key_image(bits_of(v[i]));
            expect(ssort::key_bits(k) == bits_of(v[i]) && (!i || ssort::key_image(bits_of(v[i - 1])) < k), "the map's order and round trip");
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
    return report();
}
