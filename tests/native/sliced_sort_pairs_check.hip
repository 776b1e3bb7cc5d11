// The key-index segmented sort of fadtk_amd/csrc/sliced_sort_pairs.h on its own, below fad_sliced_shares: this file includes that
// header (which includes sliced_sort.h) and nothing else of the library.  Every segment's keys AND indices are compared bit for bit with
// std::stable_sort of (mapped uint32 key, position) by key -- so equal keys must carry ascending positions -- over the key families
// of sliced_keys.h (kinds 0 .. 10): random bits, denormals and both zeros, a few special values with many ties (+-0, +-FLT_MAX, +-FLT_MIN,
// +-inf), keys that share three of their four bytes (one digit alone decides, per byte position), all keys equal (the indices must come
// out as the identity), sorted, reversed and two-valued input -- at 1, 3 and 65 segments of 1, 255, 256, 257, 2047, 2048, 2049, 4100
// and 10 007 keys.  The index buffer goes in filled with the guard word: the sort must not need it initialised.  The words after each
// segment (the pitch is longer than the segment) and the guard words around all four buffers and behind the counts and the bases must
// come back untouched.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tests/native/sliced_sort_pairs_check tests/native/sliced_sort_pairs_check.hip
#include "../../fadtk_amd/csrc/sliced_sort_pairs.h"

#include "sliced_keys.h"

#include <utility>

using namespace fad;

static int run(int kind, int64_t n, int64_t segs) {
    const int64_t pitch = n + 5, guard = 64;
    const int64_t total = segs * pitch + 2 * guard;
    std::mt19937 rng((uint32_t)(kind * 1000003 + n * 131 + segs));
    std::vector<uint32_t> host((size_t)total, kGuard);
    for (int64_t s = 0; s < segs; ++s)
        for (int64_t i = 0; i < n; ++i) host[(size_t)(guard + s * pitch + i)] = make_key(kind, s, i, n, rng);
    const int64_t nc = ssort::counts_elems(n, segs), nb = ssort::bases_elems(segs);
    std::vector<uint32_t> fill((size_t)std::max<int64_t>(total, std::max(nc, nb) + guard), kGuard);
    uint32_t* dev[4];                                      // keys, tmp, idx, idx_tmp
    uint32_t *counts, *bases;
    for (int b = 0; b < 4; ++b) {
        CK(hipMalloc(&dev[b], (size_t)total * 4));
        CK(hipMemcpy(dev[b], b == 0 ? host.data() : fill.data(), (size_t)total * 4, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&counts, (size_t)(nc + guard) * 4));
    CK(hipMalloc(&bases, (size_t)(nb + guard) * 4));
    CK(hipMemcpy(counts, fill.data(), (size_t)(nc + guard) * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(bases, fill.data(), (size_t)(nb + guard) * 4, hipMemcpyHostToDevice));
    CK(ssort::sort_segment_pairs(reinterpret_cast<float*>(dev[0] + guard), reinterpret_cast<float*>(dev[1] + guard), dev[2] + guard,
                                 dev[3] + guard, pitch, n, segs, counts, bases, nullptr));
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> back[4];
    for (int b = 0; b < 4; ++b) {
        back[b].resize((size_t)total);
        CK(hipMemcpy(back[b].data(), dev[b], (size_t)total * 4, hipMemcpyDeviceToHost));
        CK(hipFree(dev[b]));
    }
    std::vector<uint32_t> cg((size_t)guard), bg((size_t)guard);
    CK(hipMemcpy(cg.data(), counts + nc, (size_t)guard * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(bg.data(), bases + nb, (size_t)guard * 4, hipMemcpyDeviceToHost));
    CK(hipFree(counts)); CK(hipFree(bases));

    int bad = 0;
    std::vector<std::pair<uint32_t, uint32_t>> want((size_t)n);
    for (int64_t s = 0; s < segs; ++s) {
        for (int64_t i = 0; i < n; ++i) want[(size_t)i] = {ssort::key_image(host[(size_t)(guard + s * pitch + i)]), (uint32_t)i};
        std::stable_sort(want.begin(), want.end(), [](const auto& u, const auto& v) { return u.first < v.first; });
        for (int64_t i = 0; i < n; ++i) {
            bad += back[0][(size_t)(guard + s * pitch + i)] != ssort::key_bits(want[(size_t)i].first);
            bad += back[2][(size_t)(guard + s * pitch + i)] != want[(size_t)i].second;
            if (kind == 7) bad += back[2][(size_t)(guard + s * pitch + i)] != (uint32_t)i;           // all equal: the identity
        }
        for (int64_t i = n; i < pitch; ++i)
            for (int b = 0; b < 4; ++b) bad += back[b][(size_t)(guard + s * pitch + i)] != kGuard;
    }
    for (int64_t i = 0; i < guard; ++i) {
        for (int b = 0; b < 4; ++b) bad += back[b][(size_t)i] != kGuard || back[b][(size_t)(total - 1 - i)] != kGuard;
        bad += cg[(size_t)i] != kGuard || bg[(size_t)i] != kGuard;
    }
    expect_none(bad, "keys x segments", kind, n, segs);
    return 0;
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    const int64_t lengths[] = {1, 255, 256, 257, 2047, 2048, 2049, 4100, 10007};
    const int64_t counts[] = {1, 3, 65};
    for (int kind = 0; kind < 11; ++kind)
        for (int64_t n : lengths)
            for (int64_t segs : counts) {
                const int rc = run(kind, n, segs);
                if (rc) return rc;
            }
    return report();
}
