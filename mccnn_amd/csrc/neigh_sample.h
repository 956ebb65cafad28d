// The stratified sample of a capped neighbour row (mccnn_find_neighbors_fill_sampled): which hit of a row of k > K hits
// slot t keeps. Plain integer C++ with no other header of the library behind it, so that the host compiles the very
// predicate the fill kernel runs (tools/sample_slot_check.cpp).
//
// Strata: lo_t = floor(t * k / K), t = 0 .. K (lo_K = k); stratum t is the canonical ranks [lo_t, lo_{t+1}), len_t >= 1
// because k > K. The canonical cap (cap_slot in neighbors.hip) keeps offset 0 of every stratum; the sample keeps offset
//     off_t = (h * len_t) >> 32,   h = mix(mix(seed + 0x9E3779B9 * (i + 1)) + t)   (uint32, mix = the murmur3 finaliser)
// of stratum t of the row of centre i (the caller's index of the centre, not its visiting position). No state, no
// atomics: the same (inputs, K, seed) give the same bytes; still one hit per stratum, in canonical order.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MCCNN_SAMPLE_FN __host__ __device__ __forceinline__
#else
#define MCCNN_SAMPLE_FN inline
#endif

namespace mccnn {

MCCNN_SAMPLE_FN uint32_t sample_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// the per-row half of the hash: a = mix(seed + 0x9E3779B9 * (i + 1))
MCCNN_SAMPLE_FN uint32_t sample_row_hash(uint32_t seed, int i) {
    return sample_mix(seed + 0x9E3779B9u * ((uint32_t)i + 1u));
}

// Slot of the hit at canonical rank r (0 <= r < k) of a row of k > cap hits, or -1 when the sample drops it: r lies in
// stratum t = floor(((r + 1) * cap - 1) / k) and is kept iff r == lo_t + off_t. `a` = sample_row_hash of the row. k and
// cap are wave-uniform in the kernel: 32-bit division where the products fit (the bound of cap_slot).
MCCNN_SAMPLE_FN int sample_slot(int r, int k, int cap, uint32_t a) {
    if ((uint64_t)k * ((uint64_t)cap + 1ull) <= 0xffffffffull) {
        const uint32_t uk = (uint32_t)k, uc = (uint32_t)cap;
        const uint32_t t = (((uint32_t)r + 1u) * uc - 1u) / uk;      // (r + 1) * cap <= k * cap
        const uint32_t lo = (t * uk) / uc, hi = ((t + 1u) * uk) / uc;  // (t + 1) * k <= cap * k
        const uint32_t off = (uint32_t)(((uint64_t)sample_mix(a + t) * (uint64_t)(hi - lo)) >> 32);
        return (uint32_t)r == lo + off ? (int)t : -1;
    }
    const uint64_t uk = (uint64_t)k, uc = (uint64_t)cap;
    const uint64_t t = (((uint64_t)r + 1ull) * uc - 1ull) / uk;
    const uint64_t lo = (t * uk) / uc, hi = ((t + 1ull) * uk) / uc;
    const uint64_t off = ((uint64_t)sample_mix(a + (uint32_t)t) * (hi - lo)) >> 32;
    return (uint64_t)r == lo + off ? (int)t : -1;
}

}  // namespace mccnn
