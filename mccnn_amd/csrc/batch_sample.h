// The counter-based draws of the device batcher (mccnn_batch_sample, batch_sample.hip): which points of a model a slot of a
// training batch keeps. Plain integer C++ on top of neigh_sample.h's mix, so that the host compiles the very functions the
// kernel runs (tools/batch_sample_check.cpp). All arithmetic is uint32 modulo 2^32 unless a 64-bit product is spelled out.
//
// Per-point draw of pass t (protocols split, gradient, lambert), i = the point's index inside its model:
//     a_t = mix(seed + 0x9E3779B9 * (t + 1))          batch_pass_hash
//     d   = mix(a_t + i) >> 8                          batch_draw24, 24 bits
//     u   = d * 2^-24                                  exact in f32, in [0, 1); the point is accepted when u < prob
// Uniform protocol, row t of K over the first n points of the model, a = a_0:
//     n >= K: lo_t = floor(t * n / K), len_t = lo_{t+1} - lo_t >= 1, index = lo_t + ((mix(a + t) * len_t) >> 32)
//             -- the strata of sample_slot: K distinct ascending indices, one per stratum
//     n <  K: index = (mix(a + t) * n) >> 32           with replacement, as the host loader draws there
#pragma once
#include "neigh_sample.h"

#define MCCNN_BATCH_MAX_PASSES 64   // passes over a model before a slot gives up (status MCCNN_BATCH_PASS_BOUND)
#define MCCNN_BATCH_CHUNK 1024      // points a workgroup handles per iteration (= its threads)

namespace mccnn {

MCCNN_SAMPLE_FN uint32_t batch_pass_hash(uint32_t seed, int pass) {
    return sample_mix(seed + 0x9E3779B9u * ((uint32_t)pass + 1u));
}

MCCNN_SAMPLE_FN uint32_t batch_draw24(uint32_t a, uint32_t i) { return sample_mix(a + i) >> 8; }

// n > 0, K > 0, t < K
MCCNN_SAMPLE_FN uint32_t batch_uniform_index(uint32_t t, uint32_t n, uint32_t K, uint32_t a) {
    const uint64_t h = (uint64_t)sample_mix(a + t);
    if (n < K) return (uint32_t)((h * (uint64_t)n) >> 32);
    const uint64_t lo = (uint64_t)t * (uint64_t)n / (uint64_t)K, hi = ((uint64_t)t + 1ull) * (uint64_t)n / (uint64_t)K;
    return (uint32_t)(lo + ((h * (hi - lo)) >> 32));
}

}  // namespace mccnn
