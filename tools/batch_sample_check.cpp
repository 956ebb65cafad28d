// Host check of the device batcher's draws (mccnn_amd/csrc/batch_sample.h), no GPU and no Python:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/batch_sample_check.cpp -o batch_sample_check
//   ./batch_sample_check          the hash and the stratum rule against a restatement with 64-bit integers only, and the
//                                 properties the batcher relies on: K distinct ascending indices, one per stratum, every
//                                 index below n (also with n < K), draws of 24 bits whose f32 value is exact and below 1;
//                                 exit status 0 = everything agrees
//   ./batch_sample_check --dump   one line "U n K seed: indices" per uniform case and "D seed pass: first 8 draws" per
//                                 seed and pass, for a comparison with another statement of the rule
//                                 (tests/test_device_batcher_cpu.py reads it against NumPy)
#include "batch_sample.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

static uint32_t mix_ref(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

static long check_uniform(uint32_t n, uint32_t K, uint32_t seed, bool dump) {
    const uint32_t a = mccnn::batch_pass_hash(seed, 0);
    long bad = a != mix_ref(seed + 0x9E3779B9u);
    uint64_t prev = 0;
    if (dump) std::printf("U %" PRIu32 " %" PRIu32 " %" PRIu32 ":", n, K, seed);
    for (uint32_t t = 0; t < K; ++t) {
        const uint64_t idx = mccnn::batch_uniform_index(t, n, K, a);
        const uint64_t h = mix_ref(a + t);
        if (n < K) {
            if (idx != ((h * (uint64_t)n) >> 32) || idx >= n) ++bad;
        } else {
            const uint64_t lo = (uint64_t)t * n / K, hi = ((uint64_t)t + 1) * n / K;
            if (idx != lo + ((h * (hi - lo)) >> 32) || idx < lo || idx >= hi || hi > n || (t > 0 && idx <= prev)) ++bad;
            prev = idx;
        }
        if (dump) std::printf(" %" PRIu64, idx);
    }
    if (dump) std::printf("\n");
    return bad;
}

static long check_draws(uint32_t seed, int pass, bool dump) {
    const uint32_t a = mccnn::batch_pass_hash(seed, pass);
    long bad = a != mix_ref(seed + 0x9E3779B9u * ((uint32_t)pass + 1u));
    if (dump) std::printf("D %" PRIu32 " %d:", seed, pass);
    const uint32_t probes[] = {0u, 1u, 2u, 3u, 1023u, 1024u, 99999u, 0x7FFFFFFEu};
    for (uint32_t i : probes) {
        const uint32_t d = mccnn::batch_draw24(a, i);
        const float u = (float)d * 5.9604644775390625e-8f;
        if (d != (mix_ref(a + i) >> 8) || d >= (1u << 24) || !(u < 1.0f) || (double)u * 16777216.0 != (double)d) ++bad;
        if (dump) std::printf(" %" PRIu32, d);
    }
    if (dump) std::printf("\n");
    return bad;
}

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !std::strcmp(argv[1], "--dump");
    const uint32_t seeds[] = {0u, 1u, 12345u, 0xFFFFFFFFu};
    const uint32_t shapes[][2] = {{1, 1}, {7, 7}, {8, 7}, {1000, 64}, {1023, 1024}, {50, 1024}, {10000, 1024}, {2049, 1023}};
    long bad = 0, cases = 0;
    for (uint32_t s : seeds) {
        for (const auto& nk : shapes) {
            bad += check_uniform(nk[0], nk[1], s, dump);
            ++cases;
        }
        for (int pass : {0, 1, 63}) {
            bad += check_draws(s, pass, dump);
            ++cases;
        }
    }
    // products beyond 2^32: t * n with n = 2^31 - 1 rows (not dumped)
    bad += check_uniform(2147483647u, 100003u, 7u, false);
    ++cases;
    if (!dump) std::printf("batch_sample: %ld cases checked, %ld disagreements\n", cases, bad);
    return bad ? 1 : 0;
}
