// Host check of the fused glue's dropout predicate (mccnn_amd/csrc/bn_drop.h: bn_drop_keep), no GPU and no Python:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/bn_drop_check.cpp -o bn_drop_check
//   ./bn_drop_check          the predicate against the rule restated here with 64-bit integers only, the thresholds of a few
//                            keep probabilities, and the kept share of a large block; exit status 0 = all agree
//   ./bn_drop_check --dump   one line "seed i j T keep" per tuple of the same grid, for a comparison with another statement
//                            of the rule (tests/test_bn_act_cpu.py reads it against NumPy)
// Grid: seeds 0, 1, 12345, 2^32-1 x rows 0, 1, 255, 1019, 2^31-2 x columns 0, 1, 31, 130, 2^31-1 x T in {1, 2^31, floor(0.7 * 2^32),
// 2^32 - 1, 2^32}.
#include "bn_drop.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>

static uint32_t mix_ref(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

static bool keep_ref(uint32_t seed, uint32_t i, uint32_t j, uint64_t T) {
    const uint32_t a = mix_ref(seed + 0x9E3779B9u * (i + 1u));
    return (uint64_t)mix_ref(a + j) < T;
}

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !std::strcmp(argv[1], "--dump");
    const uint32_t seeds[] = {0u, 1u, 12345u, 0xFFFFFFFFu};
    const int rows[] = {0, 1, 255, 1019, 2147483646};
    const uint32_t cols[] = {0u, 1u, 31u, 130u, 2147483647u};
    const uint64_t thr[] = {1ull, 1ull << 31, mccnn::bn_drop_threshold(0.7), 0xFFFFFFFFull, mccnn::kBnDropAll};
    long bad = 0, n = 0;
    for (uint32_t s : seeds)
        for (int i : rows) {
            const uint32_t a = mccnn::bn_drop_row(s, i);
            for (uint32_t j : cols)
                for (uint64_t T : thr) {
                    const bool k = mccnn::bn_drop_keep(a, j, T);
                    if (k != keep_ref(s, (uint32_t)i, j, T)) ++bad;
                    if (T == mccnn::kBnDropAll && !k) ++bad;   // 2^32 keeps everything
                    if (dump) std::printf("%" PRIu32 " %d %" PRIu32 " %" PRIu64 " %d\n", s, i, j, T, k ? 1 : 0);
                    ++n;
                }
        }
    // thresholds: floor(keepProb * 2^32)
    if (mccnn::bn_drop_threshold(1.0) != mccnn::kBnDropAll) ++bad;
    if (mccnn::bn_drop_threshold(0.5) != (1ull << 31)) ++bad;
    if (mccnn::bn_drop_threshold(0.7) != 3006477107ull) ++bad;
    // the kept share of 1000 x 1000 elements at keepProb 0.7: within 5 sigma of it (sigma = sqrt(0.21 / 1e6) = 4.6e-4)
    long kept = 0;
    for (int i = 0; i < 1000; ++i) {
        const uint32_t a = mccnn::bn_drop_row(7u, i);
        for (uint32_t j = 0; j < 1000u; ++j) kept += mccnn::bn_drop_keep(a, j, mccnn::bn_drop_threshold(0.7)) ? 1 : 0;
    }
    if (kept < 697700 || kept > 702300) ++bad;
    if (!dump) std::printf("bn_drop_keep: %ld tuples checked, %ld disagreements, kept %ld of 1000000 at 0.7\n", n, bad, kept);
    return bad ? 1 : 0;
}
