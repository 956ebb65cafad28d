// Host check of the fill pass's sampling predicate (mccnn_amd/csrc/neigh_sample.h: sample_slot), no GPU and no Python:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/sample_slot_check.cpp -o sample_slot_check
//   ./sample_slot_check          the predicate, rank by rank, against the forward rule (strata, hash, offset) restated here
//                                with 64-bit integers only; exit status 0 = all rows agree
//   ./sample_slot_check --dump   one line "K k seed i: kept ranks" per row of the same grid, for a comparison with another
//                                statement of the rule (tests/test_neighbor_sampling_cpu.py reads it against NumPy)
// Grid: K in {1, 16, 64} x k in {K+1, 2K-1, 2K, 59, 1015} (k > K), seeds 0, 1, 12345, 2^32-1, rows 0, 1, 1019, 2^31-2; and
// one row with k * K > 2^32 (the predicate's 64-bit path).
#include "neigh_sample.h"

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

// forward rule: the rank slot t keeps
static uint64_t kept_rank(uint64_t t, uint64_t k, uint64_t K, uint32_t seed, uint32_t i) {
    const uint64_t lo = t * k / K, hi = (t + 1) * k / K;
    const uint32_t a = mix_ref(seed + 0x9E3779B9u * (i + 1u));
    const uint32_t h = mix_ref(a + (uint32_t)t);
    return lo + (((uint64_t)h * (hi - lo)) >> 32);
}

static long check_row(int k, int K, uint32_t seed, int i, bool dump) {
    const uint32_t a = mccnn::sample_row_hash(seed, i);
    std::vector<int> slot((size_t)k);
    for (int r = 0; r < k; ++r) slot[(size_t)r] = mccnn::sample_slot(r, k, K, a);
    long bad = 0;
    uint64_t prev = 0;
    std::vector<char> want((size_t)k, 0);
    for (int t = 0; t < K; ++t) {
        const uint64_t r = kept_rank((uint64_t)t, (uint64_t)k, (uint64_t)K, seed, (uint32_t)i);
        if (r >= (uint64_t)k || (t > 0 && r <= prev) || slot[(size_t)r] != t) { ++bad; continue; }
        want[(size_t)r] = 1;
        prev = r;
    }
    for (int r = 0; r < k; ++r)
        if ((slot[(size_t)r] >= 0) != (want[(size_t)r] != 0)) ++bad;
    if (dump) {
        std::printf("%d %d %" PRIu32 " %d:", K, k, seed, i);
        for (int r = 0; r < k; ++r)
            if (slot[(size_t)r] >= 0) std::printf(" %d", r);
        std::printf("\n");
    }
    return bad;
}

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !std::strcmp(argv[1], "--dump");
    const int caps[] = {1, 16, 64};
    const uint32_t seeds[] = {0u, 1u, 12345u, 0xFFFFFFFFu};
    const int rows[] = {0, 1, 1019, 2147483646};
    long bad = 0, n = 0;
    for (int K : caps) {
        const int ks[] = {K + 1, 2 * K - 1, 2 * K, 59, 1015};
        for (int k : ks) {
            if (k <= K) continue;
            for (uint32_t s : seeds)
                for (int i : rows) {
                    bad += check_row(k, K, s, i, dump);
                    ++n;
                }
        }
    }
    // k * K beyond 2^32: the 64-bit path (the kernel switches on k * (K + 1)); not dumped (2 000 003 ranks)
    bad += check_row(3000017, 2000003, 7u, 5, false);
    ++n;
    if (!dump) std::printf("sample_slot: %ld rows checked, %ld disagreements\n", n, bad);
    return bad ? 1 : 0;
}
