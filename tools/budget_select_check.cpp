// mccnn_amd/csrc/neigh_budget.h compiled for the host: the selection's scalar half against brute force.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/budget_select_check.cpp -o budget_select_check
//   ./budget_select_check        random row-length vectors (short rows, rows above 2^16 and 2^30, empty lists, sums beyond 2^32)
//                                 at budgets below, on and above every crossing; exit status 0 and "ok <cases>" when all agree
// The histograms are built here as the kernels build them (budget_hist in neigh_budget.hip): rows whose k lies in the level's
// range add (1, k) to bucket (k - lo) >> shift.
#include "neigh_budget.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace mccnn;

// the device's path: MCCNN_NB_LEVELS histograms, budget_pick on each, budget_cap at the end
static int select_levels(const std::vector<uint32_t>& k, uint64_t B, int Ku) {
    BudgetRange r{0ull, (uint32_t)k.size(), 0u};
    uint32_t kmax = 0;
    for (uint32_t x : k) kmax = std::max(kmax, x);
    for (int level = 0; level < MCCNN_NB_LEVELS; ++level) {
        const int nb = budget_level_buckets(level), shift = budget_level_shift(level);
        std::vector<uint32_t> rows(nb, 0u);
        std::vector<uint64_t> sums(nb, 0ull);
        for (uint32_t x : k) {
            if (x < r.lo) continue;
            const uint32_t d = (x - r.lo) >> shift;
            if (d < (uint32_t)nb) { rows[d] += 1u; sums[d] += x; }
        }
        const int b = budget_pick(rows.data(), sums.data(), nb, shift, r, B);
        if (b < 0) {
            if (level == 0) return budget_cap(0, 0u, Ku, (int)kmax);
            std::printf("level %d found no bucket\n", level);
            std::exit(2);
        }
        if (level == MCCNN_NB_LEVELS - 1) return budget_cap(1, r.lo, Ku, (int)kmax);
    }
    return -1;
}

static uint64_t S(const std::vector<uint32_t>& k, uint64_t K) {
    uint64_t s = 0;
    for (uint32_t x : k) s += std::min<uint64_t>(x, K);
    return s;
}

// the definition: the largest K in [1, min(Ku, kmax)] with S(K) <= B, by bisection (S is monotone), 1 on the floor
static int select_brute(const std::vector<uint32_t>& k, uint64_t B, int Ku) {
    uint64_t top = 1;
    for (uint32_t x : k) top = std::max<uint64_t>(top, x);
    if (Ku > 0) top = std::min<uint64_t>(top, (uint64_t)Ku);
    if (S(k, 1) > B) return 1;
    uint64_t lo = 1, hi = top;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (S(k, mid) <= B) lo = mid; else hi = mid - 1;
    }
    return (int)lo;
}

int main() {
    std::mt19937_64 rng(12345);
    long cases = 0, beyond32 = 0, onBoundary = 0;
    auto check = [&](const std::vector<uint32_t>& k, uint64_t B, int Ku) {
        if (B == 0 || B > 0x7fffffffull) return;   // the entry takes 0 < B < 2^31
        const int a = select_levels(k, B, Ku), b = select_brute(k, B, Ku);
        if (a != b) {
            std::printf("MISMATCH rows %zu B %llu Ku %d: levels %d, brute force %d\n", k.size(), (unsigned long long)B, Ku, a, b);
            std::exit(1);
        }
        if (S(k, 0x7fffffffull) > 0xffffffffull) ++beyond32;
        if (S(k, (uint64_t)a) == B) ++onBoundary;
        ++cases;
    };
    const uint32_t tops[] = {1u, 7u, 300u, 1023u, 1024u, 1025u, 70000u, 1u << 20, (1u << 20) + 3u, 0x7fffffffu};
    for (int round = 0; round < 400; ++round) {
        const uint32_t top = tops[round % 10];
        const size_t m = (size_t)(rng() % (round % 7 == 0 ? 3 : 600));
        std::vector<uint32_t> k(m);
        for (auto& x : k) x = (rng() % 5 == 0) ? 0u : (uint32_t)(rng() % ((uint64_t)top + 1ull));
        if (m > 2 && round % 3 == 0) k[0] = k[1] = top;   // ties at the top
        const uint64_t E = S(k, 0x7fffffffull);
        // budgets: the crossings S(K) - 1, S(K), S(K) + 1 of a few K, the ends, random ones
        std::vector<uint64_t> budgets = {1, 2, m ? m - 1 : 1, m, m + 1, E ? E - 1 : 1, E, E + 1, 0x7fffffffull};
        for (int t = 0; t < 6; ++t) {
            const uint64_t K = 1 + rng() % ((uint64_t)top + 1ull);
            const uint64_t s = S(k, K);
            budgets.push_back(s ? s - 1 : 1);
            budgets.push_back(s);
            budgets.push_back(s + 1);
            budgets.push_back(1 + rng() % 0x7fffffffull);
        }
        for (uint64_t B : budgets) {
            check(k, B, 0);
            check(k, B, 1 + (int)(rng() % ((uint64_t)top + 1ull)));
        }
    }
    // a list whose uncapped total is far beyond 2^32 and 2^31 rows' worth of sums: 40 000 rows of 2^31 - 1 hits
    {
        std::vector<uint32_t> k(40000, 0x7fffffffu);
        k[5] = 3u; k[6] = 0u;
        for (uint64_t B : {1ull, 39999ull, 40000ull, 40001ull, 79997ull, 79998ull, 0x7fffffffull, 0x7ffffffeull}) check(k, B, 0), check(k, B, 5);
    }
    if (beyond32 == 0 || onBoundary == 0) {
        std::printf("the cases miss a regime: beyond 2^32 %ld, S(K*) = B %ld\n", beyond32, onBoundary);
        return 3;
    }
    std::printf("ok %ld (uncapped totals beyond 2^32: %ld, S(K*) = B: %ld)\n", cases, beyond32, onBoundary);
    return 0;
}
