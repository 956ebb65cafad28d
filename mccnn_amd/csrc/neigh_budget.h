// The edge budget of a neighbour search (mccnn_find_neighbors_count_budget): the scalar half of the selection that turns
// the uncapped row lengths k_i into the cap K*. Plain integer C++ with no other header of the library behind it, so that
// the host compiles the very routine the selection kernels run (tools/budget_select_check.cpp).
//
// S(K) = sum_i min(k_i, K) is non-decreasing in K, so K* + 1 is the FIRST value v with S(v) > B (none: the list fits).
// v is found by a radix descent over the 31 bits of k, MCCNN_NB_LEVELS levels from the top: a level splits the current
// range [lo, lo + nb * W) into nb buckets of W = 1 << shift values and holds, per bucket, the rows whose k falls in it and
// the sum of their k. With
//     lowSum = sum of k over the rows below the range,   rowsGE = rows at or above its start,
// the value at the END of bucket b is exact without looking inside it:
//     S(hi_b - 1) = lowSum + (sum of k over buckets 0..b) + (hi_b - 1) * (rows at or above hi_b),   hi_b = lo + (b + 1) W
// The first bucket whose end exceeds B holds v and becomes the range of the next level; at the last level W = 1 and the
// bucket IS v. Every sum is below 2^62 for m, k < 2^31: unsigned 64-bit words never wrap.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MCCNN_BUDGET_FN __host__ __device__ __forceinline__
#else
#define MCCNN_BUDGET_FN inline
#endif

namespace mccnn {

#define MCCNN_NB_LEVELS 3
#define MCCNN_NB_BUCKETS 2048   // buckets of the widest level (LDS: 4 + 8 bytes each)
// bits 30..20 | 19..10 | 9..0
MCCNN_BUDGET_FN int budget_level_shift(int level) { return level == 0 ? 20 : (level == 1 ? 10 : 0); }
MCCNN_BUDGET_FN int budget_level_buckets(int level) { return level == 0 ? 2048 : 1024; }

struct BudgetRange {
    uint64_t lowSum;   // sum of k over the rows with k < lo
    uint32_t rowsGE;   // rows with k >= lo
    uint32_t lo;       // first value of the range
};

// The bucket of [r.lo, r.lo + nb << shift) in which S crosses `budget`, or -1 when S stays at or below it over the whole
// range (then no row lies above the range either: the loop ends where the rows do). On a hit `r` becomes that bucket's range.
MCCNN_BUDGET_FN int budget_pick(const uint32_t* rows, const uint64_t* sums, int nb, int shift, BudgetRange& r, uint64_t budget) {
    uint64_t cum = 0;
    uint32_t ge = r.rowsGE;
    for (int b = 0; b < nb; ++b) {
        const uint32_t c = rows[b];
        const uint64_t s = sums[b];
        const uint64_t hi = (uint64_t)r.lo + ((uint64_t)(b + 1) << shift);
        const uint32_t above = ge - c;
        if (r.lowSum + cum + s + (hi - 1ull) * (uint64_t)above > budget) {
            r.lowSum += cum;
            r.rowsGE = ge;
            r.lo = (uint32_t)(hi - (1ull << shift));
            return b;
        }
        if (above == 0) return -1;   // S is constant from here on
        cum += s;
        ge = above;
    }
    return -1;
}

// K* from the first value v with S(v) > B (found == 0: there is none), the user's cap Ku (0 = none) and the longest row
MCCNN_BUDGET_FN int budget_cap(int found, uint32_t v, int Ku, int kmaxRows) {
    int64_t K = found ? (int64_t)v - 1 : (int64_t)0x7fffffff;
    const int64_t kmax = kmaxRows > 1 ? kmaxRows : 1;
    if (K > kmax) K = kmax;
    if (Ku > 0 && K > Ku) K = Ku;
    return K < 1 ? 1 : (int)K;   // the floor: every non-empty row keeps one hit
}

}  // namespace mccnn
