// Host check of the dense glue over a concatenation (mccnn_amd/csrc/bn_cat.h: bn_cat_fill, bn_cat_at, bn_cat_widths_by4 and the
// plan bn_plan), no GPU and no Python:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/bn_cat_check.cpp -o bn_cat_check
//   ./bn_cat_check      exit status 0 = everything agrees
// For every tuple of 1 .. 4 widths in 1 .. 9, and the tuples of 5 .. 8 widths over {1, 4, 5}, with the pointers taken as
// aligned (vec = 4 iff every width is a multiple of 4) and as not aligned (vec = 1):
//   - the prefixes of bn_cat_fill and its C against a plain running sum;
//   - bn_cat_at of every column against a plain loop over the segments: segment, width and column inside it;
//   - the plan is the contiguous op's: walking the grid (tiles x 2^tw_log units of vec columns) as bn_coord does, every
//     column of [0, C) is owned by exactly one thread, and all vec columns of a thread lie in one segment, in a row of
//     it that is vec * 4 bytes aligned when the segment's pointer is;
//   - slab rule: bn_plan's slab rows and slabs cover [0, n) for a few n around the thresholds.
#include "bn_cat.h"

#include <cstdio>
#include <vector>

using namespace mccnn;

static long g_bad = 0, g_tuples = 0;

static void check_tuple(const int* cs, int nseg, bool aligned) {
    ++g_tuples;
    BnCat t = {};
    const long long C = bn_cat_fill(t, cs, nseg);
    long long sum = 0;
    for (int s = 0; s < nseg; ++s) {
        if (t.col0[s] != sum || t.c[s] != cs[s]) ++g_bad;
        sum += cs[s];
    }
    if (C != sum) ++g_bad;
    for (int s = nseg; s <= kBnCatMax; ++s)
        if (t.col0[s] != sum) ++g_bad;
    static float rows[kBnCatMax][4];   // stand-ins: only their addresses are compared
    for (int s = 0; s < kBnCatMax; ++s) { t.x[s] = rows[s < nseg ? s : 0]; t.dx[s] = rows[s < nseg ? s : 0] + 1; }
    // the lookup against a plain loop
    for (int col = 0; col < (int)C; ++col) {
        int seg = 0, first = 0;
        while (col >= first + cs[seg]) { first += cs[seg]; ++seg; }
        const BnCatAt at = bn_cat_at(t, col);
        if (at.seg != seg || at.ld != cs[seg] || at.col != col - first || at.x != rows[seg] || at.dx != rows[seg] + 1) ++g_bad;
    }
    // the plan: the contiguous op's at width C
    const bool wide = aligned && bn_cat_widths_by4(cs, nseg);
    const BnPlan p = bn_plan(300, (int)C, wide, 0);
    const BnPlan q = bn_plan(300, (int)C, aligned, 0);   // what the contiguous op takes on the concatenated tensor
    if (p.vec != (wide ? 4 : 1)) ++g_bad;
    if ((C % 4 != 0 || wide) != (p.vec == q.vec && p.tw_log == q.tw_log && p.tiles == q.tiles) && aligned) ++g_bad;
    std::vector<int> owner((size_t)C, 0);
    for (int tile = 0; tile < p.tiles; ++tile)
        for (int cx = 0; cx < (1 << p.tw_log); ++cx) {
            const long long col = ((long long)tile * (1 << p.tw_log) + cx) * p.vec;
            if (col >= C) continue;
            const BnCatAt at = bn_cat_at(t, (int)col);
            for (int k = 0; k < p.vec; ++k) {
                if (col + k >= C) { ++g_bad; continue; }
                ++owner[(size_t)(col + k)];
                const BnCatAt ak = bn_cat_at(t, (int)col + k);
                if (ak.seg != at.seg || ak.col != at.col + k) ++g_bad;
            }
            if (at.col % p.vec != 0 || at.ld % p.vec != 0) ++g_bad;   // r * c_s + col stays on vec * 4 bytes
        }
    for (int o : owner)
        if (o != 1) ++g_bad;
    if ((1 << p.tw_log) * p.vec > 32 || p.tiles < 1) ++g_bad;
}

static void tuples(int* cs, int at, int nseg, const int* widths, int nwidths) {
    if (at == nseg) {
        check_tuple(cs, nseg, true);
        check_tuple(cs, nseg, false);
        return;
    }
    for (int i = 0; i < nwidths; ++i) { cs[at] = widths[i]; tuples(cs, at + 1, nseg, widths, nwidths); }
}

int main() {
    int cs[kBnCatMax];
    const int small[] = {1, 2, 3, 4, 5, 6, 7, 8, 9}, few[] = {1, 4, 5};
    for (int nseg = 1; nseg <= 4; ++nseg) tuples(cs, 0, nseg, small, 9);
    for (int nseg = 5; nseg <= kBnCatMax; ++nseg) tuples(cs, 0, nseg, few, 3);
    // wider segments: boundaries on and inside tiles of 32 columns
    const int wide_cases[][4] = {{32, 4, 28, 0}, {16, 16, 1, 0}, {3, 5, 122, 0}, {64, 64, 0, 0}, {128, 36, 60, 4}};
    for (const auto& w : wide_cases) {
        int n = 0;
        while (n < 4 && w[n]) ++n;
        check_tuple(w, n, true);
        check_tuple(w, n, false);
    }
    // the slab rule
    const int ns[] = {1, 2, 255, 256, 257, 300, 8192, 8193, 20000, 1 << 20};
    for (int n : ns) {
        const BnPlan p = bn_plan(n, 8, true, 0);
        if (p.slab_rows < 1 || (long long)p.slabs * p.slab_rows < n || (long long)(p.slabs - 1) * p.slab_rows >= n) ++g_bad;
        if (n <= kBnSmallRows ? p.slabs != 1 : (p.slabs > kBnMaxSlabs || p.slab_rows < kBnSlabRows)) ++g_bad;
    }
    std::printf("bn_cat: %ld tuples checked, %ld disagreements\n", g_tuples, g_bad);
    return g_bad ? 1 : 0;
}
