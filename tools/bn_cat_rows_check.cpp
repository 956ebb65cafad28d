// Host check of the typed segments of the dense glue over a concatenation (mccnn_amd/csrc/bn_cat.h: bn_cat_rows_wide,
// bn_cat_set_types and the type bn_cat_at hands out), no GPU and no Python:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/bn_cat_rows_check.cpp -o bn_cat_rows_check
//   ./bn_cat_rows_check      exit status 0 = everything it checks itself agrees
// Over small tuples of widths, type flags, byte offsets of x_s and of dx_s (-1: that gradient is not wanted; a whole call
// without dxs as well) it prints one line per tuple
//   <widths> | <flags> | <x offsets> | <dx offsets, or "none"> | <columns per thread>
// with the answer of bn_cat_rows_wide, for tests/test_bn_cat_rows_cpu.py to hold against the rule as
// tests/bn_cat_rows_ref.py restates it. Itself it checks, per tuple:
//   - bn_cat_at of every column hands out the flag of the column's segment (a plain loop over the segments);
//   - with no flag set (and with xs_bf16 == NULL) the answer is the f32 rule: widths by 4 and every pointer on 16 bytes;
//   - 4 columns per thread: every thread's 4 elements of a row start on 16 bytes (f32) or 8 (bf16) in x_s and in dx_s.
// Pointers are made from an offset into one aligned buffer and never dereferenced.
#include "bn_cat.h"

#include <cstdio>
#include <initializer_list>

using namespace mccnn;

static long g_bad = 0, g_tuples = 0;
alignas(64) static char g_mem[2 * kBnCatMax * 64];

static void check_tuple(const int* cs, const int* bf, const int* xo, const int* dxo, int nseg, bool with_dxs) {
    ++g_tuples;
    const void* xs[kBnCatMax];
    const void* dxs[kBnCatMax];
    for (int s = 0; s < nseg; ++s) {
        xs[s] = g_mem + 64 * s + xo[s];
        dxs[s] = dxo[s] < 0 ? nullptr : g_mem + 64 * (kBnCatMax + s) + dxo[s];
    }
    const bool wide = bn_cat_rows_wide(xs, bf, cs, nseg, with_dxs ? dxs : nullptr);
    for (int s = 0; s < nseg; ++s) std::printf("%s%d", s ? "," : "", cs[s]);
    std::printf(" | ");
    for (int s = 0; s < nseg; ++s) std::printf("%s%d", s ? "," : "", bf[s]);
    std::printf(" | ");
    for (int s = 0; s < nseg; ++s) std::printf("%s%d", s ? "," : "", xo[s]);
    std::printf(" | ");
    if (!with_dxs) std::printf("none");
    else for (int s = 0; s < nseg; ++s) std::printf("%s%d", s ? "," : "", dxo[s]);
    std::printf(" | %d\n", wide ? 4 : 1);

    // the type the lookup hands out
    BnCat t = {};
    const long long C = bn_cat_fill(t, cs, nseg);
    bool any = false;
    for (int s = 0; s < nseg; ++s) any = any || bf[s];
    if (bn_cat_set_types(t, bf, nseg) != any) ++g_bad;
    for (int s = 0; s < kBnCatMax; ++s) { t.x[s] = xs[s < nseg ? s : 0]; t.dx[s] = const_cast<void*>(dxs[s < nseg ? s : 0]); }
    for (int col = 0; col < (int)C; ++col) {
        int seg = 0, first = 0;
        while (col >= first + cs[seg]) { first += cs[seg]; ++seg; }
        const BnCatAt at = bn_cat_at(t, col);
        if (at.seg != seg || at.bf16 != (bf[seg] != 0) || at.x != xs[seg] || at.col != col - first) ++g_bad;
    }
    BnCat u = {};
    if (bn_cat_set_types(u, nullptr, nseg) || u.bf16 != 0) ++g_bad;
    // no flag: the f32 rule
    if (!any) {
        bool f32 = bn_cat_widths_by4(cs, nseg);
        for (int s = 0; s < nseg; ++s) {
            f32 = f32 && ((uintptr_t)xs[s] & 15u) == 0;
            if (with_dxs) f32 = f32 && ((uintptr_t)dxs[s] & 15u) == 0;
        }
        if (f32 != wide || bn_cat_rows_wide(xs, nullptr, cs, nseg, with_dxs ? dxs : nullptr) != wide) ++g_bad;
    }
    // 4 columns per thread: every access of a thread is aligned to its 4 elements
    if (wide)
        for (int col = 0; col < (int)C; col += 4) {
            const BnCatAt at = bn_cat_at(t, col);
            const size_t el = at.bf16 ? 2 : 4;
            for (size_t r = 0; r < 3; ++r) {
                const size_t off = (r * (size_t)at.ld + (size_t)at.col) * el;
                if (((uintptr_t)at.x + off) % (4 * el) != 0) ++g_bad;
                if (with_dxs && at.dx && ((uintptr_t)at.dx + off) % (4 * el) != 0) ++g_bad;
            }
        }
}

struct Sets {
    const int* widths; int nwidths;
    const int* xoffs; int nxoffs;
    const int* dxoffs; int ndxoffs;
};

static void tuples(const Sets& z, int nseg, int at, int* cs, int* bf, int* xo, int* dxo) {
    if (at == nseg) {
        check_tuple(cs, bf, xo, dxo, nseg, true);
        bool first = true;   // (the call without dxs: once per (widths, flags, x offsets), at the first dx tuple)
        for (int s = 0; s < nseg; ++s) first = first && dxo[s] == z.dxoffs[0];
        if (first) check_tuple(cs, bf, xo, dxo, nseg, false);
        return;
    }
    for (int w = 0; w < z.nwidths; ++w)
        for (int b = 0; b < 2; ++b)
            for (int x = 0; x < z.nxoffs; ++x)
                for (int d = 0; d < z.ndxoffs; ++d) {
                    cs[at] = z.widths[w]; bf[at] = b; xo[at] = z.xoffs[x]; dxo[at] = z.dxoffs[d];
                    tuples(z, nseg, at + 1, cs, bf, xo, dxo);
                }
}

int main() {
    int cs[kBnCatMax], bf[kBnCatMax], xo[kBnCatMax], dxo[kBnCatMax];
    // byte offsets: 0 and 16 pass for both types, 8 for bf16 alone, 4 and 2 (a bf16 pointer's least) for neither
    const int w12[] = {1, 3, 4, 8}, x12[] = {0, 2, 4, 8, 16}, d12[] = {-1, 0, 4, 8};
    const Sets small = {w12, 4, x12, 5, d12, 4};
    tuples(small, 1, 0, cs, bf, xo, dxo);
    tuples(small, 2, 0, cs, bf, xo, dxo);
    const int w3[] = {4, 5}, x3[] = {0, 8}, d3[] = {-1, 0, 8};
    const Sets three = {w3, 2, x3, 2, d3, 3};
    tuples(three, 3, 0, cs, bf, xo, dxo);
    // the maximum number of segments, alternating types, one pointer moved at a time
    for (int moved = -1; moved < kBnCatMax; ++moved)
        for (int off : {4, 8}) {
            for (int s = 0; s < kBnCatMax; ++s) { cs[s] = 4; bf[s] = s & 1; xo[s] = s == moved ? off : 0; dxo[s] = 0; }
            check_tuple(cs, bf, xo, dxo, kBnCatMax, true);
        }
    std::printf("bn_cat_rows: %ld tuples checked, %ld disagreements\n", g_tuples, g_bad);
    return g_bad ? 1 : 0;
}
