// The dense glue over a column-wise concatenation (mccnn_bn_act_cat_fwd / _bwd, bn_act.hip): what the host decides of a call
// -- the plan of the op at width C = sum c_s, and whether a thread moves 4 columns or 1 -- and where a thread finds the rows
// of its columns. Plain C++ without a device call, so that the host compiles the very code the kernels run
// (tools/bn_cat_check.cpp).
//
// The plan is the contiguous op's at (n, C): the grid, tw_log, the slabs and the thread -> global column mapping do not know
// of the segments. 4 columns per thread iff every c_s % 4 == 0 and every row pointer allows it; a thread's columns then lie
// inside one segment, because every segment starts at a multiple of 4. A thread walks the at most 8 column prefixes once
// (an unrolled compare and select over kernel arguments, uniform loads) and from then on addresses
// x_s + r * c_s + (col - col0_s) where the contiguous op addresses x + r * C + col.
//
// A segment is f32 or bf16 storage (mccnn_bn_act_cat_fwd_rows / _bwd_rows; tools/bn_cat_rows_check.cpp): the table carries a
// bit per segment, the lookup hands the thread its segment's, and the plan stays the f32 one at (n, C) whatever the types.
// 4 columns per thread then ask a bf16 segment's rows for 8-byte alignment where they ask an f32 one's for 16
// (bn_cat_rows_wide).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MCCNN_CAT_FN __host__ __device__ __forceinline__
#else
#define MCCNN_CAT_FN inline
#endif

namespace mccnn {

constexpr int kBnThreads = 256;
constexpr int kBnTileCols = 64;     // most columns of a workgroup: 128 bytes of a row of x (32 f32, 64 bf16)
constexpr int kBnSmallRows = 256;   // up to here: the one-launch form
constexpr int kBnSlabRows = 128;    // rows of a slab ...
constexpr int kBnMaxSlabs = 64;     // ... until there would be more slabs than this: then the slabs grow

struct BnPlan {
    int vec, tw_log, tiles, slab_rows, slabs;
};
inline int bn_cdiv(int a, int b) { return (a + b - 1) / b; }
inline int bn_slab_rows_of(int n) {
    if (n <= kBnSmallRows) return n;
    if (bn_cdiv(n, kBnSlabRows) <= kBnMaxSlabs) return kBnSlabRows;
    return bn_cdiv(bn_cdiv(n, kBnMaxSlabs), 32) * 32;
}
// aligned: every row pointer allows the wide form (bn_rows_aligned); x_bf16: the thread layout follows x's type
inline BnPlan bn_plan(int n, int c, bool aligned, int x_bf16 = 0) {
    BnPlan p;
    if (x_bf16) p.vec = (c % 8 == 0 && aligned) ? 8 : 2;
    else p.vec = (c % 4 == 0 && aligned) ? 4 : 1;
    const int units = c / p.vec, most = (x_bf16 ? 64 : 32) / p.vec;
    p.tw_log = 0;
    while ((1 << p.tw_log) < most && (1 << p.tw_log) < units) ++p.tw_log;
    p.tiles = bn_cdiv(units, 1 << p.tw_log);
    p.slab_rows = bn_slab_rows_of(n);
    p.slabs = bn_cdiv(n, p.slab_rows);
    return p;
}

constexpr int kBnCatMax = 8;   // segments of a call

// The segment table of a call, by value in the kernel arguments. col0[s]: the first global column of segment s; from
// s = nseg on col0 is C (no column reaches it) and x, dx, c repeat segment 0's. bf16: bit s is set where x_s (and dx_s) is
// bfloat16 storage; only the typed-segment instantiations look at it.
struct BnCat {
    const void* x[kBnCatMax];
    void* dx[kBnCatMax];    // backward: NULL where no gradient is wanted; x_s's type
    int c[kBnCatMax];
    int col0[kBnCatMax + 1];
    unsigned bf16;
};

// the widths of a call: every segment a multiple of 4 columns wide (with aligned pointers: 4 columns per thread)
inline bool bn_cat_widths_by4(const int* cs, int nseg) {
    for (int s = 0; s < nseg; ++s)
        if (cs[s] % 4 != 0) return false;
    return true;
}

// Columns per thread of a call over typed segments (xs_bf16: NULL, or per segment 1 for bf16 rows; dxs: NULL, or per segment
// where its gradient goes, NULL: not wanted): 4 iff every width is a multiple of 4, every f32 x_s and wanted f32 dx_s is on
// 16 bytes and every bf16 x_s and wanted bf16 dx_s on 8 -- what a thread's 4 elements of a row take in either type. (y, dy
// and the workspace come on top: the rule of the _rows entries, bn_setup in bn_act.hip.) Otherwise 1; a bf16 element then
// moves as one 16-bit access.
inline bool bn_cat_rows_wide(const void* const* xs, const int* xs_bf16, const int* cs, int nseg, const void* const* dxs) {
    if (!bn_cat_widths_by4(cs, nseg)) return false;
    for (int s = 0; s < nseg; ++s) {
        const uintptr_t mask = (xs_bf16 && xs_bf16[s]) ? 7u : 15u;
        if ((uintptr_t)xs[s] & mask) return false;
        if (dxs && ((uintptr_t)dxs[s] & mask)) return false;   // (NULL: not wanted, and on every boundary)
    }
    return true;
}

// the types of the nseg segments into the table (xs_bf16: NULL -- all f32 -- or per segment 0 / 1); -> some segment is bf16
inline bool bn_cat_set_types(BnCat& t, const int* xs_bf16, int nseg) {
    t.bf16 = 0;
    for (int s = 0; xs_bf16 && s < nseg; ++s)
        if (xs_bf16[s]) t.bf16 |= 1u << s;
    return t.bf16 != 0;
}

// fills c and col0 from the nseg widths (1 <= nseg <= kBnCatMax, every width >= 1); -> C, as 64 bits
inline long long bn_cat_fill(BnCat& t, const int* cs, int nseg) {
    long long at = 0;
    for (int s = 0; s < kBnCatMax; ++s) {
        t.col0[s] = (int)(at > 0x7fffffffll ? 0x7fffffffll : at);
        t.c[s] = s < nseg ? cs[s] : cs[0];
        if (s < nseg) at += cs[s];
    }
    t.col0[kBnCatMax] = (int)(at > 0x7fffffffll ? 0x7fffffffll : at);
    return at;
}

// where global column col (0 <= col < C) is: its segment, that segment's rows and the column inside them
struct BnCatAt {
    int seg, ld, col;
    const void* x;
    void* dx;
    bool bf16;   // the segment's rows are bf16 storage
};
MCCNN_CAT_FN BnCatAt bn_cat_at(const BnCat& t, int col) {
    BnCatAt at;
    at.seg = 0; at.ld = t.c[0]; at.x = t.x[0]; at.dx = t.dx[0];
    int first = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 1; s < kBnCatMax; ++s) {   // (every entry is read, then selected: values, never an address into the table)
        const int c0 = t.col0[s], ld = t.c[s];
        const void* const x = t.x[s];
        void* const dx = t.dx[s];
        const bool in = col >= c0;
        at.seg = in ? s : at.seg; at.ld = in ? ld : at.ld; at.x = in ? x : at.x; at.dx = in ? dx : at.dx; first = in ? c0 : first;
    }
    at.col = col - first;
    at.bf16 = (t.bf16 >> at.seg) & 1u;
    return at;
}

}  // namespace mccnn
