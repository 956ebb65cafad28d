// The 27-cell window walk that the neighbour search (neighbors.hip: neigh_window_impl), the per-point density sweep and its
// position gradients (pdf_points.hip: pdf_points_body, pdf_points_bwd_body) share: a wave takes G consecutive members
// (centres / sorted points, lanes 0 .. G-1), groups them by grid cell, builds the 27-entry table of the cell's window in LDS, and walks the window's candidates as one
// flat list in canonical order (table order of find_neighbors.cu:282-291, ascending j inside a cell). The library's
// discrete decisions -- the cell of a point, the canonical order, membership by the unfused d2 < T -- are spelled here and
// in common.h (cell_coord, point_dist2, sqrt_threshold) and nowhere else. Every function is stateless: what it needs comes
// in as arguments, pointers as `__restrict__` PARAMETERS (the qualifier holds for parameters only; the search's fill pass
// loses a wave per SIMD when its loads may alias its stores, see neighbors.hip).
// What sharing may cost a kernel, and what was measured for each: NOTES.md, "One window walk".
#pragma once
#include "common.h"

namespace mccnn {

#ifndef MCCNN_PP_CAP
#define MCCNN_PP_CAP 256   // candidates the density sweeps stage per segment and wave (a multiple of 64)
#endif

__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// ---- 1. a member's context: batch id, position, radius, threshold and grid cell
struct CentreCtx {
    float cx, cy, cz, R, T;  // T: squared-distance threshold equivalent to sqrt(d2) < R (common.h)
    int b, x, y, z;
};

__device__ __forceinline__ CentreCtx centre_ctx(const float* __restrict__ centres, const int* __restrict__ cb,
                                                const float* __restrict__ mn, const float* __restrict__ mx,
                                                int i, int B, int nc, float radius, int scaleInv, float Tabs) {
    CentreCtx c;
    c.b = clamp_batch(cb[i], B);
    c.cx = centres[(size_t)i * 3];
    c.cy = centres[(size_t)i * 3 + 1];
    c.cz = centres[(size_t)i * 3 + 2];
    float ext = max_extent(mn, mx, c.b);
    float cs = ext / (float)nc;
    c.R = scaleInv ? radius * ext : radius;  // find_neighbors.cu:73
    c.T = scaleInv ? sqrt_threshold(c.R) : Tabs;  // an absolute radius has ONE threshold: the host computes it
    c.x = cell_coord(c.cx, mn[c.b * 3], cs, nc);
    c.y = cell_coord(c.cy, mn[c.b * 3 + 1], cs, nc);
    c.z = cell_coord(c.cz, mn[c.b * 3 + 2], cs, nc);
    return c;
}

// the key members are grouped by: the cell's index in the table of all clouds, -1 for a lane without a member
__device__ __forceinline__ int cell_key(const CentreCtx& c, int nc, bool own) {
    return own ? ((c.b * nc + c.x) * nc + c.y) * nc + c.z : -1;
}

// ---- 2. the window of a cell
// The next group of members that share a cell: `lead`, the lowest lane still in `todo`, and the mask of the lanes whose key
// is the lead's; they leave `todo`. Wave-uniform.
__device__ __forceinline__ unsigned window_next_group(unsigned& todo, bool own, int key, int& lead) {
    lead = __builtin_ctz(todo);
    const int wkey = __builtin_amdgcn_readlane(key, lead);
    const unsigned members = (unsigned)(__ballot(own && key == wkey)) & todo;
    todo &= ~members;
    return members;
}

// The 27 cell ranges of the window of cell (wb; wx, wy, wz), all wave-uniform: lane o < 27 owns table entry o
// (find_neighbors.cu:282-291: slab, then u % 3 and u / 3), the wave scan gives the flat offset of every cell in the canonical
// candidate list, tab[o] = (j0 - off, off + len) -- what to add to a flat position of cell o to get its point, and the
// cell's end. -> the number of candidates. `tab`: the wave's 32 int2 of LDS.
__device__ __forceinline__ int window_table(int wb, int wx, int wy, int wz, int nc, const int2* __restrict__ ct, int lane,
                                            int2* tab) {
    int j0 = 0, len = 0;
    if (lane < 27) {
        const int slab = lane / 9, u = lane - slab * 9;
        const int X = wx + 1 - (u % 3), Y = wy + 1 - (u / 3), Z = wz + 1 - slab;
        if (X >= 0 && X < nc && Y >= 0 && Y < nc && Z >= 0 && Z < nc) {
            const int2 r = ct[(size_t)wb * nc * nc * nc + (size_t)X * nc * nc + (size_t)Y * nc + Z];
            j0 = r.x;
            len = r.y - r.x;
        }
    }
    const int off = wave_incl_scan(len) - len;   // flat offset of cell `lane` in the canonical candidate list
    const int total = __builtin_amdgcn_readlane(off + len, 26);
    __builtin_amdgcn_wave_barrier();
    if (lane < 27) tab[lane] = make_int2(j0 - off, off + len);
    __builtin_amdgcn_wave_barrier();
    return total;
}

// point index of flat position f of the window: its cell by a 5-step binary search over the 27 cell ends
__device__ __forceinline__ int flat_to_j(const int2* tab, int f) {
    int lo = 0, hi = 26;  // smallest o with end[o] > f
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const int mid = (lo + hi) >> 1;
        const bool right = tab[mid].y <= f;
        lo = right ? mid + 1 : lo;
        hi = right ? hi : mid;
    }
    return tab[lo].x + f;  // (j0 - off) + f
}

// ---- 3. the segmented sweep of the density bodies: the `total` candidates of a window in segments of MCCNN_PP_CAP, staged
// in the wave's `lw` as float4 and read back with lanes = candidates. stage(q) -> what is kept of point q (q clamped into
// [0, n): a valid cell table never needs it); round(p, in, members) once per 64 candidates: p the lane's candidate, `in`
// false on the lanes beyond the segment's end (p is then the segment's last, a defined value). One conflict-free
// ds_read_b128 per round serves every member of the cell.
template <class Stage, class Round>
__device__ __forceinline__ void window_sweep(const int2* tab, float4* lw, int total, int n, int lane, unsigned members,
                                             Stage stage, Round round) {
    for (int seg = 0; seg < total; seg += MCCNN_PP_CAP) {
        const int segN = min(MCCNN_PP_CAP, total - seg);
        for (int r = 0; r < segN; r += 64) {
            const int q = min(max(flat_to_j(tab, min(seg + r + lane, total - 1)), 0), n - 1);
            if (r + lane < segN) lw[r + lane] = stage(q);
        }
        __builtin_amdgcn_wave_barrier();
        for (int r = 0; r < segN; r += 64) {
            const int t = r + lane;
            round(lw[min(t, segN - 1)], t < segN, members);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace mccnn
