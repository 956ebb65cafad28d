// Per-POINT kernel density estimate (pdfMode = 'point'): the Gaussian sum of every sorted point over its own ball, once
// per point, and its expansion to the edges of a neighbour list. The per-edge form (neighbors.hip: compute_pdf) sums over
// the CENTRE's row for every edge -- sum of k_i^2 pair terms; this one sweeps the 27-cell window once per point and depends
// on (grid, window) only, so every list over the same grid shares it.
#include "batch.h"
#include <cstring>
#include <cmath>

namespace mccnn {

#ifndef MCCNN_PP_CAP
#define MCCNN_PP_CAP 256   // candidates staged per segment and wave (a multiple of 64)
#endif

// One wave per G consecutive SORTED points (cell-coherent by construction: no visiting order needed). The points of one
// cell share their 27-cell window: the wave stages the window's candidates once in LDS as float4 (canonical order of the
// search, neighbors.hip: neigh_window_body -- the table set-up below is that kernel's, kept apart so that the search
// compiles to what it did) and tests every member against them with lanes = candidates: one conflict-free ds_read_b128
// serves all members of the cell, whose coordinates are wave-uniform (SGPRs). Each lane keeps a (sum, count) pair per
// member and adds hit ? exp2(c d2) : 0 -- no ballots, masks or second pass; one butterfly reduction per member at the
// end, lane g writes member g. No atomics: per lane the candidates arrive in canonical order and the butterfly is a fixed
// tree, so the same inputs give the same bytes. Membership is the search's own predicate: d2 = dx*dx + dy*dy + dz*dz
// without FMA (point_dist2) against T = sqrt_threshold(R_b), or the host's threshold for an absolute radius.
// (The other mapping -- lanes = points, candidates broadcast from LDS -- needs one LDS read per pair step and leaves the
// lanes beyond a cell's population idle: ~8 points per cell on a room.)
// (One body, two thin kernels: `a` is the record the host fills -- PointPdfItem, batch.h -- and (blk, nblk) the workgroup's
// place among the workgroups of ITS item; the single form hands in its own grid, the batch form what batch_item finds.)
template <int G>
__device__ __forceinline__ void pdf_points_body(const PointPdfItem& a, int blk, int nblk) {
    const float* __restrict__ pts = a.pts;
    const int* __restrict__ bids = a.bids;
    const int* __restrict__ cells = a.cells;
    const float* __restrict__ mn = a.mn;
    const float* __restrict__ mx = a.mx;
    float* __restrict__ density = a.density;
    int* __restrict__ counts = a.counts;
    const int n = a.n, B = a.B, nc = a.nc, scaleInv = a.scaleInv;
    const float window = a.window, radius = a.radius, Tabs = a.Tabs;
    static_assert(G >= 1 && G <= 8, "members per wave: lanes 0 .. G-1, accumulators in registers");
    __shared__ float4 win[4][MCCNN_PP_CAP];
    __shared__ int2 ctab[4][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (xcd_contiguous(blk, nblk) * 4 + wave) * G;
    if (g0 >= n) return;
    float4* lw = win[wave];
    int2* tab = ctab[wave];
    // lanes 0 .. G-1: one point each
    const int ji = g0 + lane;
    const bool own = lane < G && ji < n;
    const int j = own ? ji : g0;
    const float px = pts[(size_t)j * 3], py = pts[(size_t)j * 3 + 1], pz = pts[(size_t)j * 3 + 2];
    const int b = clamp_batch(bids[j], B);
    const float ext = max_extent(mn, mx, b);
    const float cs = ext / (float)nc;
    const float R = scaleInv ? radius * ext : radius;               // (centre_ctx of the search)
    const float T = scaleInv ? sqrt_threshold(R) : Tabs;
    const float s = (float)(1.0 / (double)(R * window));            // 1 / (R h); inf for R = 0, where nothing is a hit
    const float cexp = (-0.5f * 1.44269504088896f) * (s * s);       // exp(-|d s|^2 / 2) = exp2(cexp |d|^2)
    const int X = cell_coord(px, mn[b * 3], cs, nc), Y = cell_coord(py, mn[b * 3 + 1], cs, nc);
    const int Z = cell_coord(pz, mn[b * 3 + 2], cs, nc);
    const int key = own ? ((b * nc + X) * nc + Y) * nc + Z : -1;
    // the members' coordinates, thresholds and exponent scales, wave-uniform (SGPRs)
    float mxs[G], mys[G], mzs[G], mT[G], mc[G], acc[G];
    int cnt[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mxs[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px), g));
        mys[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py), g));
        mzs[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz), g));
        mT[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T), g));
        mc[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cexp), g));
        acc[g] = 0.f;
        cnt[g] = 0;
    }
    unsigned todo = (unsigned)(__ballot(own) & ((1ull << G) - 1));
    const int2* ct = reinterpret_cast<const int2*>(cells);
    while (todo) {
        const int lead = __builtin_ctz(todo);
        const int wkey = __builtin_amdgcn_readlane(key, lead);
        const unsigned members = (unsigned)(__ballot(own && key == wkey)) & todo;
        todo &= ~members;
        // the 27 cell ranges of the window: lane o < 27 owns table entry o (find_neighbors.cu:282-291)
        const int wb = __builtin_amdgcn_readlane(b, lead), wx = __builtin_amdgcn_readlane(X, lead);
        const int wy = __builtin_amdgcn_readlane(Y, lead), wz = __builtin_amdgcn_readlane(Z, lead);
        int j0 = 0, len = 0;
        if (lane < 27) {
            const int slab = lane / 9, u = lane - slab * 9;
            const int cx = wx + 1 - (u % 3), cy = wy + 1 - (u / 3), cz = wz + 1 - slab;
            if (cx >= 0 && cx < nc && cy >= 0 && cy < nc && cz >= 0 && cz < nc) {
                const int2 r = ct[(size_t)wb * nc * nc * nc + (size_t)cx * nc * nc + (size_t)cy * nc + cz];
                j0 = r.x;
                len = r.y - r.x;
            }
        }
        const int off = wave_incl_scan(len) - len;   // flat offset of cell `lane` in the canonical candidate list
        const int total = __builtin_amdgcn_readlane(off + len, 26);
        __builtin_amdgcn_wave_barrier();
        if (lane < 27) tab[lane] = make_int2(j0 - off, off + len);
        __builtin_amdgcn_wave_barrier();
        for (int seg = 0; seg < total; seg += MCCNN_PP_CAP) {
            const int segN = min(MCCNN_PP_CAP, total - seg);
            // stage [seg, seg + segN) of the flat list: its cell by a 5-step binary search over the 27 cell ends
            for (int r = 0; r < segN; r += 64) {
                const int f = min(seg + r + lane, total - 1);
                int lo = 0, hi = 26;  // smallest o with end[o] > f
#pragma unroll
                for (int it = 0; it < 5; ++it) {
                    const int mid = (lo + hi) >> 1;
                    const bool right = tab[mid].y <= f;
                    lo = right ? mid + 1 : lo;
                    hi = right ? hi : mid;
                }
                const int q = min(max(tab[lo].x + f, 0), n - 1);   // (a valid cell table never needs the clamp)
                const float* p = pts + (size_t)q * 3;
                if (r + lane < segN) lw[r + lane] = make_float4(p[0], p[1], p[2], 0.f);
            }
            __builtin_amdgcn_wave_barrier();
            // one LDS read per 64 candidates serves every member of the cell
            for (int r = 0; r < segN; r += 64) {
                const int t = r + lane;
                const float4 p = lw[min(t, segN - 1)];
                const bool in = t < segN;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if ((members >> g) & 1u) {   // wave-uniform
                        const float d2 = point_dist2(p.x, p.y, p.z, mxs[g], mys[g], mzs[g]);
                        const bool hit = in && d2 < mT[g];
                        acc[g] += hit ? __builtin_amdgcn_exp2f(mc[g] * d2) : 0.f;
                        cnt[g] += hit ? 1 : 0;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    const float g1 = (1.0f / window) * 0.39894228f;
    const float norm = g1 * g1 * g1;
    float myS = 0.f;
    int myC = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float a = acc[g];
        int c = cnt[g];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            a += __shfl_xor(a, d, 64);
            c += __shfl_xor(c, d, 64);
        }
        if (lane == g) { myS = a; myC = c; }
    }
    if (own) {
        density[ji] = myC > 0 ? myS * norm : 0.f;
        counts[ji] = myC;
    }
}

template <int G>
__global__ __launch_bounds__(256) void pdf_points_k(PointPdfItem a) {
    pdf_points_body<G>(a, (int)blockIdx.x, (int)gridDim.x);
}

// One launch over the points of up to MCCNN_BATCH_MAX grids (mccnn_geometry_build_batch_point): ONE G for all items -- a
// point's density does not depend on it (see above), so every item gets the bytes of its single form.
template <int G>
__global__ __launch_bounds__(256) void pdf_points_batch_k(PointPdfBatch pb, BatchBlocks bb) {
    int local, blocks;
    const PointPdfItem& a = pb.it[batch_item(bb, (int)blockIdx.x, local, blocks)];
    pdf_points_body<G>(a, local, blocks);
}

// One thread per edge (j, i): pdfs[e] = density[j] / float(len_i), the reference's division by the row length
// (compute_pdf.cu:92), one correctly rounded f32 divide.
__global__ __launch_bounds__(256) void expand_pdf_k(const float* __restrict__ density, const int* __restrict__ startIdx, int m,
                                                    const int2* __restrict__ packed, int e, float* __restrict__ pdfs) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= e) return;
    const int2 pr = packed[t];
    const int i = max(0, min(pr.y, m - 1));
    const int i0 = startIdx[i];
    const int i1 = (i < m - 1) ? startIdx[i + 1] : e;
    pdfs[t] = density[pr.x] / (float)(i1 - i0);
}

// The same inside a geometry's chain, where the edge total exists only in the device word: grid-stride over
// E = min(*total_dev, e_capacity) edges, the last row ends at E; nothing is written beyond E. A list that overflowed its
// capacity (the geometry is rebuilt afterwards) holds rows cut at the capacity and start indices beyond it: every index is
// clamped into its buffer (n points, m rows) and such a row's values are never used.
__device__ __forceinline__ void expand_pdf_dn_body(const ExpandItem& a, int blk, int nblk) {
    const int E = min(max(*a.totalDev, 0), a.eCap);
    const int2* __restrict__ packed = a.packed;
    const int* __restrict__ startIdx = a.startIdx;
    const float* __restrict__ density = a.density;
    float* __restrict__ pdfs = a.pdfs;
    const int m = a.m, n = a.n;
    const long long stride = (long long)nblk * 256;
    for (long long t = (long long)blk * 256 + threadIdx.x; t < E; t += stride) {
        const int2 pr = packed[t];
        const int i = max(0, min(pr.y, m - 1));
        const int j = max(0, min(pr.x, n - 1));
        const int i0 = startIdx[i];
        const int i1 = (i < m - 1) ? min(startIdx[i + 1], E) : E;
        pdfs[t] = density[j] / (float)(i1 - i0);
    }
}
__global__ __launch_bounds__(256) void expand_pdf_dn_k(ExpandItem a) { expand_pdf_dn_body(a, (int)blockIdx.x, (int)gridDim.x); }
__global__ __launch_bounds__(256) void expand_pdf_dn_batch_k(ExpandBatch eb, BatchBlocks bb) {
    int local, blocks;
    const ExpandItem& a = eb.it[batch_item(bb, (int)blockIdx.x, local, blocks)];
    expand_pdf_dn_body(a, local, blocks);
}

// sqrt_threshold (common.h) on the host: the same float operations, both square roots correctly rounded (as
// neighbors.hip's: an absolute radius has ONE threshold, computed once per call)
static float pp_sqrt_threshold_host(float R) {
    auto prev = [](float v) { uint32_t u; memcpy(&u, &v, 4); --u; memcpy(&v, &u, 4); return v; };
    auto next = [](float v) { uint32_t u; memcpy(&u, &v, 4); ++u; memcpy(&v, &u, 4); return v; };
    float t = R * R;
    for (int it = 0; it < 8 && t > 0.0f && sqrtf(prev(t)) >= R; ++it) t = prev(t);
    for (int it = 0; it < 8 && sqrtf(t) < R; ++it) t = next(t);
    return t;
}

// points per wave: 8 share most of their windows on a large level, a small one needs the waves (neigh_group of the search)
static int pp_group(long long n) { return n >= 32768 ? 8 : n >= 16384 ? 4 : n >= 8192 ? 2 : 1; }

int point_pdf_item(PointPdfItem& it, const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                   const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window, float radius,
                   int scale_inv, float* density, int* counts) {
    if (n <= 0 || batch_size <= 0 || num_cells <= 0 || !(radius > 0.0f) || !(window > 0.0f)) return MCCNN_E_BADARG;
    if (!sorted_pts || !sorted_batch_ids || !cell_indexs || !aabb_min || !aabb_max || !density || !counts) return MCCNN_E_BADARG;
    it = PointPdfItem{sorted_pts, sorted_batch_ids, cell_indexs, aabb_min, aabb_max, density, counts, n, batch_size, num_cells,
                      scale_inv ? 1 : 0, window, radius, scale_inv ? 0.0f : pp_sqrt_threshold_host(radius)};
    return 0;
}

int launch_point_pdf(const PointPdfItem& it, hipStream_t s) {
#define MCCNN_PP_LAUNCH(G) pdf_points_k<G><<<ceil_div(it.n, 4 * G), 256, 0, s>>>(it)
    switch (pp_group(it.n)) {
        case 8: MCCNN_PP_LAUNCH(8); break;
        case 4: MCCNN_PP_LAUNCH(4); break;
        case 2: MCCNN_PP_LAUNCH(2); break;
        default: MCCNN_PP_LAUNCH(1); break;
    }
#undef MCCNN_PP_LAUNCH
    MCCNN_LAUNCHED();
    return 0;
}

// ONE G for the launch, from the points of all its items together (what fills the chip is their sum)
int launch_point_pdf_batch(const PointPdfBatch& pb, int count, hipStream_t s) {
    if (count <= 0) return 0;
    if (count > MCCNN_BATCH_MAX) return MCCNN_E_BADARG;
    long long total = 0;
    for (int k = 0; k < count; ++k) total += pb.it[k].n;
    const int G = pp_group(total);
    BatchBlocks bb;
    bb.count = count;
    int run = 0;
    for (int k = 0; k < count; ++k) { bb.first[k] = run; run += ceil_div(pb.it[k].n, 4 * G); }
    for (int k = count; k <= MCCNN_BATCH_MAX; ++k) bb.first[k] = run;
    if (run == 0) return 0;
#define MCCNN_PP_LAUNCH(G) pdf_points_batch_k<G><<<run, 256, 0, s>>>(pb, bb)
    switch (G) {
        case 8: MCCNN_PP_LAUNCH(8); break;
        case 4: MCCNN_PP_LAUNCH(4); break;
        case 2: MCCNN_PP_LAUNCH(2); break;
        default: MCCNN_PP_LAUNCH(1); break;
    }
#undef MCCNN_PP_LAUNCH
    MCCNN_LAUNCHED();
    return 0;
}

// workgroups of one expansion: one per 1024 edges of the capacity (four grid-stride steps each), at most 1024
static int expand_blocks(int e_cap) { return max(1, min(ceil_div(e_cap, 1024), 1024)); }

int expand_item(ExpandItem& it, const float* density, int n, const int* start_idx, int m, const int* packed, int e_capacity,
                const int* total_dev, float* pdfs) {
    if (n <= 0 || m <= 0 || e_capacity <= 0 || !density || !start_idx || !packed || !total_dev || !pdfs) return MCCNN_E_BADARG;
    it = ExpandItem{density, start_idx, reinterpret_cast<const int2*>(packed), total_dev, pdfs, n, m, e_capacity};
    return 0;
}

int launch_expand_dn(const ExpandItem& it, hipStream_t s) {
    expand_pdf_dn_k<<<expand_blocks(it.eCap), 256, 0, s>>>(it);
    MCCNN_LAUNCHED();
    return 0;
}

int launch_expand_batch(const ExpandBatch& eb, int count, hipStream_t s) {
    if (count <= 0) return 0;
    if (count > MCCNN_BATCH_MAX) return MCCNN_E_BADARG;
    BatchBlocks bb;
    bb.count = count;
    int run = 0;
    for (int k = 0; k < count; ++k) { bb.first[k] = run; run += expand_blocks(eb.it[k].eCap); }
    for (int k = count; k <= MCCNN_BATCH_MAX; ++k) bb.first[k] = run;
    expand_pdf_dn_batch_k<<<run, 256, 0, s>>>(eb, bb);
    MCCNN_LAUNCHED();
    return 0;
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

int mccnn_compute_pdf_points(const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                             const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window,
                             float radius, int scale_inv, float* density, int* counts, mccnn_stream_t stream) {
    if (n < 0 || batch_size <= 0 || num_cells <= 0 || !(radius > 0.0f) || !(window > 0.0f)) return MCCNN_E_BADARG;
    if (n == 0) return 0;
    PointPdfItem it;
    int rc = point_pdf_item(it, sorted_pts, sorted_batch_ids, n, cell_indexs, aabb_min, aabb_max, batch_size, num_cells, window,
                            radius, scale_inv, density, counts);
    if (rc) return rc;
    return launch_point_pdf(it, (hipStream_t)stream);
}

int mccnn_expand_pdf(const float* density, const int* start_idx, int m, const int* packed, int e, float* pdfs,
                     mccnn_stream_t stream) {
    if (m < 0 || e < 0) return MCCNN_E_BADARG;
    if (e == 0) return 0;
    if (!density || !start_idx || !packed || !pdfs || m == 0) return MCCNN_E_BADARG;
    expand_pdf_k<<<ceil_div(e, 256), 256, 0, (hipStream_t)stream>>>(density, start_idx, m, reinterpret_cast<const int2*>(packed), e,
                                                                   pdfs);
    MCCNN_LAUNCHED();
    return 0;
}

}  // extern "C"
