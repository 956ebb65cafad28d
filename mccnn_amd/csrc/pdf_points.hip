// Per-POINT kernel density estimate (pdfMode = 'point'): the Gaussian sum of every sorted point over its own ball, once
// per point, and its expansion to the edges of a neighbour list. The per-edge form (neighbors.hip: compute_pdf) sums over
// the CENTRE's row for every edge -- sum of k_i^2 pair terms; this one sweeps the 27-cell window once per point and depends
// on (grid, window) only, so every list over the same grid shares it.
#include "common.h"
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
template <int G>
__global__ __launch_bounds__(256) void pdf_points_k(const float* __restrict__ pts, const int* __restrict__ bids, int n,
                                                    const int* __restrict__ cells, const float* __restrict__ mn,
                                                    const float* __restrict__ mx, int B, int nc, float window, float radius,
                                                    int scaleInv, float Tabs, float* __restrict__ density,
                                                    int* __restrict__ counts) {
    static_assert(G >= 1 && G <= 8, "members per wave: lanes 0 .. G-1, accumulators in registers");
    __shared__ float4 win[4][MCCNN_PP_CAP];
    __shared__ int2 ctab[4][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (xcd_contiguous((int)blockIdx.x, (int)gridDim.x) * 4 + wave) * G;
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

}  // namespace mccnn

using namespace mccnn;

extern "C" {

int mccnn_compute_pdf_points(const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                             const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window,
                             float radius, int scale_inv, float* density, int* counts, mccnn_stream_t stream) {
    if (n < 0 || batch_size <= 0 || num_cells <= 0 || !(radius > 0.0f) || !(window > 0.0f)) return MCCNN_E_BADARG;
    if (n == 0) return 0;
    if (!sorted_pts || !sorted_batch_ids || !cell_indexs || !aabb_min || !aabb_max || !density || !counts) return MCCNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const float Tabs = scale_inv ? 0.0f : pp_sqrt_threshold_host(radius);
    // points per wave: 8 share most of their windows on a large level, a small one needs the waves (neigh_group of the search)
#define MCCNN_PP_LAUNCH(G)                                                                                                  \
    pdf_points_k<G><<<ceil_div(n, 4 * G), 256, 0, s>>>(sorted_pts, sorted_batch_ids, n, cell_indexs, aabb_min, aabb_max,    \
                                                      batch_size, num_cells, window, radius, scale_inv, Tabs, density, counts)
    if (n >= 32768) MCCNN_PP_LAUNCH(8);
    else if (n >= 16384) MCCNN_PP_LAUNCH(4);
    else if (n >= 8192) MCCNN_PP_LAUNCH(2);
    else MCCNN_PP_LAUNCH(1);
#undef MCCNN_PP_LAUNCH
    MCCNN_LAUNCHED();
    return 0;
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
