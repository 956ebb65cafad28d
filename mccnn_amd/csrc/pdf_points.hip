// Per-POINT kernel density estimate (pdfMode = 'point'): the Gaussian sum of every sorted point over its own ball, once
// per point, its expansion to the edges of a neighbour list, and the gradients of both. The per-edge form (neighbors.hip: compute_pdf) sums over
// the CENTRE's row for every edge -- sum of k_i^2 pair terms; this one sweeps the 27-cell window once per point and depends
// on (grid, window) only, so every list over the same grid shares it.
#include "batch.h"
#include "cell_window.h"

namespace mccnn {

// One wave per G consecutive SORTED points (cell-coherent by construction: no visiting order needed). The points of one
// cell share their 27-cell window: the wave stages the window's candidates once in LDS as float4 (the window walk of the
// search, piece by piece: cell_window.h) and tests every member against them with lanes = candidates: one conflict-free
// ds_read_b128 serves all members of the cell, whose coordinates are wave-uniform (SGPRs). Each lane keeps a (sum, count)
// pair per member and adds hit ? exp2(c d2) : 0 -- no ballots, masks or second pass; one butterfly reduction per member at
// the end, lane g writes member g. No atomics: per lane the candidates arrive in canonical order and the butterfly is a
// fixed tree, so the same inputs give the same bytes. Membership is the search's own predicate: d2 = dx*dx + dy*dy + dz*dz
// without FMA (point_dist2) against T = sqrt_threshold(R_b), or the host's threshold for an absolute radius.
// (The other mapping -- lanes = points, candidates broadcast from LDS -- needs one LDS read per pair step and leaves the
// lanes beyond a cell's population idle: ~8 points per cell on a room.)
// (One body, two thin kernels: `a` is the record the host fills -- PointPdfItem, batch.h -- and (blk, nblk) the workgroup's
// place among the workgroups of ITS item; the single form hands in its own grid, the batch form what batch_item finds.)
template <int G>
__device__ __forceinline__ void pdf_points_body(const PointPdfItem& a, int blk, int nblk) {
    const float* __restrict__ pts = a.pts;
    float* __restrict__ density = a.density;
    int* __restrict__ counts = a.counts;
    const int n = a.n, nc = a.nc;
    const float window = a.window;
    static_assert(G >= 1 && G <= 8, "members per wave: lanes 0 .. G-1, accumulators in registers");
    __shared__ float4 win[4][MCCNN_PP_CAP];
    __shared__ int2 ctab[4][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (xcd_contiguous(blk, nblk) * 4 + wave) * G;
    if (g0 >= n) return;
    // lanes 0 .. G-1: one point each
    const int ji = g0 + lane;
    const bool own = lane < G && ji < n;
    const CentreCtx c = centre_ctx(pts, a.bids, a.mn, a.mx, own ? ji : g0, a.B, nc, a.radius, a.scaleInv, a.Tabs);
    const float s = (float)(1.0 / (double)(c.R * window));          // 1 / (R h); inf for R = 0, where nothing is a hit
    const float cexp = (-0.5f * 1.44269504088896f) * (s * s);       // exp(-|d s|^2 / 2) = exp2(cexp |d|^2)
    const int key = cell_key(c, nc, own);
    // the members' coordinates, thresholds and exponent scales, wave-uniform (SGPRs)
    float mxs[G], mys[G], mzs[G], mT[G], mc[G], acc[G];
    int cnt[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mxs[g] = readlane_f(c.cx, g);
        mys[g] = readlane_f(c.cy, g);
        mzs[g] = readlane_f(c.cz, g);
        mT[g] = readlane_f(c.T, g);
        mc[g] = readlane_f(cexp, g);
        acc[g] = 0.f;
        cnt[g] = 0;
    }
    unsigned todo = (unsigned)(__ballot(own) & ((1ull << G) - 1));
    while (todo) {
        int lead;
        const unsigned members = window_next_group(todo, own, key, lead);
        const int total = window_table(__builtin_amdgcn_readlane(c.b, lead), __builtin_amdgcn_readlane(c.x, lead),
                                       __builtin_amdgcn_readlane(c.y, lead), __builtin_amdgcn_readlane(c.z, lead), nc,
                                       reinterpret_cast<const int2*>(a.cells), lane, ctab[wave]);
        window_sweep(
            ctab[wave], win[wave], total, n, lane, members,
            [&](int q) { return make_float4(pts[(size_t)q * 3], pts[(size_t)q * 3 + 1], pts[(size_t)q * 3 + 2], 0.f); },
            [&](const float4 p, bool in, unsigned mem) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if ((mem >> g) & 1u) {   // wave-uniform
                        const float d2 = point_dist2(p.x, p.y, p.z, mxs[g], mys[g], mzs[g]);
                        const bool hit = in && d2 < mT[g];
                        acc[g] += hit ? __builtin_amdgcn_exp2f(mc[g] * d2) : 0.f;
                        cnt[g] += hit ? 1 : 0;
                    }
                }
            });
    }
    const float g1 = (1.0f / window) * 0.39894228f;
    const float norm = g1 * g1 * g1;
    float myS = 0.f;
    int myC = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float sv = acc[g];
        int cv = cnt[g];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sv += __shfl_xor(sv, d, 64);
            cv += __shfl_xor(cv, d, 64);
        }
        if (lane == g) { myS = sv; myC = cv; }
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

// ---- gradients with respect to positions --------------------------------------------------------------------------------
// density[j] = norm sum_{l in N(j)} w_jl, w_jl = exp(-0.5 s_b^2 d2_jl). Inside a cloud the ball relation is symmetric (d2
// without FMA is the same f32 number from both ends; R_b, T and s_b are per cloud): l in N(j) <=> j in N(l), so everything
// that depends on p_j -- its own sum and its terms in the sums of its neighbours -- is summed by the wave that owns j:
//   dpts[j] = -s_b^2 norm sum_{l in N(j)} (gd[j] + gd[l]) w_jl (p_j - p_l)
//   dRpt[j] =  gd[j] norm (s_b^2 / R_b) sum_{l in N(j)} w_jl d2_jl          (BOX: scaleInv and a box gradient wanted)
// The forward's sweep again, in gather form, over the same pieces (cell_window.h: context, groups, table, segmented sweep):
// candidates staged as (x, y, z, gd[l]), three (BOX: four) accumulators per member and lane, one butterfly per accumulator
// at the end, lane g stores member g. No atomics, no per-edge rows, no transposed list: the same inputs give the same
// bytes. Every discrete decision (cells, membership, the longest box axis) is held fixed. A point whose ball is empty
// (R_b = 0: the one-point cloud under a relative radius, s = inf) stores exact zeros.
// (In this file again: with these templates beside them every forward kernel keeps its registers, waves per SIMD, LDS and
// instruction count, and so does every kernel here -- NOTES.md, "One window walk".)
template <int G, bool BOX>
__device__ __forceinline__ void pdf_points_bwd_body(const PointPdfItem& a, const float* __restrict__ gd,
                                                    float* __restrict__ dpts, float* __restrict__ dRpt, int blk, int nblk) {
    const float* __restrict__ pts = a.pts;
    const int n = a.n, nc = a.nc;
    const float window = a.window;
    static_assert(G >= 1 && G <= 4, "members per wave: lanes 0 .. G-1, accumulators in registers");
    __shared__ float4 win[4][MCCNN_PP_CAP];
    __shared__ int2 ctab[4][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (xcd_contiguous(blk, nblk) * 4 + wave) * G;
    if (g0 >= n) return;
    const int ji = g0 + lane;
    const bool own = lane < G && ji < n;
    const int j = own ? ji : g0;
    const CentreCtx c = centre_ctx(pts, a.bids, a.mn, a.mx, j, a.B, nc, a.radius, a.scaleInv, a.Tabs);
    const float gj = gd[j];
    const float s = (float)(1.0 / (double)(c.R * window));
    const float s2 = s * s;
    const float cexp = (-0.5f * 1.44269504088896f) * s2;
    const int key = cell_key(c, nc, own);
    float mxs[G], mys[G], mzs[G], mT[G], mc[G], mg[G], ax[G], ay[G], az[G], ar[BOX ? G : 1];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mxs[g] = readlane_f(c.cx, g);
        mys[g] = readlane_f(c.cy, g);
        mzs[g] = readlane_f(c.cz, g);
        mT[g] = readlane_f(c.T, g);
        mc[g] = readlane_f(cexp, g);
        mg[g] = readlane_f(gj, g);
        ax[g] = ay[g] = az[g] = 0.f;
        if (BOX) ar[g] = 0.f;
    }
    unsigned todo = (unsigned)(__ballot(own) & ((1ull << G) - 1));
    while (todo) {
        int lead;
        const unsigned members = window_next_group(todo, own, key, lead);
        const int total = window_table(__builtin_amdgcn_readlane(c.b, lead), __builtin_amdgcn_readlane(c.x, lead),
                                       __builtin_amdgcn_readlane(c.y, lead), __builtin_amdgcn_readlane(c.z, lead), nc,
                                       reinterpret_cast<const int2*>(a.cells), lane, ctab[wave]);
        window_sweep(
            ctab[wave], win[wave], total, n, lane, members,
            [&](int q) { return make_float4(pts[(size_t)q * 3], pts[(size_t)q * 3 + 1], pts[(size_t)q * 3 + 2], gd[q]); },
            [&](const float4 p, bool in, unsigned mem) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if ((mem >> g) & 1u) {   // wave-uniform
                        // (point_dist2 spelled out for its differences: the candidate first, membership is the forward's bit for bit)
                        const float dx = p.x - mxs[g], dy = p.y - mys[g], dz = p.z - mzs[g];
                        const float d2 = dx * dx + dy * dy + dz * dz;
                        const bool hit = in && d2 < mT[g];
                        const float w = hit ? __builtin_amdgcn_exp2f(mc[g] * d2) : 0.f;
                        const float cw = (mg[g] + p.w) * w;
                        ax[g] = fmaf(cw, dx, ax[g]);     // sum of cw (p_l - p_j): the sign goes into the final scale
                        ay[g] = fmaf(cw, dy, ay[g]);
                        az[g] = fmaf(cw, dz, az[g]);
                        if (BOX) ar[g] = fmaf(w, d2, ar[g]);
                    }
                }
            });
    }
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float v0 = ax[g], v1 = ay[g], v2 = az[g], v3 = BOX ? ar[g] : 0.f;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            v0 += __shfl_xor(v0, d, 64);
            v1 += __shfl_xor(v1, d, 64);
            v2 += __shfl_xor(v2, d, 64);
            if (BOX) v3 += __shfl_xor(v3, d, 64);
        }
        if (lane == g) { m0 = v0; m1 = v1; m2 = v2; m3 = v3; }
    }
    if (own) {
        const float g1 = (1.0f / window) * 0.39894228f;
        const float norm = g1 * g1 * g1;
        // R = 0 (or a product R h that leaves the f32 range): s = inf, nothing was a hit -- exact zeros, never 0 * inf
        const bool live = c.R > 0.f && s2 < 3.0e38f;
        const float k = live ? s2 * norm : 0.f;     // d/dp_j of -0.5 s^2 |p_j - p_l|^2 = s^2 (p_l - p_j)
        float* o = dpts + (size_t)ji * 3;
        o[0] = live ? k * m0 : 0.f;
        o[1] = live ? k * m1 : 0.f;
        o[2] = live ? k * m2 : 0.f;
        if (BOX) dRpt[ji] = live ? gj * norm * (s2 / c.R) * m3 : 0.f;
    }
}

template <int G, bool BOX>
__global__ __launch_bounds__(256) void pdf_points_bwd_k(PointPdfItem a, const float* __restrict__ gd, float* __restrict__ dpts,
                                                        float* __restrict__ dRpt) {
    pdf_points_bwd_body<G, BOX>(a, gd, dpts, dRpt, (int)blockIdx.x, (int)gridDim.x);
}

// dR[b] = sum of dRpt over the points of cloud b, one workgroup per cloud, fixed order. The sorted points of a cloud are
// contiguous (the sort key leads with the batch id): two binary searches find its range.
__global__ __launch_bounds__(256) void pdf_points_cloud_sum(const float* __restrict__ dRpt, const int* __restrict__ bids, int n,
                                                            int B, float* __restrict__ dR) {
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int range[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {   // first point whose (clamped) batch id is >= b + k
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (int)(((long long)lo + hi) >> 1);
            if (clamp_batch(bids[mid], B) < b + k) lo = mid + 1; else hi = mid;
        }
        range[k] = lo;
    }
    float s = 0.f;
    for (int r = range[0] + tid; r < range[1]; r += 256) s += dRpt[r];
    red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) dR[b] = red[0];
}

// gd[j] = sum over the edges e whose point is j of g[e] / float(len_centre(e)), in the order of the transposed list
// (start_t, perm_t); 16 lanes per point, a fixed butterfly: no float atomics, the same bytes in every run. Every j is
// stored: a point that no edge names gets 0.f.
constexpr int kExpandLanes = 16;
__global__ __launch_bounds__(256) void expand_pdf_bwd_k(const float* __restrict__ g, const int* __restrict__ startIdx, int m,
                                                        const int2* __restrict__ packed, int e, const int* __restrict__ startT,
                                                        const int* __restrict__ permT, int n, float* __restrict__ gd) {
    const int j = (int)(((long long)blockIdx.x * 256 + threadIdx.x) / kExpandLanes);
    const int l = (int)(threadIdx.x % kExpandLanes);
    const bool act = j < n;
    float s = 0.f;
    if (act) {
        const int k0 = max(0, min(startT[j], e)), k1 = max(0, min(startT[j + 1], e));
        for (int k = k0 + l; k < k1; k += kExpandLanes) {
            const int t = max(0, min(permT[k], e - 1));
            const int i = max(0, min(packed[t].y, m - 1));
            const int i0 = startIdx[i];
            const int i1 = (i < m - 1) ? startIdx[i + 1] : e;
            s += g[t] / (float)(i1 - i0);
        }
    }
#pragma unroll
    for (int o = kExpandLanes / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kExpandLanes);
    if (act && l == 0) gd[j] = s;
}

// (points per wave: window_group, batch.h -- 8 share most of their windows on a large level, a small one needs the waves)
static_assert(MCCNN_NW_G == 8, "the instantiations the launchers below pick from: G = 8, 4, 2, 1");

int point_pdf_item(PointPdfItem& it, const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                   const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window, float radius,
                   int scale_inv, float* density, int* counts) {
    if (n <= 0 || batch_size <= 0 || num_cells <= 0 || !(radius > 0.0f) || !(window > 0.0f)) return MCCNN_E_BADARG;
    if (!sorted_pts || !sorted_batch_ids || !cell_indexs || !aabb_min || !aabb_max || !density || !counts) return MCCNN_E_BADARG;
    it = PointPdfItem{sorted_pts, sorted_batch_ids, cell_indexs, aabb_min, aabb_max, density, counts, n, batch_size, num_cells,
                      scale_inv ? 1 : 0, window, radius, scale_inv ? 0.0f : sqrt_threshold_host(radius)};
    return 0;
}

int launch_point_pdf(const PointPdfItem& it, hipStream_t s) {
#define MCCNN_PP_LAUNCH(G) pdf_points_k<G><<<ceil_div(it.n, 4 * G), 256, 0, s>>>(it)
    switch (window_group(it.n)) {
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
    const int G = window_group(total);
    BatchBlocks bb;
    const int run = batch_blocks(bb, count, [&](int k) { return ceil_div(pb.it[k].n, 4 * G); });
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
    const int run = batch_blocks(bb, count, [&](int k) { return expand_blocks(eb.it[k].eCap); });
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


size_t mccnn_compute_pdf_points_bwd_workspace_bytes(int n, int batch_size) {
    (void)batch_size;
    return align_up((size_t)(n > 0 ? n : 1) * 4) + 256;
}

int mccnn_compute_pdf_points_bwd(const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                                 const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window,
                                 float radius, int scale_inv, const float* density_grad, float* dpts, float* dradius, void* ws,
                                 size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 0 || batch_size <= 0 || num_cells <= 0 || !(radius > 0.0f) || !(window > 0.0f)) return MCCNN_E_BADARG;
    if (dradius && !scale_inv) return MCCNN_E_BADARG;
    if (n == 0) return 0;
    if (!sorted_pts || !sorted_batch_ids || !cell_indexs || !aabb_min || !aabb_max || !density_grad || !dpts) return MCCNN_E_BADARG;
    float* dRpt = nullptr;
    if (dradius) {
        if (!ws || ws_bytes < mccnn_compute_pdf_points_bwd_workspace_bytes(n, batch_size)) return MCCNN_E_WORKSPACE;
        Arena ar(ws, ws_bytes);
        dRpt = ar.take<float>((size_t)n);
        if (!dRpt) return MCCNN_E_WORKSPACE;
    }
    // the forward's record (its host threshold for an absolute radius); the backward writes neither density nor counts
    PointPdfItem it;
    const int rc = point_pdf_item(it, sorted_pts, sorted_batch_ids, n, cell_indexs, aabb_min, aabb_max, batch_size, num_cells, window,
                                  radius, scale_inv, dpts, reinterpret_cast<int*>(dpts));
    if (rc) return rc;
    it.density = nullptr;
    it.counts = nullptr;
    hipStream_t s = (hipStream_t)stream;
#define MCCNN_PP_LAUNCH(G)                                                                                         \
    do {                                                                                                           \
        if (dRpt) pdf_points_bwd_k<G, true><<<ceil_div(n, 4 * G), 256, 0, s>>>(it, density_grad, dpts, dRpt);       \
        else pdf_points_bwd_k<G, false><<<ceil_div(n, 4 * G), 256, 0, s>>>(it, density_grad, dpts, nullptr);        \
    } while (0)
    // points per wave: the forward's rule up to 4. Eight members need six wave-uniform values each (the forward: five) beside
    // 24 or 32 accumulators, which no longer fit the scalar registers (10 - 12 SGPRs spilled at G = 8).
    switch (min(window_group(n), 4)) {
        case 4: MCCNN_PP_LAUNCH(4); break;
        case 2: MCCNN_PP_LAUNCH(2); break;
        default: MCCNN_PP_LAUNCH(1); break;
    }
#undef MCCNN_PP_LAUNCH
    MCCNN_LAUNCHED();
    if (dRpt) {
        pdf_points_cloud_sum<<<batch_size, 256, 0, s>>>(dRpt, sorted_batch_ids, n, batch_size, dradius);
        MCCNN_LAUNCHED();
    }
    return 0;
}

int mccnn_expand_pdf_bwd(float* density_grad, const float* pdfs_grad, const int* start_idx, int m, const int* packed, int e,
                         const int* start_t, const int* perm_t, int n, mccnn_stream_t stream) {
    if (m < 0 || e < 0 || n < 0) return MCCNN_E_BADARG;
    if (n == 0 || e == 0) return 0;
    if (!density_grad || !pdfs_grad || !start_idx || !packed || !start_t || !perm_t || m == 0) return MCCNN_E_BADARG;
    const long long threads = (long long)n * kExpandLanes;
    expand_pdf_bwd_k<<<(int)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        pdfs_grad, start_idx, m, reinterpret_cast<const int2*>(packed), e, start_t, perm_t, n, density_grad);
    MCCNN_LAUNCHED();
    return 0;
}

}  // extern "C"
