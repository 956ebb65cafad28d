// Gradients of the per-point kernel density estimate (pdf_points.hip) with respect to positions: the sweep backward, the
// per-cloud sum of its radius terms and the expansion backward.
#include "batch.h"

namespace mccnn {

#ifndef MCCNN_PP_CAP
#define MCCNN_PP_CAP 256   // candidates staged per segment and wave (pdf_points.hip)
#endif

// ---- gradients with respect to positions --------------------------------------------------------------------------------
// density[j] = norm sum_{l in N(j)} w_jl, w_jl = exp(-0.5 s_b^2 d2_jl). Inside a cloud the ball relation is symmetric (d2
// without FMA is the same f32 number from both ends; R_b, T and s_b are per cloud): l in N(j) <=> j in N(l), so everything
// that depends on p_j -- its own sum and its terms in the sums of its neighbours -- is summed by the wave that owns j:
//   dpts[j] = -s_b^2 norm sum_{l in N(j)} (gd[j] + gd[l]) w_jl (p_j - p_l)
//   dRpt[j] =  gd[j] norm (s_b^2 / R_b) sum_{l in N(j)} w_jl d2_jl          (BOX: scaleInv and a box gradient wanted)
// The forward's sweep again, in gather form (the set-up below is pdf_points_body's; this file is a translation unit of its
// own because the G = 1 forward kernels compile differently with these templates beside them, see NOTES): candidates staged as (x, y, z, gd[l]), three (BOX: four) accumulators per member and lane, one
// butterfly per accumulator at the end, lane g stores member g. No atomics, no per-edge rows, no transposed list: the same
// inputs give the same bytes. Every discrete decision (cells, membership, the longest box axis) is held fixed. A point
// whose ball is empty (R_b = 0: the one-point cloud under a relative radius, s = inf) stores exact zeros.
template <int G, bool BOX>
__device__ __forceinline__ void pdf_points_bwd_body(const PointPdfItem& a, const float* __restrict__ gd,
                                                    float* __restrict__ dpts, float* __restrict__ dRpt, int blk, int nblk) {
    const float* __restrict__ pts = a.pts;
    const int* __restrict__ bids = a.bids;
    const int* __restrict__ cells = a.cells;
    const float* __restrict__ mn = a.mn;
    const float* __restrict__ mx = a.mx;
    const int n = a.n, B = a.B, nc = a.nc, scaleInv = a.scaleInv;
    const float window = a.window, radius = a.radius, Tabs = a.Tabs;
    static_assert(G >= 1 && G <= 4, "members per wave: lanes 0 .. G-1, accumulators in registers");
    __shared__ float4 win[4][MCCNN_PP_CAP];
    __shared__ int2 ctab[4][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (xcd_contiguous(blk, nblk) * 4 + wave) * G;
    if (g0 >= n) return;
    float4* lw = win[wave];
    int2* tab = ctab[wave];
    const int ji = g0 + lane;
    const bool own = lane < G && ji < n;
    const int j = own ? ji : g0;
    const float px = pts[(size_t)j * 3], py = pts[(size_t)j * 3 + 1], pz = pts[(size_t)j * 3 + 2];
    const float gj = gd[j];
    const int b = clamp_batch(bids[j], B);
    const float ext = max_extent(mn, mx, b);
    const float cs = ext / (float)nc;
    const float R = scaleInv ? radius * ext : radius;
    const float T = scaleInv ? sqrt_threshold(R) : Tabs;
    const float s = (float)(1.0 / (double)(R * window));
    const float s2 = s * s;
    const float cexp = (-0.5f * 1.44269504088896f) * s2;
    const int X = cell_coord(px, mn[b * 3], cs, nc), Y = cell_coord(py, mn[b * 3 + 1], cs, nc);
    const int Z = cell_coord(pz, mn[b * 3 + 2], cs, nc);
    const int key = own ? ((b * nc + X) * nc + Y) * nc + Z : -1;
    float mxs[G], mys[G], mzs[G], mT[G], mc[G], mg[G], ax[G], ay[G], az[G], ar[BOX ? G : 1];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mxs[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px), g));
        mys[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py), g));
        mzs[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz), g));
        mT[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T), g));
        mc[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cexp), g));
        mg[g] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gj), g));
        ax[g] = ay[g] = az[g] = 0.f;
        if (BOX) ar[g] = 0.f;
    }
    unsigned todo = (unsigned)(__ballot(own) & ((1ull << G) - 1));
    const int2* ct = reinterpret_cast<const int2*>(cells);
    while (todo) {
        const int lead = __builtin_ctz(todo);
        const int wkey = __builtin_amdgcn_readlane(key, lead);
        const unsigned members = (unsigned)(__ballot(own && key == wkey)) & todo;
        todo &= ~members;
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
        const int off = wave_incl_scan(len) - len;
        const int total = __builtin_amdgcn_readlane(off + len, 26);
        __builtin_amdgcn_wave_barrier();
        if (lane < 27) tab[lane] = make_int2(j0 - off, off + len);
        __builtin_amdgcn_wave_barrier();
        for (int seg = 0; seg < total; seg += MCCNN_PP_CAP) {
            const int segN = min(MCCNN_PP_CAP, total - seg);
            for (int r = 0; r < segN; r += 64) {
                const int f = min(seg + r + lane, total - 1);
                int lo = 0, hi = 26;
#pragma unroll
                for (int it = 0; it < 5; ++it) {
                    const int mid = (lo + hi) >> 1;
                    const bool right = tab[mid].y <= f;
                    lo = right ? mid + 1 : lo;
                    hi = right ? hi : mid;
                }
                const int q = min(max(tab[lo].x + f, 0), n - 1);
                const float* p = pts + (size_t)q * 3;
                if (r + lane < segN) lw[r + lane] = make_float4(p[0], p[1], p[2], gd[q]);
            }
            __builtin_amdgcn_wave_barrier();
            for (int r = 0; r < segN; r += 64) {
                const int t = r + lane;
                const float4 p = lw[min(t, segN - 1)];
                const bool in = t < segN;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if ((members >> g) & 1u) {   // wave-uniform
                        // (the forward's d2: the candidate first, so that membership is the forward's bit for bit)
                        const float dx = p.x - mxs[g], dy = p.y - mys[g], dz = p.z - mzs[g];
                        const float d2 = dx * dx + dy * dy + dz * dz;
                        const bool hit = in && d2 < mT[g];
                        const float w = hit ? __builtin_amdgcn_exp2f(mc[g] * d2) : 0.f;
                        const float c = (mg[g] + p.w) * w;
                        ax[g] = fmaf(c, dx, ax[g]);     // sum of c (p_l - p_j): the sign goes into the final scale
                        ay[g] = fmaf(c, dy, ay[g]);
                        az[g] = fmaf(c, dz, az[g]);
                        if (BOX) ar[g] = fmaf(w, d2, ar[g]);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
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
        const bool live = R > 0.f && s2 < 3.0e38f;
        const float k = live ? s2 * norm : 0.f;     // d/dp_j of -0.5 s^2 |p_j - p_l|^2 = s^2 (p_l - p_j)
        float* o = dpts + (size_t)ji * 3;
        o[0] = live ? k * m0 : 0.f;
        o[1] = live ? k * m1 : 0.f;
        o[2] = live ? k * m2 : 0.f;
        if (BOX) dRpt[ji] = live ? gj * norm * (s2 / R) * m3 : 0.f;
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

// points per wave: the forward's rule (pp_group, pdf_points.hip) up to 4. Eight members need six wave-uniform values each
// (the forward: five) beside 24 or 32 accumulators, which no longer fit the scalar registers (10 - 12 SGPRs spilled at G = 8).
static int pp_bwd_group(long long n) { return n >= 16384 ? 4 : n >= 8192 ? 2 : 1; }

}  // namespace mccnn

using namespace mccnn;

extern "C" {

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
    switch (pp_bwd_group(n)) {
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
