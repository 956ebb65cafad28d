// Gradients of the Monte-Carlo convolution with respect to POSITIONS (extension, no TF counterpart): the neighbour points,
// the centres, the per-edge PDFs and, with scale_inv, the per-batch radius R_b = radius * maxExtent_b.
//
// Every discrete decision of the forward pass (cells, sort order, neighbour sets, K of `avg`) is held fixed; the result is
// the exact derivative of the forward arithmetic wherever one exists. All arithmetic is f32. Nothing here uses float
// atomics: per-edge results are STORED (each edge has one owner), the per-centre and per-batch sums are reduced inside a
// workgroup in a fixed order, and the per-point sum is gathered through the transposed neighbour list in a fixed order
// (mccnn_edge_grad_reduce) -- two backward passes give bit-identical gradients.
#include "common.h"

namespace mccnn {
namespace {

constexpr int kRowsPerBlock = 4;     // conv_bwd_points: one wave per centre row
constexpr int kPdfTile = 1024;       // pdf_bwd_points: neighbour points staged in LDS per pass
constexpr int kReduceLanes = 16;     // edge_grad_reduce: lanes per point

__device__ __forceinline__ float feat_at(const float* __restrict__ f, size_t i) { return f[i]; }
__device__ __forceinline__ float feat_at(const unsigned short* __restrict__ f, size_t i) {
    return __uint_as_float(((unsigned)f[i]) << 16);   // bf16 storage -> f32
}

__device__ __forceinline__ float wave_sum(float v) {
    // butterfly over the 64 lanes: the same order on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per centre row i, lanes over the row's edges. Per edge (j, i) and block q of the kernel MLP (flat layouts:
// w1[nu*3+d], w2/w3[q*64 + out*8 + in]):
//   u_nu   = g[i, fo(nu)] f[j, fin(nu)] / (pdf K)          (0 for padded neurons)
//   dpdf  -= sum_nu u_nu a3_nu / pdf
//   t3     = 1[pre2 >= 0] * W3^T u,  t4 = 1[pre1 >= 0] * W2^T t3,  ddelta += W1^T t4
// then dp_j = ddelta / R (stored per edge), dc_i -= ddelta / R, dR_b -= ddelta . delta / R.
template <bool COMBIN, typename FT>
__global__ __launch_bounds__(256) void conv_bwd_points(
    const float* __restrict__ pts, const FT* __restrict__ feats, const int* __restrict__ bids,
    const float* __restrict__ pdfs, const float* __restrict__ smp, const int* __restrict__ start,
    const int2* __restrict__ packed, const float* __restrict__ mn, const float* __restrict__ mx,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3,
    const float* __restrict__ og, int m, int e, int fin, int outF, int nb, int neuronsOut, int B, float radius,
    int scaleInv, int avg, float* __restrict__ dp, float* __restrict__ dc, float* __restrict__ dpdf,
    float* __restrict__ drow, int* __restrict__ rowb) {
    const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kRowsPerBlock + (int)(threadIdx.x >> 6));
    if (i >= m) return;
    const int lane = lane_id();
    const int e0 = start[i];
    const int e1 = (i < m - 1) ? start[i + 1] : e;
    const float K = avg ? (float)(e1 - e0) : 1.0f;
    const float cx = smp[3 * i], cy = smp[3 * i + 1], cz = smp[3 * i + 2];
    const float* __restrict__ gi = og + (size_t)i * outF;
    float sc0 = 0.f, sc1 = 0.f, sc2 = 0.f, sR = 0.f;
    for (int t = e0 + lane; t < e1; t += 64) {
        const int j = packed[t].x;
        const int b = clamp_batch(bids[j], B);
        const float R = scaleInv ? radius * max_extent(mn, mx, b) : radius;
        const float dl[3] = {(pts[3 * j] - cx) / R, (pts[3 * j + 1] - cy) / R, (pts[3 * j + 2] - cz) / R};
        const float pdf = pdfs[t];
        const float inv = 1.0f / (pdf * K);
        const FT* __restrict__ fj = feats + (size_t)j * fin;
        float dd0 = 0.f, dd1 = 0.f, dd2 = 0.f, sua = 0.f;
        for (int q = 0; q < nb; ++q) {
            const int off = q * MCCNN_MLP;
            const float* __restrict__ W2 = w2 + q * 64;
            const float* __restrict__ W3 = w3 + q * 64;
            float pre1[8], h1[8], pre2[8], h2[8], u[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float* __restrict__ W1 = w1 + (off + k) * 3;
                float s = dl[0] * W1[0];
                s = fmaf(dl[1], W1[1], s);
                s = fmaf(dl[2], W1[2], s);
                pre1[k] = s + b1[off + k];
                h1[k] = fmaxf(pre1[k], 0.0f);
            }
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) s = fmaf(h1[k], W2[o * 8 + k], s);
                pre2[o] = s + b2[off + o];
                h2[o] = fmaxf(pre2[o], 0.0f);
            }
            // the neuron -> (input feature, output feature) map of this block
            int fi = COMBIN ? off % fin : off;
            int fo = COMBIN ? off / fin : off;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const bool live = off + o < neuronsOut;
                const float x = gi[live ? fo : 0] * feat_at(fj, (size_t)(live ? fi : 0)) * inv;  // (padded: no read past a row)
                u[o] = live ? x : 0.0f;
                if (dpdf) {
                    float a = 0.0f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) a = fmaf(h2[k], W3[o * 8 + k], a);
                    a = a + b3[off + o];
                    sua = fmaf(u[o], a, sua);
                }
                if (COMBIN) {
                    if (++fi == fin) { fi = 0; ++fo; }
                } else {
                    ++fi;
                    ++fo;
                }
            }
            float t3[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float s = 0.0f;
#pragma unroll
                for (int o = 0; o < 8; ++o) s = fmaf(W3[o * 8 + k], u[o], s);
                t3[k] = pre2[k] >= 0.0f ? s : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float s = 0.0f;
#pragma unroll
                for (int o = 0; o < 8; ++o) s = fmaf(W2[o * 8 + k], t3[o], s);
                const float t4 = pre1[k] >= 0.0f ? s : 0.0f;
                const float* __restrict__ W1 = w1 + (off + k) * 3;
                dd0 = fmaf(W1[0], t4, dd0);
                dd1 = fmaf(W1[1], t4, dd1);
                dd2 = fmaf(W1[2], t4, dd2);
            }
        }
        const float g0 = dd0 / R, g1 = dd1 / R, g2 = dd2 / R;
        dp[3 * (size_t)t] = g0;
        dp[3 * (size_t)t + 1] = g1;
        dp[3 * (size_t)t + 2] = g2;
        if (dpdf) dpdf[t] = -sua / pdf;
        sc0 -= g0;
        sc1 -= g1;
        sc2 -= g2;
        sR -= g0 * dl[0] + g1 * dl[1] + g2 * dl[2];
    }
    sc0 = wave_sum(sc0);
    sc1 = wave_sum(sc1);
    sc2 = wave_sum(sc2);
    sR = wave_sum(sR);
    if (lane == 0) {
        dc[3 * (size_t)i] = sc0;
        dc[3 * (size_t)i + 1] = sc1;
        dc[3 * (size_t)i + 2] = sc2;
        if (drow) {
            drow[i] = sR;
            rowb[i] = e1 > e0 ? clamp_batch(bids[packed[e0].x], B) : 0;
        }
    }
}

// One workgroup per centre row i of the KDE (k = row length, h = window, s = 1 / (R h)):
//   pdf_t = (1/k) sum_{t' in row} g(p_j' - p_j),  g(D) = (0.39894228 / h)^3 exp(-s^2 |D|^2 / 2)
// With c = dpdf_t g / k, the pair (t, t') adds c s^2 D to slot t, -c s^2 D to slot t' and c s^2 |D|^2 / R to dR_b. Each
// slot sums its own terms (as t and as t'), so every slot has one writer.
__global__ __launch_bounds__(256) void pdf_bwd_points(
    const float* __restrict__ pts, const int* __restrict__ bids, const int* __restrict__ start,
    const int2* __restrict__ packed, int m, int e, const float* __restrict__ mn, const float* __restrict__ mx, int B,
    float window, float radius, int scaleInv, const float* __restrict__ gpdf, int accumulate, float* __restrict__ dp,
    float* __restrict__ drow, int* __restrict__ rowb) {
    __shared__ float sx[kPdfTile], sy[kPdfTile], sz[kPdfTile], ss[kPdfTile], sw[kPdfTile];
    __shared__ float red[256];
    const int i = blockIdx.x;
    const int tid = threadIdx.x;
    const int e0 = start[i];
    const int e1 = (i < m - 1) ? start[i + 1] : e;
    const float invK = 1.0f / (float)max(e1 - e0, 1);
    const float invH = 1.0f / window;
    const float c0 = 0.39894228f * invH;
    const float C3 = c0 * c0 * c0;
    float accR = 0.0f;
    for (int base = e0; base < e1; base += 256) {
        const int t = base + tid;
        const bool act = t < e1;
        float px = 0.f, py = 0.f, pz = 0.f, s = 0.f, w = 0.f, R = 1.f;
        if (act) {
            const int j = packed[t].x;
            px = pts[3 * j];
            py = pts[3 * j + 1];
            pz = pts[3 * j + 2];
            R = scaleInv ? radius * max_extent(mn, mx, clamp_batch(bids[j], B)) : radius;
            s = 1.0f / (R * window);
            w = gpdf[t] * invK;
        }
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, aR = 0.f;
        for (int tb = e0; tb < e1; tb += kPdfTile) {
            const int cnt = min(kPdfTile, e1 - tb);
            __syncthreads();
            for (int k = tid; k < cnt; k += 256) {
                const int j = packed[tb + k].x;
                const float Rk = scaleInv ? radius * max_extent(mn, mx, clamp_batch(bids[j], B)) : radius;
                sx[k] = pts[3 * j];
                sy[k] = pts[3 * j + 1];
                sz[k] = pts[3 * j + 2];
                ss[k] = 1.0f / (Rk * window);
                sw[k] = gpdf[tb + k] * invK;
            }
            __syncthreads();
            if (act) {
                const float s2 = s * s;
                for (int k = 0; k < cnt; ++k) {
                    const float dx = sx[k] - px, dy = sy[k] - py, dz = sz[k] - pz;
                    const float d2 = dx * dx + dy * dy + dz * dz;
                    const float gA = C3 * expf(-0.5f * s2 * d2);               // pdf_t's term (scale of slot t)
                    const float sk2 = ss[k] * ss[k];
                    const float gB = sk2 == s2 ? gA : C3 * expf(-0.5f * sk2 * d2);  // pdf_t''s term
                    const float cA = w * gA * s2;
                    const float c = cA + sw[k] * gB * sk2;
                    a0 = fmaf(c, dx, a0);
                    a1 = fmaf(c, dy, a1);
                    a2 = fmaf(c, dz, a2);
                    aR = fmaf(cA, d2, aR);
                }
            }
        }
        if (act) {
            float* o = dp + 3 * (size_t)t;
            if (accumulate) {
                o[0] += a0;
                o[1] += a1;
                o[2] += a2;
            } else {
                o[0] = a0;
                o[1] = a1;
                o[2] = a2;
            }
            accR += aR / R;
        }
    }
    if (drow) {
        red[tid] = accR;
        __syncthreads();
#pragma unroll
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            drow[i] = red[0];
            rowb[i] = e1 > e0 ? clamp_batch(bids[packed[e0].x], B) : 0;
        }
    }
}

// dR[b] = sum of the per-row values of batch b, one workgroup per batch, fixed order
__global__ __launch_bounds__(256) void batch_sum(const float* __restrict__ drow, const int* __restrict__ rowb, int m,
                                                 float* __restrict__ dR) {
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float s = 0.0f;
    for (int r = tid; r < m; r += 256)
        if (rowb[r] == b) s += drow[r];
    red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) dR[b] = red[0];
}

// dpts[j] = sum of dp[t] over the edges whose neighbour is j, in transposed-list order; 16 lanes per point
__global__ __launch_bounds__(256) void edge_grad_reduce(const float* __restrict__ dp, const int* __restrict__ startT,
                                                        const int* __restrict__ permT, int n, float* __restrict__ out) {
    const int j = (int)((blockIdx.x * 256u + threadIdx.x) / kReduceLanes);
    const int l = (int)(threadIdx.x % kReduceLanes);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    const bool act = j < n;
    if (act) {
        const int k1 = startT[j + 1];
        for (int k = startT[j] + l; k < k1; k += kReduceLanes) {
            const size_t t = (size_t)permT[k];
            s0 += dp[3 * t];
            s1 += dp[3 * t + 1];
            s2 += dp[3 * t + 2];
        }
    }
#pragma unroll
    for (int o = kReduceLanes / 2; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, kReduceLanes);
        s1 += __shfl_xor(s1, o, kReduceLanes);
        s2 += __shfl_xor(s2, o, kReduceLanes);
    }
    if (act && l == 0) {
        out[3 * (size_t)j] = s0;
        out[3 * (size_t)j + 1] = s1;
        out[3 * (size_t)j + 2] = s2;
    }
}

size_t rows_ws_bytes(int m) { return 2 * align_up((size_t)(m > 0 ? m : 1) * 4) + 256; }

}  // namespace
}  // namespace mccnn

using namespace mccnn;

extern "C" {

size_t mccnn_spatial_conv_bwd_points_workspace_bytes(int m, int batch_size) {
    (void)batch_size;
    return rows_ws_bytes(m);
}

int mccnn_spatial_conv_bwd_points(const float* sorted_pts, const void* sorted_feats, int feats_bf16,
                                  const int* sorted_batch_ids, const float* pdfs, const float* samples,
                                  const int* start_idx, const int* packed, const float* aabb_min, const float* aabb_max,
                                  const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                  const float* b3, const float* out_grad, int n, int m, int e, int num_in_feats,
                                  int num_out_feats, int combin, int batch_size, float radius, int scale_inv, int avg,
                                  float* dpts_edge, float* dsamples, float* dpdfs, float* dradius, void* ws,
                                  size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 0 || m < 0 || e < 0 || num_in_feats <= 0 || num_out_feats <= 0 || batch_size <= 0 || !(radius > 0.0f))
        return MCCNN_E_BADARG;
    if (dradius && !scale_inv) return MCCNN_E_BADARG;
    if (m == 0 && !dradius) return 0;
    if ((m > 0 && !dsamples) || (e > 0 && (!sorted_pts || !sorted_feats || !sorted_batch_ids || !pdfs || !packed || !dpts_edge ||
                                !w1 || !b1 || !w2 || !b2 || !w3 || !b3)) || (m > 0 && (!samples || !start_idx || !out_grad)))
        return MCCNN_E_BADARG;
    if (scale_inv && (!aabb_min || !aabb_max)) return MCCNN_E_BADARG;
    if (!combin && num_in_feats != num_out_feats) return MCCNN_E_SHAPE;
    if (feats_bf16 && (combin || (num_in_feats & 1))) return MCCNN_E_SHAPE;
    const long long neurons = combin ? (long long)num_in_feats * num_out_feats : num_in_feats;
    if (neurons > (1 << 28)) return MCCNN_E_TOOLARGE;
    const int nb = (int)((neurons + MCCNN_MLP - 1) / MCCNN_MLP);
    const int outF = combin ? num_out_feats : num_in_feats;
    hipStream_t s = (hipStream_t)stream;
    float* drow = nullptr;
    int* rowb = nullptr;
    if (dradius) {
        if (!ws || ws_bytes < mccnn_spatial_conv_bwd_points_workspace_bytes(m, batch_size)) return MCCNN_E_WORKSPACE;
        Arena ar(ws, ws_bytes);
        drow = ar.take<float>((size_t)(m > 0 ? m : 1));
        rowb = ar.take<int>((size_t)(m > 0 ? m : 1));
        if (!drow || !rowb) return MCCNN_E_WORKSPACE;
    }
    if (m > 0) {
        const int2* pk = reinterpret_cast<const int2*>(packed);
        const dim3 grid(ceil_div(m, kRowsPerBlock)), blk(256);
        if (feats_bf16) {
            conv_bwd_points<false, unsigned short><<<grid, blk, 0, s>>>(
                sorted_pts, (const unsigned short*)sorted_feats, sorted_batch_ids, pdfs, samples, start_idx, pk, aabb_min,
                aabb_max, w1, b1, w2, b2, w3, b3, out_grad, m, e, num_in_feats, outF, nb, (int)neurons, batch_size, radius,
                scale_inv, avg, dpts_edge, dsamples, dpdfs, drow, rowb);
        } else if (combin) {
            conv_bwd_points<true, float><<<grid, blk, 0, s>>>(
                sorted_pts, (const float*)sorted_feats, sorted_batch_ids, pdfs, samples, start_idx, pk, aabb_min, aabb_max,
                w1, b1, w2, b2, w3, b3, out_grad, m, e, num_in_feats, outF, nb, (int)neurons, batch_size, radius,
                scale_inv, avg, dpts_edge, dsamples, dpdfs, drow, rowb);
        } else {
            conv_bwd_points<false, float><<<grid, blk, 0, s>>>(
                sorted_pts, (const float*)sorted_feats, sorted_batch_ids, pdfs, samples, start_idx, pk, aabb_min, aabb_max,
                w1, b1, w2, b2, w3, b3, out_grad, m, e, num_in_feats, outF, nb, (int)neurons, batch_size, radius,
                scale_inv, avg, dpts_edge, dsamples, dpdfs, drow, rowb);
        }
        MCCNN_LAUNCHED();
    }
    if (dradius) {
        batch_sum<<<batch_size, 256, 0, s>>>(drow, rowb, m, dradius);
        MCCNN_LAUNCHED();
    }
    return 0;
}

size_t mccnn_compute_pdf_bwd_points_workspace_bytes(int m, int batch_size) {
    (void)batch_size;
    return rows_ws_bytes(m);
}

int mccnn_compute_pdf_bwd_points(const float* sorted_pts, const int* sorted_batch_ids, const int* start_idx, int m,
                                 const int* packed, int e, const float* aabb_min, const float* aabb_max, int batch_size,
                                 float window, float radius, int scale_inv, const float* pdf_grad, int accumulate,
                                 float* dpts_edge, float* dradius, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (m < 0 || e < 0 || batch_size <= 0 || !(radius > 0.0f) || !(window > 0.0f)) return MCCNN_E_BADARG;
    if (dradius && !scale_inv) return MCCNN_E_BADARG;
    if (m == 0 && !dradius) return 0;
    if (m > 0 && (!start_idx || (e > 0 && (!sorted_pts || !sorted_batch_ids || !packed || !pdf_grad || !dpts_edge))))
        return MCCNN_E_BADARG;
    if (scale_inv && (!aabb_min || !aabb_max)) return MCCNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    float* drow = nullptr;
    int* rowb = nullptr;
    if (dradius) {
        if (!ws || ws_bytes < mccnn_compute_pdf_bwd_points_workspace_bytes(m, batch_size)) return MCCNN_E_WORKSPACE;
        Arena ar(ws, ws_bytes);
        drow = ar.take<float>((size_t)(m > 0 ? m : 1));
        rowb = ar.take<int>((size_t)(m > 0 ? m : 1));
        if (!drow || !rowb) return MCCNN_E_WORKSPACE;
    }
    if (m > 0) {
        pdf_bwd_points<<<m, 256, 0, s>>>(sorted_pts, sorted_batch_ids, start_idx, reinterpret_cast<const int2*>(packed), m, e,
                                         aabb_min, aabb_max, batch_size, window, radius, scale_inv, pdf_grad, accumulate,
                                         dpts_edge, drow, rowb);
        MCCNN_LAUNCHED();
    }
    if (dradius) {
        batch_sum<<<batch_size, 256, 0, s>>>(drow, rowb, m, dradius);
        MCCNN_LAUNCHED();
    }
    return 0;
}

int mccnn_edge_grad_reduce(const float* dpts_edge, const int* start_t, const int* perm_t, int n, int e, float* dpts,
                           mccnn_stream_t stream) {
    if (n < 0 || e < 0 || (n > 0 && (!start_t || !dpts)) || (e > 0 && (!dpts_edge || !perm_t))) return MCCNN_E_BADARG;
    if (n == 0) return 0;
    const long long threads = (long long)n * kReduceLanes;
    edge_grad_reduce<<<(int)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(dpts_edge, start_t, perm_t, n, dpts);
    MCCNN_LAUNCHED();
    return 0;
}

}  // extern "C"
