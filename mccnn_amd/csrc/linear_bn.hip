// A linear layer and the dense glue behind it as one op (mccnn_linear_bn_act_fwd / _bwd): z = x W + b, y = drop(act(bn(z)))
// with x [n, cin], W [cin, cout] float32 row-major, batch statistics over the rows of z; bn, act and drop as bn_act.hip
// defines them. New here: the matmul on the f32-input matrix cores (v_mfma_f32_16x16x4_f32: exact f32, one fmaf chain over k
// per element) and what it folds in.
//
// One GEMM body (lin_tile, in lin_tile.h: linear_xent.hip shares it) for a 64 x 64 output tile of a workgroup of 4 waves: A and B go through LDS in chunks of 32 k,
// either operand read as stored or transposed, rows and columns past the edge padded with zeros; wave w owns rows
// 16 w .. 16 w + 15 of the tile in four 16 x 16 accumulators. The k order of an element is fixed and does not depend on
// the other rows of the call.
//   forward, training   launch 1: a workgroup per (column tile, slab of bn_slab_rows(n) rows) walks its slab 64 rows at a
//                                 time; the epilogue adds b, stores z and keeps per lane the sums of what it stored, shifted
//                                 by an anchor K (the lane's own first value: no cancellation when |mean| >> std). A mean is
//                                 carried as the pair K + q, K an exact value of the column and q of the size of its std: z has
//                                 columns with |mean| of hundreds of std, where one f32 for the mean would cost xhat several
//                                 1e-5 of its scale. The 16 lane groups of a column are merged by Chan's rule in a fixed
//                                 order (the anchor of the first stays, only q moves) into the slab's partial
//                                 (count, K, q, M2).
//                       launch 2: lin_apply_k merges the partials of its columns in slab order, writes saved -- the mean
//                                 m = fl(K + q), rstd and the remainder c = (K - m) + q -- and the moving statistics from
//                                 slab 0, and normalises z as ((z - m) - c) * rstd, which is what the backward recomputes.
//                       one slab (n <= 256): the workgroup that made z and its statistics applies them itself. One launch.
//   eval                one launch: the epilogue normalises with the moving statistics and stores y alone.
//   backward            bn_act's backward over z writes dz into the workspace (two launches, one up to 256 rows);
//                       dx = dz W^T is the GEMM body with W read transposed; dW = x^T dz is the body with x read transposed,
//                       split over row slabs into partial planes, db = the column sums of the dz chunks the first row of
//                       workgroups has in LDS anyway; one more launch adds the planes in slab order (none for one slab).
// No atomics, no memset, fixed merge orders: the same inputs and seed give the same bytes.
#include "common.h"
#include "bn_drop.h"
#include "bn_act.h"
#include "lin_tile.h"

namespace mccnn {

struct LinFwdArgs {
    const float* x;
    const float* w;
    const float* b;
    float* z;          // training
    float* part;       // training, more than one slab: planes count, K, q, M2 of [slabs, cout]
    void* y;
    const float* gamma;
    const float* beta;
    float* mov_mean;
    float* mov_var;
    float* saved;      // training: [3, cout]: mean, rstd, what the exact mean has over that f32 mean
    int n, cin, cout, slab_rows, slabs, relu, y_bf16;
    float momentum, eps, keep_scale;
    unsigned seed;
    unsigned long long T;
};

// Chan's merge of (nB, KB + qB, mB) into (nA, KA + qA, mA): A's anchor stays
__device__ __forceinline__ void lin_chan(float& nA, float& KA, float& qA, float& mA, float nB, float KB, float qB, float mB) {
    if (nB == 0.f) return;
    if (nA == 0.f) { nA = nB; KA = KB; qA = qB; mA = mB; return; }
    const float n = nA + nB, f = nB / n, w = nA * f;
    const float d = (KB - KA) + (qB - qA);
    qA = qA + d * f;
    mA = mA + mB + d * d * w;
    nA = n;
}

__device__ __forceinline__ void lin_store_y(const LinFwdArgs& a, size_t at, float v) {
    if (a.y_bf16) static_cast<uint16_t*>(a.y)[at] = (uint16_t)(f32x2_to_bf16(v, 0.f) & 0xffffu);
    else static_cast<float*>(a.y)[at] = v;
}

// from the merged (n, K + q, M2) of column c0 + tid (tid < 64): the mean as m = fl(K + q) and the remainder c = (K - m) + q,
// rstd, and when `first` saved = [m; rstd; c] and the moving statistics; m, c and rstd into st[3][64] for the workgroup.
// Every thread calls it (a barrier at the end).
__device__ __forceinline__ void lin_finish_stats(const LinFwdArgs& a, int c0, float K, float q, float m2, bool first, float* st) {
    const int tid = (int)threadIdx.x;
    if (tid < kLinTile && c0 + tid < a.cout) {
        const int j = c0 + tid;
        const float var = m2 / (float)a.n;
        const float rstd = 1.0f / sqrtf(var + a.eps);
        const float mean = K + q, c = (K - mean) + q;
        st[tid] = mean;
        st[kLinTile + tid] = c;
        st[2 * kLinTile + tid] = rstd;
        if (first) {
            const float keep = 1.0f - a.momentum;
            a.saved[j] = mean;
            a.saved[(size_t)a.cout + j] = rstd;
            a.saved[2 * (size_t)a.cout + j] = c;
            a.mov_mean[j] = a.mov_mean[j] * a.momentum + mean * keep;
            a.mov_var[j] = a.mov_var[j] * a.momentum + var * keep;
        }
    }
    __syncthreads();
}

// y = drop(act(((z - m) - c) * rstd * gamma + beta)), bn_act.hip's backward arithmetic operand for operand, over rows [row0, row1) of columns c0 .. c0 + 63: thread tid has column
// tid & 63 and rows row0 + (tid >> 6), + 4, ...
__device__ __forceinline__ void lin_apply_rows(const LinFwdArgs& a, int c0, int row0, int row1, const float* st) {
    const int tid = (int)threadIdx.x, cx = tid & 63, ry = tid >> 6, col = c0 + cx;
    if (col >= a.cout) return;   // (no barrier follows)
    const float m = st[cx], c = st[kLinTile + cx], rstd = st[2 * kLinTile + cx], g = a.gamma[col], be = a.beta[col];
    const bool drop = a.T < kBnDropAll;
    constexpr int U = 4;
    for (int r = row0 + ry; r < row1; r += 4 * U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (r + 4 * u < row1) v[u] = a.z[(size_t)(r + 4 * u) * a.cout + col];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ru = r + 4 * u;
            if (ru >= row1) break;
            const float xh = ((v[u] - m) - c) * rstd;
            const float pre = xh * g + be;
            float act = a.relu ? (pre > 0.f ? pre : 0.f) : pre;
            if (drop) act = bn_drop_keep(bn_drop_row(a.seed, ru), (uint32_t)col, a.T) ? act * a.keep_scale : 0.f;
            lin_store_y(a, (size_t)ru * a.cout + col, act);
        }
    }
}

// TRAIN 1: z, the slab's statistics, and with one slab y as well; 0: eval, y alone
template <bool AV, int TRAIN>
__global__ __launch_bounds__(kLinThreads) void lin_fwd_k(LinFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float as[kLinTile * kLinAS];
    __shared__ __attribute__((aligned(16))) float bs[kLinKC * kLinBS];
    __shared__ float red[TRAIN ? 4 * 16 * kLinTile : 1];
    __shared__ float st[TRAIN ? 3 * kLinTile : 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)blockIdx.x * kLinTile, slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    int col[4];
    bool cok[4];
    float bias[4], mean[4], rstd[4], g[4], be[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        col[t] = c0 + t * 16 + (lane & 15);
        cok[t] = col[t] < a.cout;
        bias[t] = cok[t] ? a.b[col[t]] : 0.f;
        if constexpr (!TRAIN) {
            mean[t] = cok[t] ? a.mov_mean[col[t]] : 0.f;
            rstd[t] = cok[t] ? 1.0f / sqrtf(a.mov_var[col[t]] + a.eps) : 0.f;
            g[t] = cok[t] ? a.gamma[col[t]] : 0.f;
            be[t] = cok[t] ? a.beta[col[t]] : 0.f;
        }
    }
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, K[4] = {0.f, 0.f, 0.f, 0.f};
    int rows = 0;
    for (int m0 = row0; m0 < row1; m0 += kLinTile) {
        lin_f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = lin_f32x4{0.f, 0.f, 0.f, 0.f};
        lin_tile<false, false, AV>(a.x, a.cin, a.w, a.cout, row1, a.cout, m0, c0, 0, a.cin, as, bs, acc, [](int) {});
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + wave * 16 + 4 * (lane >> 4) + i;
            if (row >= row1) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float v = acc[t][i] + bias[t];
                if constexpr (TRAIN) {
                    if (cok[t]) a.z[(size_t)row * a.cout + col[t]] = v;
                    if (rows == 0) K[t] = v;
                    const float d = v - K[t];
                    s1[t] = s1[t] + d;
                    s2[t] = s2[t] + d * d;
                } else {
                    const float xh = (v - mean[t]) * rstd[t];
                    const float pre = xh * g[t] + be[t];
                    const float act = a.relu ? (pre > 0.f ? pre : 0.f) : pre;
                    if (cok[t]) lin_store_y(a, (size_t)row * a.cout + col[t], act);
                }
            }
            ++rows;
        }
    }
    if constexpr (TRAIN) {
        // the 16 lane groups (wave, lane >> 4) of a column, each with its own rows: Chan's merge in group order
        const int grp = wave * 4 + (lane >> 4);
        const float cnt = (float)rows;
        constexpr int P = 16 * kLinTile;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float q = rows ? s1[t] / cnt : 0.f;
            const int at = grp * kLinTile + t * 16 + (lane & 15);
            red[at] = cnt;
            red[P + at] = K[t];
            red[2 * P + at] = q;
            red[3 * P + at] = fmaxf(s2[t] - s1[t] * q, 0.f);
        }
        __syncthreads();
        float nA = 0.f, KA = 0.f, qA = 0.f, mA = 0.f;
        if (tid < kLinTile && c0 + tid < a.cout) {
            for (int gi = 0; gi < 16; ++gi) {
                const int at = gi * kLinTile + tid;
                lin_chan(nA, KA, qA, mA, red[at], red[P + at], red[2 * P + at], red[3 * P + at]);
            }
            if (a.slabs > 1) {
                const size_t plane = (size_t)a.slabs * a.cout;
                float* p = a.part + (size_t)slab * a.cout + c0 + tid;
                p[0] = nA;
                p[plane] = KA;
                p[2 * plane] = qA;
                p[3 * plane] = mA;
            }
        }
        if (a.slabs == 1) {
            // (__syncthreads inside: the workgroup's own stores of z are visible to all its threads behind it)
            lin_finish_stats(a, c0, KA, qA, mA, true, st);
            lin_apply_rows(a, c0, row0, row1, st);
        }
    }
}

// forward, training, launch 2 (more than one slab): grid (column tiles, slabs)
__global__ __launch_bounds__(kLinThreads) void lin_apply_k(LinFwdArgs a) {
    __shared__ float st[3 * kLinTile];
    const int tid = (int)threadIdx.x;
    const int c0 = (int)blockIdx.x * kLinTile, slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float nA = 0.f, KA = 0.f, qA = 0.f, mA = 0.f;
    if (tid < kLinTile && c0 + tid < a.cout) {
        const size_t plane = (size_t)a.slabs * a.cout;
        for (int s = 0; s < a.slabs; ++s) {
            const float* p = a.part + (size_t)s * a.cout + c0 + tid;
            lin_chan(nA, KA, qA, mA, p[0], p[plane], p[2 * plane], p[3 * plane]);
        }
    }
    lin_finish_stats(a, c0, KA, qA, mA, slab == 0, st);
    lin_apply_rows(a, c0, row0, row1, st);
}

inline size_t lin_stats_bytes(int n, int cout) {
    const int slabs = ceil_div(n, bn_slab_rows(n));
    if (slabs == 1) return 0;
    return align_up((size_t)4 * (size_t)slabs * (size_t)cout * sizeof(float));
}

template <int TRAIN>
inline int lin_fwd_launch(bool av, dim3 grid, hipStream_t st, const LinFwdArgs& a) {
    if (av) lin_fwd_k<true, TRAIN><<<grid, kLinThreads, 0, st>>>(a);
    else lin_fwd_k<false, TRAIN><<<grid, kLinThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    return 0;
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

size_t mccnn_linear_bn_act_workspace_bytes(int n, int cin, int cout) {
    if (n < 1 || cin < 1 || cout < 1 || !lin_sizes_ok(n, cin, cout)) return 0;
    // the backward's: dz, bn_act's own workspace over z, the dW / db planes; the forward's partials (four values per slab
    // and column, at most 64 slabs of at least 128 rows) fit the front of it
    return lin_dz_bytes(n, cout) + mccnn_bn_act_workspace_bytes(n, cout) + lin_dw_bytes(n, cin, cout);
}

int mccnn_linear_bn_act_fwd(const float* x, const float* w, const float* b, int n, int cin, int cout, const float* gamma,
                            const float* beta, float* moving_mean, float* moving_var, float momentum, float eps, int training,
                            int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed, float* z, void* y,
                            int y_bf16, float* saved, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || cin < 1 || cout < 1) return MCCNN_E_BADARG;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !w || !b || !gamma || !beta || !moving_mean || !moving_var || !y) return MCCNN_E_BADARG;
    if (training && (!z || !saved)) return MCCNN_E_BADARG;
    if (y_bf16 & ~1) return MCCNN_E_BADARG;
    if (y_bf16 && (cout % 2 != 0 || ((uintptr_t)y & 3u) != 0)) return MCCNN_E_SHAPE;
    if (!lin_sizes_ok(n, cin, cout)) return MCCNN_E_TOOLARGE;
    const size_t need = training ? lin_stats_bytes(n, cout) : 0;
    if (need && (!ws || ws_bytes < need)) return MCCNN_E_WORKSPACE;
    LinFwdArgs a = {};
    a.x = x; a.w = w; a.b = b; a.z = z; a.part = (float*)ws; a.y = y; a.gamma = gamma; a.beta = beta;
    a.mov_mean = moving_mean; a.mov_var = moving_var; a.saved = saved;
    a.n = n; a.cin = cin; a.cout = cout; a.relu = relu ? 1 : 0; a.y_bf16 = y_bf16;
    a.momentum = momentum; a.eps = eps; a.keep_scale = keep_scale; a.seed = seed;
    a.T = training ? keep_threshold : kBnDropAll;
    a.slab_rows = training ? bn_slab_rows(n) : kLinTile;
    a.slabs = ceil_div(n, a.slab_rows);
    const bool av = cin % 4 == 0 && lin_aligned16(x);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(cout, kLinTile), (unsigned)a.slabs);
    if (!training) return lin_fwd_launch<0>(av, grid, st, a);
    if (const int e = lin_fwd_launch<1>(av, grid, st, a)) return e;
    if (a.slabs > 1) {
        lin_apply_k<<<grid, kLinThreads, 0, st>>>(a);
        MCCNN_LAUNCHED();
    }
    return 0;
}

int mccnn_linear_bn_act_bwd(const float* x, const float* w, const float* z, const void* dy, int dy_bf16, int n, int cin, int cout,
                            const float* gamma, const float* beta, const float* saved, int relu,
                            unsigned long long keep_threshold, float keep_scale, unsigned seed, float* dx, float* dw, float* db,
                            float* dgamma, float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || cin < 1 || cout < 1) return MCCNN_E_BADARG;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !w || !z || !dy || !gamma || !beta || !saved || !dw || !db || !dgamma || !dbeta) return MCCNN_E_BADARG;
    if (dy_bf16 & ~1) return MCCNN_E_BADARG;
    if (dy_bf16 && (cout % 2 != 0 || ((uintptr_t)dy & 3u) != 0)) return MCCNN_E_SHAPE;
    if (!lin_sizes_ok(n, cin, cout)) return MCCNN_E_TOOLARGE;
    const size_t need = mccnn_linear_bn_act_workspace_bytes(n, cin, cout);
    if (!ws || ws_bytes < need) return MCCNN_E_WORKSPACE;
    char* base = (char*)ws;
    float* dz = (float*)base;
    const size_t bn_bytes = mccnn_bn_act_workspace_bytes(n, cout);
    void* bn_ws = base + lin_dz_bytes(n, cout);
    float* planes = (float*)(base + lin_dz_bytes(n, cout) + bn_bytes);
    hipStream_t st = (hipStream_t)stream;
    if (const int e = bn_act_bwd_impl(z, 0, dy, dy_bf16, n, cout, gamma, beta, saved, saved + 2 * (size_t)cout, relu, keep_threshold,
                                      keep_scale, seed, dz, dgamma, dbeta, bn_ws, bn_bytes, stream))
        return e;
    if (dx) {
        LinMmArgs a = {};
        a.a = dz; a.lda = cout; a.b = w; a.ldb = cout; a.out = dx; a.M = n; a.N = cin; a.K = cout; a.kper = cout;
        const dim3 grid((unsigned)ceil_div(cin, kLinTile), (unsigned)ceil_div(n, kLinTile), 1);
        if (cout % 4 == 0 && lin_aligned16(dz)) lin_mm_k<false, true, true, false><<<grid, kLinThreads, 0, st>>>(a);
        else lin_mm_k<false, true, false, false><<<grid, kLinThreads, 0, st>>>(a);
        MCCNN_LAUNCHED();
    }
    const LinDwPlan p = lin_dw_plan(n, cin, cout);
    const int wn = cin * cout;
    LinMmArgs a = {};
    a.a = x; a.lda = cin; a.b = dz; a.ldb = cout; a.M = cin; a.N = cout; a.K = n; a.kper = p.kper; a.plane = (size_t)wn;
    a.out = p.slabs == 1 ? dw : planes;
    a.colsum = p.slabs == 1 ? db : planes + (size_t)p.slabs * wn;
    const dim3 grid((unsigned)ceil_div(cout, kLinTile), (unsigned)ceil_div(cin, kLinTile), (unsigned)p.slabs);
    lin_mm_k<true, false, false, true><<<grid, kLinThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    if (p.slabs > 1) {
        lin_dw_merge_k<<<(unsigned)ceil_div((long long)wn + cout, kLinThreads), kLinThreads, 0, st>>>(
            planes, planes + (size_t)p.slabs * wn, dw, db, wn, cout, p.slabs);
        MCCNN_LAUNCHED();
    }
    return 0;
}

}  // extern "C"
