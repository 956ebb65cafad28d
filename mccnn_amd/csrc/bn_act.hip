// The dense glue between two MC convolutions as one op (mccnn_bn_act_fwd / _bwd): y = drop(act(bn(x))) over an [n, c]
// float32 row-major tensor, batch statistics over the rows.
//
// A workgroup of 256 threads owns a tile of up to 32 columns and a slab of rows: tw threads across (4 columns each when
// c % 4 == 0 and the row pointers are 16-byte aligned, one column each otherwise), 256 / tw row lanes down.
//   forward, training   launch 1: per slab and column a partial (count, mean, M2) -- per thread sums shifted by the slab's
//                                 first row (no cancellation when |mean| >> std), merged across the row lanes by Chan's
//                                 rule in a fixed tree through LDS.
//                       launch 2: every workgroup merges the partials of ITS columns itself (they are the previous launch's:
//                                 stream order is the only hand-off), then normalises, gates, drops and stores; slab 0 of a
//                                 column tile writes saved = [mean; rstd] and updates the moving statistics.
//   backward            the same two shapes with the partial (sum g, sum g * xhat, sum xhat); xhat, the gate and the mask
//                       are recomputed from x, saved and the seed.
//   n <= 256            one workgroup per column tile does both halves in ONE launch, forward and backward.
//   eval                one launch.
// No atomics, no memset, no ticket or spin-wait between workgroups; a fixed merge order: the same inputs and seed give the
// same bytes. The gate is pre > 0 (torch's relu'), not the >= 0 of the convolution kernels.
#include "common.h"
#include "bn_drop.h"

namespace mccnn {

constexpr int kBnThreads = 256;
constexpr int kBnTileCols = 32;     // columns of a workgroup: 128 bytes of a row
constexpr int kBnSmallRows = 256;   // up to here: the one-launch form
constexpr int kBnSlabRows = 128;    // rows of a slab ...
constexpr int kBnMaxSlabs = 64;     // ... until there would be more slabs than this: then the slabs grow

struct BnPlan {
    int vec, tw_log, tiles, slab_rows, slabs;
};
inline int bn_slab_rows(int n) {
    if (n <= kBnSmallRows) return n;
    if (ceil_div(n, kBnSlabRows) <= kBnMaxSlabs) return kBnSlabRows;
    return ceil_div(ceil_div(n, kBnMaxSlabs), 32) * 32;
}
inline BnPlan bn_plan(int n, int c, bool aligned16) {
    BnPlan p;
    p.vec = (c % 4 == 0 && aligned16) ? 4 : 1;
    const int units = c / p.vec, most = kBnTileCols / p.vec;
    p.tw_log = 0;
    while ((1 << p.tw_log) < most && (1 << p.tw_log) < units) ++p.tw_log;
    p.tiles = ceil_div(units, 1 << p.tw_log);
    p.slab_rows = bn_slab_rows(n);
    p.slabs = ceil_div(n, p.slab_rows);
    return p;
}

struct BnArgs {
    const float* x;
    const float* dy;
    float* out;          // y (forward) or dx (backward)
    const float* gamma;
    const float* beta;
    float* mov_mean;
    float* mov_var;
    float* saved;        // [2, c]: written by the forward, read by the backward
    float* part;         // the slab partials: planes of [slabs, c]
    float* dgamma;
    float* dbeta;
    int n, c, tw_log, slab_rows, slabs, relu, want_dx;
    float momentum, eps, keep_scale;
    unsigned seed;
    unsigned long long T;
};

struct BnCoord {
    int tid, cx, ry, R, col;
    bool ok;
};
template <int VEC>
__device__ __forceinline__ BnCoord bn_coord(const BnArgs& a) {
    BnCoord t;
    t.tid = (int)threadIdx.x;
    t.cx = t.tid & ((1 << a.tw_log) - 1);
    t.ry = t.tid >> a.tw_log;
    t.R = kBnThreads >> a.tw_log;
    const long long col = ((long long)blockIdx.x * (1 << a.tw_log) + t.cx) * VEC;
    t.ok = col < (long long)a.c;    // (VEC == 4: c % 4 == 0, so all four columns are inside)
    t.col = t.ok ? (int)col : 0;
    return t;
}

template <int VEC>
__device__ __forceinline__ void bn_ld(const float* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}
template <int VEC>
__device__ __forceinline__ void bn_st(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *p = v[0];
    }
}

// Chan's merge of (nB, mB, qB) into (nA, mA, qA); one count for the VEC columns of a thread (they share their rows)
template <int VEC>
__device__ __forceinline__ void bn_chan(float& nA, float (&mA)[VEC], float (&qA)[VEC], float nB, const float (&mB)[VEC],
                                        const float (&qB)[VEC]) {
    if (nB == 0.f) return;
    if (nA == 0.f) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) { mA[k] = mB[k]; qA[k] = qB[k]; }
        nA = nB;
        return;
    }
    const float n = nA + nB, f = nB / n, w = nA * f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float d = mB[k] - mA[k];
        mA[k] = mA[k] + d * f;
        qA[k] = qA[k] + qB[k] + d * d * w;
    }
    nA = n;
}

// the row lanes of a column merged in a fixed tree through LDS (lds: 256 * (1 + 2 * VEC) floats); the result is in the
// threads of row lane 0. Every thread of the workgroup calls it.
template <int VEC>
__device__ __forceinline__ void bn_tree_merge(const BnArgs& a, const BnCoord& t, float& cnt, float (&mean)[VEC],
                                              float (&m2)[VEC], float* lds) {
    float* lc = lds;
    float* lm = lds + kBnThreads;
    float* lq = lm + kBnThreads * VEC;
    for (int s = t.R >> 1; s >= 1; s >>= 1) {
        if (t.ry >= s && t.ry < 2 * s) {
            lc[t.tid] = cnt;
            bn_st<VEC>(lm + t.tid * VEC, mean);
            bn_st<VEC>(lq + t.tid * VEC, m2);
        }
        __syncthreads();
        if (t.ry < s) {
            const int o = t.tid + (s << a.tw_log);
            float mB[VEC], qB[VEC];
            bn_ld<VEC>(lm + o * VEC, mB);
            bn_ld<VEC>(lq + o * VEC, qB);
            bn_chan<VEC>(cnt, mean, m2, lc[o], mB, qB);
        }
        __syncthreads();
    }
}
// ... and of three plain sums (the backward's; lds: 256 * 3 * VEC floats)
template <int VEC>
__device__ __forceinline__ void bn_tree_sum(const BnArgs& a, const BnCoord& t, float (&sg)[VEC], float (&sx)[VEC],
                                            float (&sh)[VEC], float* lds) {
    float* lg = lds;
    float* lx = lds + kBnThreads * VEC;
    float* lh = lx + kBnThreads * VEC;
    for (int s = t.R >> 1; s >= 1; s >>= 1) {
        if (t.ry >= s && t.ry < 2 * s) {
            bn_st<VEC>(lg + t.tid * VEC, sg);
            bn_st<VEC>(lx + t.tid * VEC, sx);
            bn_st<VEC>(lh + t.tid * VEC, sh);
        }
        __syncthreads();
        if (t.ry < s) {
            const int o = t.tid + (s << a.tw_log);
            float gB[VEC], xB[VEC], hB[VEC];
            bn_ld<VEC>(lg + o * VEC, gB);
            bn_ld<VEC>(lx + o * VEC, xB);
            bn_ld<VEC>(lh + o * VEC, hB);
#pragma unroll
            for (int k = 0; k < VEC; ++k) { sg[k] = sg[k] + gB[k]; sx[k] = sx[k] + xB[k]; sh[k] = sh[k] + hB[k]; }
        }
        __syncthreads();
    }
}

// (count, mean, M2) of rows [row0, row1) of the thread's columns, merged over the row lanes
template <int VEC>
__device__ __forceinline__ void bn_slab_stats(const BnArgs& a, const BnCoord& t, int row0, int row1, float& cnt,
                                              float (&mean)[VEC], float (&m2)[VEC], float* lds) {
    float s1[VEC], s2[VEC], K[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { s1[k] = 0.f; s2[k] = 0.f; K[k] = 0.f; }
    int rows = 0;
    if (t.ok && row0 < row1) {
        bn_ld<VEC>(a.x + (size_t)row0 * a.c + t.col, K);   // the shift: the slab's first row
#pragma unroll 4
        for (int r = row0 + t.ry; r < row1; r += t.R) {
            float v[VEC];
            bn_ld<VEC>(a.x + (size_t)r * a.c + t.col, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float d = v[k] - K[k];
                s1[k] = s1[k] + d;
                s2[k] = s2[k] + d * d;
            }
            ++rows;
        }
    }
    cnt = (float)rows;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float q = rows ? s1[k] / cnt : 0.f;
        mean[k] = K[k] + q;
        m2[k] = fmaxf(s2[k] - s1[k] * q, 0.f);
    }
    bn_tree_merge<VEC>(a, t, cnt, mean, m2, lds);
}

// the slab partials of the thread's columns (planes count, mean, M2 of [slabs, c]), merged: slabs ry, ry + R, ... in
// order per row lane, then the tree
template <int VEC>
__device__ __forceinline__ void bn_merge_partials(const BnArgs& a, const BnCoord& t, float& cnt, float (&mean)[VEC],
                                                  float (&m2)[VEC], float* lds) {
    cnt = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) { mean[k] = 0.f; m2[k] = 0.f; }
    const size_t plane = (size_t)a.slabs * a.c;
    if (t.ok)
        for (int s = t.ry; s < a.slabs; s += t.R) {
            const float* p = a.part + (size_t)s * a.c + t.col;
            float mB[VEC], qB[VEC];
            bn_ld<VEC>(p + plane, mB);
            bn_ld<VEC>(p + 2 * plane, qB);
            bn_chan<VEC>(cnt, mean, m2, p[0], mB, qB);
        }
    bn_tree_merge<VEC>(a, t, cnt, mean, m2, lds);
}

// row lane 0: mean and rstd of the thread's columns into LDS for the workgroup; `first`: also saved and the moving statistics
template <int VEC>
__device__ __forceinline__ void bn_finish_stats(const BnArgs& a, const BnCoord& t, const float (&mean)[VEC],
                                                const float (&m2)[VEC], bool first, float (*sm)[kBnTileCols]) {
    if (t.ry == 0 && t.ok) {
        const float fn = (float)a.n, keep = 1.0f - a.momentum;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float var = m2[k] / fn;
            const float rstd = 1.0f / sqrtf(var + a.eps);
            sm[0][t.cx * VEC + k] = mean[k];
            sm[1][t.cx * VEC + k] = rstd;
            if (first) {
                const int j = t.col + k;
                a.saved[j] = mean[k];
                a.saved[(size_t)a.c + j] = rstd;
                a.mov_mean[j] = a.mov_mean[j] * a.momentum + mean[k] * keep;
                a.mov_var[j] = a.mov_var[j] * a.momentum + var * keep;
            }
        }
    }
    __syncthreads();
}

template <int VEC>
__device__ __forceinline__ void bn_apply_rows(const BnArgs& a, const BnCoord& t, int row0, int row1, const float (&mean)[VEC],
                                              const float (&rstd)[VEC], bool drop) {
    if (!t.ok) return;   // (no barrier follows)
    float g[VEC], b[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { g[k] = a.gamma[t.col + k]; b[k] = a.beta[t.col + k]; }
#pragma unroll 4
    for (int r = row0 + t.ry; r < row1; r += t.R) {
        float v[VEC], o[VEC];
        bn_ld<VEC>(a.x + (size_t)r * a.c + t.col, v);
        const uint32_t rh = drop ? bn_drop_row(a.seed, r) : 0u;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float xh = (v[k] - mean[k]) * rstd[k];
            const float pre = xh * g[k] + b[k];
            float act = a.relu ? (pre > 0.f ? pre : 0.f) : pre;
            if (drop) act = bn_drop_keep(rh, (uint32_t)(t.col + k), a.T) ? act * a.keep_scale : 0.f;
            o[k] = act;
        }
        bn_st<VEC>(a.out + (size_t)r * a.c + t.col, o);
    }
}

// forward, training, launch 1
template <int VEC>
__global__ __launch_bounds__(kBnThreads) void bn_stats_k(BnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * (1 + 2 * VEC)];
    const BnCoord t = bn_coord<VEC>(a);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float cnt, mean[VEC], m2[VEC];
    bn_slab_stats<VEC>(a, t, row0, row1, cnt, mean, m2, lds);
    if (t.ry == 0 && t.ok) {
        const size_t plane = (size_t)a.slabs * a.c;
        float* p = a.part + (size_t)slab * a.c + t.col;
        float cv[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) cv[k] = cnt;
        bn_st<VEC>(p, cv);
        bn_st<VEC>(p + plane, mean);
        bn_st<VEC>(p + 2 * plane, m2);
    }
}

// MODE 0: forward, training, launch 2 (partials from launch 1); 1: the one-launch form (n <= 256); 2: eval
template <int VEC, int MODE>
__global__ __launch_bounds__(kBnThreads) void bn_apply_k(BnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * (1 + 2 * VEC)];
    __shared__ float sm[2][kBnTileCols];
    const BnCoord t = bn_coord<VEC>(a);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float mean[VEC], rstd[VEC];
    if constexpr (MODE == 2) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            mean[k] = t.ok ? a.mov_mean[t.col + k] : 0.f;
            rstd[k] = t.ok ? 1.0f / sqrtf(a.mov_var[t.col + k] + a.eps) : 0.f;
        }
        bn_apply_rows<VEC>(a, t, row0, row1, mean, rstd, false);
    } else {
        float cnt, m2[VEC];
        if constexpr (MODE == 0) bn_merge_partials<VEC>(a, t, cnt, mean, m2, lds);
        else bn_slab_stats<VEC>(a, t, 0, a.n, cnt, mean, m2, lds);
        bn_finish_stats<VEC>(a, t, mean, m2, slab == 0, sm);
#pragma unroll
        for (int k = 0; k < VEC; ++k) { mean[k] = sm[0][t.cx * VEC + k]; rstd[k] = sm[1][t.cx * VEC + k]; }
        bn_apply_rows<VEC>(a, t, row0, row1, mean, rstd, a.T < kBnDropAll);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
template <int VEC>
struct BnCols {
    float mean[VEC], rstd[VEC], g[VEC], b[VEC];
};
template <int VEC>
__device__ __forceinline__ BnCols<VEC> bn_cols(const BnArgs& a, const BnCoord& t) {
    BnCols<VEC> q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        q.mean[k] = t.ok ? a.saved[t.col + k] : 0.f;
        q.rstd[k] = t.ok ? a.saved[(size_t)a.c + t.col + k] : 0.f;
        q.g[k] = t.ok ? a.gamma[t.col + k] : 0.f;
        q.b[k] = t.ok ? a.beta[t.col + k] : 0.f;
    }
    return q;
}
// g = dy * mask * scale * gate and xhat of row r of the thread's columns (the forward's arithmetic, operand for operand)
template <int VEC>
__device__ __forceinline__ void bn_row_grad(const BnArgs& a, const BnCoord& t, const BnCols<VEC>& q, int r, bool drop,
                                            float (&g)[VEC], float (&xh)[VEC]) {
    float v[VEC], d[VEC];
    bn_ld<VEC>(a.x + (size_t)r * a.c + t.col, v);
    bn_ld<VEC>(a.dy + (size_t)r * a.c + t.col, d);
    const uint32_t rh = drop ? bn_drop_row(a.seed, r) : 0u;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        xh[k] = (v[k] - q.mean[k]) * q.rstd[k];
        const float pre = xh[k] * q.g[k] + q.b[k];
        float w = d[k];
        if (drop) w = bn_drop_keep(rh, (uint32_t)(t.col + k), a.T) ? w * a.keep_scale : 0.f;
        if (a.relu) w = pre > 0.f ? w : 0.f;
        g[k] = w;
    }
}
template <int VEC>
__device__ __forceinline__ void bn_slab_sums(const BnArgs& a, const BnCoord& t, const BnCols<VEC>& q, int row0, int row1,
                                             float (&sg)[VEC], float (&sx)[VEC], float (&sh)[VEC], float* lds) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) { sg[k] = 0.f; sx[k] = 0.f; sh[k] = 0.f; }
    const bool drop = a.T < kBnDropAll;
    if (t.ok) {
#pragma unroll 4
        for (int r = row0 + t.ry; r < row1; r += t.R) {
            float g[VEC], xh[VEC];
            bn_row_grad<VEC>(a, t, q, r, drop, g, xh);
#pragma unroll
            for (int k = 0; k < VEC; ++k) { sg[k] = sg[k] + g[k]; sx[k] = sx[k] + g[k] * xh[k]; sh[k] = sh[k] + xh[k]; }
        }
    }
    bn_tree_sum<VEC>(a, t, sg, sx, sh, lds);
}

// backward, launch 1: the partial (sum g, sum g * xhat, sum xhat) of a slab. sum xhat is zero for the exact mean; with the
// saved f32 mean it is -n * (mean's rounding error) * rstd, and launch 2 takes that shift out of xhat again -- on a column
// of few rows with |mean| >> std (var + eps barely above var) dx is the small remainder of cancelling terms, and the
// shift alone would cost it more than 1e-4
template <int VEC>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_sums_k(BnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * 3 * VEC];
    const BnCoord t = bn_coord<VEC>(a);
    const BnCols<VEC> q = bn_cols<VEC>(a, t);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float sg[VEC], sx[VEC], sh[VEC];
    bn_slab_sums<VEC>(a, t, q, row0, row1, sg, sx, sh, lds);
    if (t.ry == 0 && t.ok) {
        const size_t plane = (size_t)a.slabs * a.c;
        float* p = a.part + (size_t)slab * a.c + t.col;
        bn_st<VEC>(p, sg);
        bn_st<VEC>(p + plane, sx);
        bn_st<VEC>(p + 2 * plane, sh);
    }
}

// backward, launch 2 (SMALL = 0: partials from launch 1, merged per workgroup) or the one-launch form (SMALL = 1): dgamma and
// dbeta from slab 0, dx when wanted (without it the grid is one slab deep: the merge alone, in the same order)
template <int VEC, int SMALL>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_dx_k(BnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * 3 * VEC];
    __shared__ float sm[3][kBnTileCols];
    const BnCoord t = bn_coord<VEC>(a);
    const BnCols<VEC> q = bn_cols<VEC>(a, t);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float sg[VEC], sx[VEC], sh[VEC];
    if constexpr (SMALL) {
        bn_slab_sums<VEC>(a, t, q, 0, a.n, sg, sx, sh, lds);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) { sg[k] = 0.f; sx[k] = 0.f; sh[k] = 0.f; }
        const size_t plane = (size_t)a.slabs * a.c;
        if (t.ok)
            for (int s = t.ry; s < a.slabs; s += t.R) {
                const float* p = a.part + (size_t)s * a.c + t.col;
                float gB[VEC], xB[VEC], hB[VEC];
                bn_ld<VEC>(p, gB);
                bn_ld<VEC>(p + plane, xB);
                bn_ld<VEC>(p + 2 * plane, hB);
#pragma unroll
                for (int k = 0; k < VEC; ++k) { sg[k] = sg[k] + gB[k]; sx[k] = sx[k] + xB[k]; sh[k] = sh[k] + hB[k]; }
            }
        bn_tree_sum<VEC>(a, t, sg, sx, sh, lds);
    }
    const float fn = (float)a.n;
    if (t.ry == 0 && t.ok) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float mh = sh[k] / fn;               // the mean of xhat: the saved mean's rounding error, in xhat units
            const float dg = sx[k] - mh * sg[k];       // sum g * (xhat - mh)
            sm[0][t.cx * VEC + k] = sg[k];
            sm[1][t.cx * VEC + k] = dg;
            sm[2][t.cx * VEC + k] = mh;
            if (slab == 0) {
                a.dbeta[t.col + k] = sg[k];
                a.dgamma[t.col + k] = dg;
            }
        }
    }
    __syncthreads();
    if (!a.want_dx || !t.ok) return;
    const bool drop = a.T < kBnDropAll;
    float kb[VEC], kg[VEC], gr[VEC], mh[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        kb[k] = sm[0][t.cx * VEC + k] / fn;
        kg[k] = sm[1][t.cx * VEC + k] / fn;
        mh[k] = sm[2][t.cx * VEC + k];
        gr[k] = q.g[k] * q.rstd[k];
    }
#pragma unroll 4
    for (int r = row0 + t.ry; r < row1; r += t.R) {
        float g[VEC], xh[VEC], o[VEC];
        bn_row_grad<VEC>(a, t, q, r, drop, g, xh);
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = gr[k] * (g[k] - kb[k] - (xh[k] - mh[k]) * kg[k]);
        bn_st<VEC>(a.out + (size_t)r * a.c + t.col, o);
    }
}

inline bool bn_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace mccnn

using namespace mccnn;

extern "C" {

size_t mccnn_bn_act_workspace_bytes(int n, int c) {
    if (n < 1 || c < 1 || n <= kBnSmallRows) return 0;
    return align_up((size_t)3 * (size_t)ceil_div(n, bn_slab_rows(n)) * (size_t)c * sizeof(float));
}

int mccnn_bn_act_fwd(const float* x, int n, int c, const float* gamma, const float* beta, float* moving_mean,
                     float* moving_var, float momentum, float eps, int training, int relu,
                     unsigned long long keep_threshold, float keep_scale, unsigned seed, float* y, float* saved, void* ws,
                     size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || c < 1) return MCCNN_E_BADARG;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !gamma || !beta || !moving_mean || !moving_var || !y) return MCCNN_E_BADARG;
    if (training && !saved) return MCCNN_E_BADARG;
    const size_t need = training ? mccnn_bn_act_workspace_bytes(n, c) : 0;
    if (need && (!ws || ws_bytes < need)) return MCCNN_E_WORKSPACE;
    const BnPlan p = bn_plan(n, c, bn_aligned16(x) && bn_aligned16(y) && (!need || bn_aligned16(ws)));
    BnArgs a = {};
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.mov_mean = moving_mean; a.mov_var = moving_var; a.saved = saved;
    a.part = (float*)ws;
    a.n = n; a.c = c; a.tw_log = p.tw_log; a.slab_rows = p.slab_rows; a.slabs = p.slabs; a.relu = relu ? 1 : 0;
    a.momentum = momentum; a.eps = eps; a.keep_scale = keep_scale; a.seed = seed;
    a.T = training ? keep_threshold : kBnDropAll;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs);
    if (!training) {
        if (p.vec == 4) bn_apply_k<4, 2><<<grid, kBnThreads, 0, st>>>(a);
        else bn_apply_k<1, 2><<<grid, kBnThreads, 0, st>>>(a);
        MCCNN_LAUNCHED();
        return 0;
    }
    if (n <= kBnSmallRows) {
        if (p.vec == 4) bn_apply_k<4, 1><<<grid, kBnThreads, 0, st>>>(a);
        else bn_apply_k<1, 1><<<grid, kBnThreads, 0, st>>>(a);
        MCCNN_LAUNCHED();
        return 0;
    }
    if (p.vec == 4) bn_stats_k<4><<<grid, kBnThreads, 0, st>>>(a);
    else bn_stats_k<1><<<grid, kBnThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    if (p.vec == 4) bn_apply_k<4, 0><<<grid, kBnThreads, 0, st>>>(a);
    else bn_apply_k<1, 0><<<grid, kBnThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    return 0;
}

int mccnn_bn_act_bwd(const float* x, const float* dy, int n, int c, const float* gamma, const float* beta,
                     const float* saved, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                     float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || c < 1) return MCCNN_E_BADARG;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !dy || !gamma || !beta || !saved || !dgamma || !dbeta) return MCCNN_E_BADARG;
    const size_t need = mccnn_bn_act_workspace_bytes(n, c);
    if (need && (!ws || ws_bytes < need)) return MCCNN_E_WORKSPACE;
    const BnPlan p = bn_plan(n, c, bn_aligned16(x) && bn_aligned16(dy) && (!dx || bn_aligned16(dx)) && (!need || bn_aligned16(ws)));
    BnArgs a = {};
    a.x = x; a.dy = dy; a.out = dx; a.gamma = gamma; a.beta = beta; a.saved = const_cast<float*>(saved);
    a.part = (float*)ws; a.dgamma = dgamma; a.dbeta = dbeta;
    a.n = n; a.c = c; a.tw_log = p.tw_log; a.slab_rows = p.slab_rows; a.slabs = p.slabs; a.relu = relu ? 1 : 0;
    a.want_dx = dx ? 1 : 0;
    a.keep_scale = keep_scale; a.seed = seed; a.T = keep_threshold;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs);
    if (n <= kBnSmallRows) {
        if (p.vec == 4) bn_bwd_dx_k<4, 1><<<grid, kBnThreads, 0, st>>>(a);
        else bn_bwd_dx_k<1, 1><<<grid, kBnThreads, 0, st>>>(a);
        MCCNN_LAUNCHED();
        return 0;
    }
    if (p.vec == 4) bn_bwd_sums_k<4><<<grid, kBnThreads, 0, st>>>(a);
    else bn_bwd_sums_k<1><<<grid, kBnThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    const dim3 grid2((unsigned)p.tiles, dx ? (unsigned)p.slabs : 1u);
    if (p.vec == 4) bn_bwd_dx_k<4, 0><<<grid2, kBnThreads, 0, st>>>(a);
    else bn_bwd_dx_k<1, 0><<<grid2, kBnThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    return 0;
}

}  // extern "C"
