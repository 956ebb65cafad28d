// The last linear layer and the sparse softmax cross-entropy behind it as one op (mccnn_linear_xent_fwd / _bwd):
//   z = x W + b,  lse_i = m_i + log(sum_j exp(z_ij - m_i)),  l_i = lse_i - z[i, y_i],  loss = sum_live rw_i l_i / D,
//   pred_i = the lowest arg-max of row i,  correct = the live rows with pred_i == y_i,  D = max(live rows, 1)
// with x [n, cin], W [cin, C] float32 row-major. A row is live when 0 <= y_i < C and its weight is not 0. The matmul is
// linear_bn.hip's GEMM body (lin_tile.h: one fmaf chain over k per element, the same k order whatever the tiling), so a
// logit here has the bytes of that op's z.
//   forward   a workgroup owns a slab of rows and walks it 64 rows at a time, per 64 rows the column tiles in order. A lane
//             holds four rows x four columns of a tile: per row it keeps the running (max, sum of exp(. - max), arg-max,
//             z_y) ONLINE over its own columns of every tile -- columns ascending, a strict > moves the arg-max, so the lowest
//             index stays -- and the 16 lanes of a row merge theirs in a butterfly whose two sides are always taken in
//             lane order. One lane per row writes lse and pred and adds the row to its own (sum rw l, live, correct); the
//             workgroup's 16 such lanes are added in lane order, the workgroups in workgroup order. One launch up to 256
//             rows (one workgroup finishes by itself), two above.
//   backward  launch 1 recomputes a z tile per (column tile, row tile) with the same body and writes
//             dz = g rw_i / D (exp(z - lse_i) - [j == y_i]) into the workspace, zeros on rows that are not live; g is read
//             from a device word. dx = dz W^T, dW = x^T dz with db as the column sums of the same dz chunks, and the slab
//             merge are linear_bn.hip's kernels. At most four launches.
// No atomics, no memset, fixed merge orders: the same inputs give the same bytes.
#include <climits>
#include "common.h"
#include "lin_tile.h"

namespace mccnn {

constexpr int kXentOneRows = 256;     // up to here one workgroup does the whole forward
constexpr int kXentMaxSlabs = 1024;   // forward workgroups (= partials the second launch merges)

struct LinXentFwdArgs {
    const float* x;
    const float* w;
    const float* b;
    const int* labels;
    const float* rw;     // NULL: all 1
    float* loss;
    float* lse;
    int* meta;           // D, correct
    int* pred;           // NULL: not wanted
    float* logits;       // NULL: not stored
    float* part;         // more than one slab: [slabs] sums, then [slabs] live rows and [slabs] correct rows as ints
    int n, cin, c, slab_rows, slabs;
};

__device__ __forceinline__ void lin_xent_finish(float sum, int live, int hit, float* loss, int* meta) {
    const int D = live > 1 ? live : 1;
    loss[0] = sum / (float)D;   // (no live row: +0 / 1)
    meta[0] = D;
    meta[1] = hit;
}

template <bool AV>
__global__ __launch_bounds__(kLinThreads) void lin_xent_fwd_k(LinXentFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float as[kLinTile * kLinAS];
    __shared__ __attribute__((aligned(16))) float bs[kLinKC * kLinBS];
    __shared__ float red_s[16];
    __shared__ int red_n[16], red_h[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = (int)blockIdx.x;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    const int ctiles = (a.c + kLinTile - 1) / kLinTile;
    float sum = 0.f;
    int live = 0, hit = 0;
    for (int m0 = row0; m0 < row1; m0 += kLinTile) {
        int y[4], arg[4];
        float m[4], s[4], zy[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + wave * 16 + 4 * (lane >> 4) + i;
            y[i] = row < row1 ? a.labels[row] : -1;
            m[i] = -INFINITY;
            s[i] = 0.f;
            zy[i] = 0.f;
            arg[i] = INT_MAX;
        }
        for (int ct = 0; ct < ctiles; ++ct) {
            const int c0 = ct * kLinTile;
            lin_f32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = lin_f32x4{0.f, 0.f, 0.f, 0.f};
            lin_tile<false, false, AV>(a.x, a.cin, a.w, a.c, row1, a.c, m0, c0, 0, a.cin, as, bs, acc, [](int) {});
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = c0 + t * 16 + (lane & 15);
                if (col >= a.c) continue;   // (columns past the edge take no part)
                const float bias = a.b[col];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = m0 + wave * 16 + 4 * (lane >> 4) + i;
                    const float v = acc[t][i] + bias;
                    if (a.logits && row < row1) a.logits[(size_t)row * a.c + col] = v;
                    if (v > m[i]) {
                        s[i] = s[i] * expf(m[i] - v) + 1.0f;
                        m[i] = v;
                        arg[i] = col;
                    } else {
                        s[i] = s[i] + expf(v - m[i]);
                    }
                    if (col == y[i]) zy[i] = v;
                }
            }
        }
        // the 16 lanes of a row: a butterfly, the lower lane's share always on the left
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const bool upper = (lane & off) != 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float om = __shfl_xor(m[i], off), os = __shfl_xor(s[i], off), oz = __shfl_xor(zy[i], off);
                const int oa = __shfl_xor(arg[i], off);
                const float mlo = upper ? om : m[i], mhi = upper ? m[i] : om;
                const float slo = upper ? os : s[i], shi = upper ? s[i] : os;
                const float zlo = upper ? oz : zy[i], zhi = upper ? zy[i] : oz;
                const int alo = upper ? oa : arg[i], ahi = upper ? arg[i] : oa;
                const float mm = fmaxf(mlo, mhi);
                const float flo = mlo == mm ? 1.0f : expf(mlo - mm), fhi = mhi == mm ? 1.0f : expf(mhi - mm);
                s[i] = slo * flo + shi * fhi;
                arg[i] = (mhi > mlo || (mhi == mlo && ahi < alo)) ? ahi : alo;
                m[i] = mm;
                zy[i] = zlo + zhi;   // (one lane at the most has the label's column; the others hold 0)
            }
        }
        if ((lane & 15) == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + wave * 16 + 4 * (lane >> 4) + i;
                if (row >= row1) continue;
                const float lse = m[i] + logf(s[i]);
                a.lse[row] = lse;
                if (a.pred) a.pred[row] = arg[i];
                const float rw = a.rw ? a.rw[row] : 1.0f;
                if (y[i] >= 0 && y[i] < a.c && rw != 0.f) {
                    sum = sum + rw * (lse - zy[i]);
                    ++live;
                    hit += arg[i] == y[i] ? 1 : 0;
                }
            }
        }
    }
    if ((lane & 15) == 0) {
        const int at = wave * 4 + (lane >> 4);
        red_s[at] = sum;
        red_n[at] = live;
        red_h[at] = hit;
    }
    __syncthreads();
    if (tid == 0) {
        float v = 0.f;
        int nl = 0, nh = 0;
        for (int k = 0; k < 16; ++k) {
            v = v + red_s[k];
            nl += red_n[k];
            nh += red_h[k];
        }
        if (a.slabs == 1) {
            lin_xent_finish(v, nl, nh, a.loss, a.meta);
        } else {
            int* pi = reinterpret_cast<int*>(a.part + a.slabs);
            a.part[slab] = v;
            pi[slab] = nl;
            pi[a.slabs + slab] = nh;
        }
    }
}

// forward, launch 2 (more than one slab): one workgroup; thread t adds its run of consecutive slabs, thread 0 the 256 runs
__global__ __launch_bounds__(kLinThreads) void lin_xent_merge_k(const float* __restrict__ part, int slabs, float* __restrict__ loss,
                                                                int* __restrict__ meta) {
    __shared__ float red_s[kLinThreads];
    __shared__ int red_n[kLinThreads], red_h[kLinThreads];
    const int tid = (int)threadIdx.x;
    const int* pi = reinterpret_cast<const int*>(part + slabs);
    const int per = (slabs + kLinThreads - 1) / kLinThreads;
    const int s0 = min(slabs, tid * per), s1 = min(slabs, s0 + per);
    float v = 0.f;
    int nl = 0, nh = 0;
    for (int s = s0; s < s1; ++s) {
        v = v + part[s];
        nl += pi[s];
        nh += pi[slabs + s];
    }
    red_s[tid] = v;
    red_n[tid] = nl;
    red_h[tid] = nh;
    __syncthreads();
    if (tid == 0) {
        v = 0.f;
        nl = nh = 0;
        for (int k = 0; k < kLinThreads; ++k) {
            v = v + red_s[k];
            nl += red_n[k];
            nh += red_h[k];
        }
        lin_xent_finish(v, nl, nh, loss, meta);
    }
}

struct LinXentDzArgs {
    const float* x;
    const float* w;
    const float* b;
    const int* labels;
    const float* rw;
    const float* lse;
    const int* meta;
    const float* g;      // the gradient of loss: one device word
    float* dz;
    int n, cin, c;
};

// backward, launch 1: grid (column tiles, row tiles)
template <bool AV>
__global__ __launch_bounds__(kLinThreads) void lin_xent_dz_k(LinXentDzArgs a) {
    __shared__ __attribute__((aligned(16))) float as[kLinTile * kLinAS];
    __shared__ __attribute__((aligned(16))) float bs[kLinKC * kLinBS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)blockIdx.x * kLinTile, m0 = (int)blockIdx.y * kLinTile;
    lin_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = lin_f32x4{0.f, 0.f, 0.f, 0.f};
    lin_tile<false, false, AV>(a.x, a.cin, a.w, a.c, a.n, a.c, m0, c0, 0, a.cin, as, bs, acc, [](int) {});
    const float g = a.g[0], D = (float)a.meta[0];
    int col[4];
    float bias[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        col[t] = c0 + t * 16 + (lane & 15);
        bias[t] = col[t] < a.c ? a.b[col[t]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + wave * 16 + 4 * (lane >> 4) + i;
        if (row >= a.n) continue;
        const int y = a.labels[row];
        const float rw = a.rw ? a.rw[row] : 1.0f;
        const bool live = y >= 0 && y < a.c && rw != 0.f;
        const float coef = live ? g * rw / D : 0.f, lse = a.lse[row];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (col[t] >= a.c) continue;
            const float v = acc[t][i] + bias[t];
            const float p = expf(v - lse) - (col[t] == y ? 1.0f : 0.f);
            a.dz[(size_t)row * a.c + col[t]] = live ? coef * p : 0.f;
        }
    }
}

inline int lin_xent_slab_rows(int n) {
    if (n <= kXentOneRows) return kXentOneRows;
    return kLinTile * ceil_div(ceil_div(n, kLinTile), kXentMaxSlabs);
}
inline size_t lin_xent_part_bytes(int n) {
    const int slabs = ceil_div(n, lin_xent_slab_rows(n));
    if (slabs == 1) return 0;
    return align_up((size_t)3 * (size_t)slabs * sizeof(float));
}
// An upper bound of lin_dw_bytes that grows with each of n, cin and c (the plan's own slab count does not: it rounds): what
// the workspace query answers for the dW / db planes.
inline size_t lin_xent_planes_bound(int n, int cin, int c) {
    long long s = ceil_div(n, kLinDwSlabRows);
    if (s > kLinDwMaxSlabs) s = kLinDwMaxSlabs;
    if (s <= 1) return 0;
    const long long per = (long long)cin * c + c;
    const long long f = s * per < kLinDwMaxFloats + per ? s * per : kLinDwMaxFloats + per;
    return align_up((size_t)f * sizeof(float));
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

size_t mccnn_linear_xent_workspace_bytes(int n, int cin, int c) {
    if (n < 1 || cin < 1 || c < 1 || !lin_sizes_ok(n, cin, c)) return 0;
    // the backward's: dz and the dW / db planes (a bound that is monotone in every size); the forward's partials (three
    // words per slab, no slab below 64 rows) fit the front of dz whatever c is -- the larger of the two all the same
    const size_t bwd = lin_dz_bytes(n, c) + lin_xent_planes_bound(n, cin, c), fwd = lin_xent_part_bytes(n);
    return bwd > fwd ? bwd : fwd;
}

int mccnn_linear_xent_fwd(const float* x, const float* w, const float* b, int n, int cin, int c, const int* labels,
                          const float* row_weights, float* loss, float* lse, int* meta, int* pred, float* logits, void* ws,
                          size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || cin < 1 || c < 1) return MCCNN_E_BADARG;
    if (!x || !w || !b || !labels || !loss || !lse || !meta) return MCCNN_E_BADARG;
    if (!lin_sizes_ok(n, cin, c)) return MCCNN_E_TOOLARGE;
    const size_t need = lin_xent_part_bytes(n);
    if (need && (!ws || ws_bytes < need)) return MCCNN_E_WORKSPACE;
    LinXentFwdArgs a = {};
    a.x = x; a.w = w; a.b = b; a.labels = labels; a.rw = row_weights; a.loss = loss; a.lse = lse; a.meta = meta; a.pred = pred;
    a.logits = logits; a.part = (float*)ws;
    a.n = n; a.cin = cin; a.c = c;
    a.slab_rows = lin_xent_slab_rows(n);
    a.slabs = ceil_div(n, a.slab_rows);
    hipStream_t st = (hipStream_t)stream;
    if (cin % 4 == 0 && lin_aligned16(x)) lin_xent_fwd_k<true><<<(unsigned)a.slabs, kLinThreads, 0, st>>>(a);
    else lin_xent_fwd_k<false><<<(unsigned)a.slabs, kLinThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    if (a.slabs > 1) {
        lin_xent_merge_k<<<1, kLinThreads, 0, st>>>(a.part, a.slabs, loss, meta);
        MCCNN_LAUNCHED();
    }
    return 0;
}

int mccnn_linear_xent_bwd(const float* x, const float* w, const float* b, int n, int cin, int c, const int* labels,
                          const float* row_weights, const float* lse, const int* meta, const float* loss_grad, float* dx, float* dw,
                          float* db, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || cin < 1 || c < 1) return MCCNN_E_BADARG;
    if (!x || !w || !b || !labels || !lse || !meta || !loss_grad || !dw || !db) return MCCNN_E_BADARG;
    if (!lin_sizes_ok(n, cin, c)) return MCCNN_E_TOOLARGE;
    const size_t need = mccnn_linear_xent_workspace_bytes(n, cin, c);
    if (!ws || ws_bytes < need) return MCCNN_E_WORKSPACE;
    float* dz = (float*)ws;
    float* planes = (float*)((char*)ws + lin_dz_bytes(n, c));
    hipStream_t st = (hipStream_t)stream;
    {
        LinXentDzArgs a = {};
        a.x = x; a.w = w; a.b = b; a.labels = labels; a.rw = row_weights; a.lse = lse; a.meta = meta; a.g = loss_grad; a.dz = dz;
        a.n = n; a.cin = cin; a.c = c;
        const dim3 grid((unsigned)ceil_div(c, kLinTile), (unsigned)ceil_div(n, kLinTile));
        if (cin % 4 == 0 && lin_aligned16(x)) lin_xent_dz_k<true><<<grid, kLinThreads, 0, st>>>(a);
        else lin_xent_dz_k<false><<<grid, kLinThreads, 0, st>>>(a);
        MCCNN_LAUNCHED();
    }
    if (dx) {
        LinMmArgs a = {};
        a.a = dz; a.lda = c; a.b = w; a.ldb = c; a.out = dx; a.M = n; a.N = cin; a.K = c; a.kper = c;
        const dim3 grid((unsigned)ceil_div(cin, kLinTile), (unsigned)ceil_div(n, kLinTile), 1);
        if (c % 4 == 0 && lin_aligned16(dz)) lin_mm_k<false, true, true, false><<<grid, kLinThreads, 0, st>>>(a);
        else lin_mm_k<false, true, false, false><<<grid, kLinThreads, 0, st>>>(a);
        MCCNN_LAUNCHED();
    }
    const LinDwPlan p = lin_dw_plan(n, cin, c);
    const int wn = cin * c;
    LinMmArgs a = {};
    a.a = x; a.lda = cin; a.b = dz; a.ldb = c; a.M = cin; a.N = c; a.K = n; a.kper = p.kper; a.plane = (size_t)wn;
    a.out = p.slabs == 1 ? dw : planes;
    a.colsum = p.slabs == 1 ? db : planes + (size_t)p.slabs * wn;
    const dim3 grid((unsigned)ceil_div(c, kLinTile), (unsigned)ceil_div(cin, kLinTile), (unsigned)p.slabs);
    lin_mm_k<true, false, false, true><<<grid, kLinThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    if (p.slabs > 1) {
        lin_dw_merge_k<<<(unsigned)ceil_div((long long)wn + c, kLinThreads), kLinThreads, 0, st>>>(
            planes, planes + (size_t)p.slabs * wn, dw, db, wn, c, p.slabs);
        MCCNN_LAUNCHED();
    }
    return 0;
}

}  // extern "C"
