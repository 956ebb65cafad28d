// The dense glue between two MC convolutions as one op (mccnn_bn_act_fwd / _bwd and their typed forms _fwd_rows /
// _bwd_rows): y = drop(act(bn(x))) over an [n, c] row-major tensor, batch statistics over the rows. x (and dx) and y (and
// dy) are float32 or bfloat16 storage, independently: bf16 is widened exactly on load and rounded to nearest even at the
// store, everything in between is f32 and the same for every type (XT, YT below change loads and stores only).
//
// A workgroup of 256 threads owns a tile of 128 bytes of a row of x and a slab of rows: tw threads across, 256 / tw row
// lanes down. f32 x: up to 32 columns, 4 per thread when c % 4 == 0 and the row pointers allow (x, f32 y / dy / dx on 16
// bytes, bf16 y / dy on 8), one per thread otherwise. bf16 x: up to 64 columns, 8 per thread (one 16-byte piece) when
// c % 8 == 0 and every row pointer is on 16 bytes, a pair (one 32-bit word) otherwise. tw is at most 8 in the wide forms
// and 32 in the narrow ones, whatever the type.
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
//   over a concatenation (mccnn_bn_act_cat_fwd / _bwd, _fwd_rows / _bwd_rows): up to 8 segments [n, c_s] in place of x, never
//                       concatenated, each f32 or bf16. The plan, the launches and the arithmetic are those of f32 x at width
//                       C = sum c_s; a thread looks its segment up once (bn_cat.h) and reads x_s + r * c_s + (col - col0_s),
//                       in its segment's type when one of them is bf16 (BnXSeg). The table is a kernel argument of those
//                       instantiations alone.
// No atomics, no memset, no ticket or spin-wait between workgroups; a fixed merge order: the same inputs and seed give the
// same bytes. The gate is pre > 0 (torch's relu'), not the >= 0 of the convolution kernels.
#include <initializer_list>
#include <type_traits>

#include "common.h"
#include "bn_drop.h"
#include "bn_act.h"
#include "bn_cat.h"   // the plan (BnPlan, bn_plan and its constants) and the segment table of the op over a concatenation

namespace mccnn {

// rows of a thread whose loads are in flight together in the streaming loops of the forward. 8 columns per thread (bf16 x)
// come with half the workgroups of the f32 layout for the same c, each moving up to twice the bytes: they keep more ahead
template <int VEC>
constexpr int kBnRowsAhead = VEC == 8 ? 8 : 4;

int bn_slab_rows(int n) { return bn_slab_rows_of(n); }

struct BnArgs {
    const void* x;       // XT
    const void* dy;      // YT
    void* out;           // y (forward, YT) or dx (backward, XT)
    const float* gamma;
    const float* beta;
    float* mov_mean;
    float* mov_var;
    float* saved;        // [2, c]: written by the forward, read by the backward
    const float* shift;  // backward, linear_bn.hip only: per column what the exact mean has over saved's (NULL: nothing)
    float* part;         // the slab partials: planes of [nparts, c]
    float* dgamma;
    float* dbeta;
    float* rparts;       // statistics across ranks (mccnn_bn_sync_*): the rank partials [world, 3, c]
    int* meta;           // ... and (rowBase, N), written by their apply
    int n, c, tw_log, slab_rows, slabs, nparts, relu, want_dx;   // slabs: the grid's; nparts: rows of a plane of `part`
    int rank, world;
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
    t.ok = col < (long long)a.c;    // (c % VEC == 0, so all VEC columns are inside)
    t.col = t.ok ? (int)col : 0;
    return t;
}

// Where the rows of a thread's columns of x (and dx) are. The contiguous op (BnXPlain): the tensor itself at the global
// column; over a concatenation (BnXCat, bn_cat.h): the thread's segment, found once. Everything else a thread touches -- y,
// dy, gamma, beta, saved, the partials, the mask -- is at the global column t.col either way.
// x / dx: the rows; at: the element offset of the thread's first column in row r; want (backward): dx is wanted. The helpers
// and kernels below take either as XS / X.
struct BnXPlain {
    __device__ __forceinline__ const void* x(const BnArgs& a) const { return a.x; }
    __device__ __forceinline__ void* dx(const BnArgs& a) const { return a.out; }
    __device__ __forceinline__ size_t at(const BnArgs& a, const BnCoord& t, size_t r) const { return r * a.c + t.col; }
    __device__ __forceinline__ bool want(const BnArgs& a) const { return a.want_dx; }
};
struct BnXCat {
    BnCatAt s;
    __device__ __forceinline__ const void* x(const BnArgs&) const { return s.x; }
    __device__ __forceinline__ void* dx(const BnArgs&) const { return s.dx; }
    __device__ __forceinline__ size_t at(const BnArgs&, const BnCoord&, size_t r) const { return r * s.ld + s.col; }
    __device__ __forceinline__ bool want(const BnArgs&) const { return s.dx != nullptr; }
};
__device__ __forceinline__ BnXPlain bn_x(const BnArgs&, const BnCoord&) { return BnXPlain(); }
__device__ __forceinline__ BnXCat bn_x(const BnArgs&, const BnCoord& t, const BnCat& s) { return BnXCat{bn_cat_at(s, t.col)}; }

// XT of the typed-segment instantiations over a concatenation (mccnn_bn_act_cat_fwd_rows / _bwd_rows with a bf16 segment): x
// and dx have the type of the thread's SEGMENT (BnCatAt::bf16), float or bn_bf16 below. The row loops -- bn_slab_stats's,
// bn_apply_rows, bn_grad_rows, bn_dx_rows, none with a barrier inside -- branch on it (bn_seg_typed)
// once, ahead of the loop, into their float or bn_bf16 member; the threads of a wave may take different sides (a tile may
// straddle a type boundary) and meet again before the next barrier. Everything else does not know x's type.
struct BnXSeg {};
template <typename XT>
constexpr bool kBnXSeg = std::is_same<XT, BnXSeg>::value;

// VEC f32 values of the library's own memory (LDS, the slab partials): p is on VEC * 4 bytes, 16 at the most
template <int VEC>
__device__ __forceinline__ void bn_ld(const float* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 8) {
        const float4 q = reinterpret_cast<const float4*>(p)[0], r = reinterpret_cast<const float4*>(p)[1];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; v[4] = r.x; v[5] = r.y; v[6] = r.z; v[7] = r.w;
    } else if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (VEC == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p);
        v[0] = q.x; v[1] = q.y;
    } else {
        v[0] = *p;
    }
}
template <int VEC>
__device__ __forceinline__ void bn_st(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 8) {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else {
        *p = v[0];
    }
}

// The element types of a caller's rows: float, or bf16 storage (bn_bf16: 16 bits, widened exactly / rounded to nearest even)
typedef uint16_t bn_bf16;

// f(xt) for a thread of a typed-segment instantiation, xt a zero of the element type of its segment. f has no barrier inside.
template <typename F>
__device__ __forceinline__ void bn_seg_typed(const BnXCat& X, F&& f) {
    if (X.s.bf16) f(bn_bf16());
    else f(float());
}

// VEC elements at element offset `at` of a caller's tensor: bn_ld_raw moves them as they are stored (bn_raw_words 32-bit
// words; one bf16 alone sits in the low half of a word), bn_widen makes f32 of them (bf16: exactly), bn_ldr is both. The
// plan has looked at the pointers: VEC 8 and 4 only where every access below is aligned (f32: 16 bytes; bf16: 16 for VEC 8,
// 8 for VEC 4); a pair of f32 moves as two words (an f32 pointer promises 4 bytes), a pair of bf16 as one (the entries
// refuse a bf16 pointer off a 4-byte boundary)
template <int VEC, typename T>
constexpr int bn_raw_words() { return VEC * (int)sizeof(T) >= 4 ? VEC * (int)sizeof(T) / 4 : 1; }
template <int VEC, typename T>
__device__ __forceinline__ void bn_ld_raw(const void* __restrict__ base, size_t at, uint32_t (&w)[bn_raw_words<VEC, T>()]) {
    const T* p = static_cast<const T*>(base) + at;
    constexpr int W = bn_raw_words<VEC, T>();
    if constexpr (sizeof(T) == 2 && VEC == 1) {
        w[0] = *p;
    } else if constexpr (W >= 4) {
#pragma unroll
        for (int i = 0; i < W / 4; ++i) {
            const uint4 u = reinterpret_cast<const uint4*>(p)[i];
            w[4 * i] = u.x; w[4 * i + 1] = u.y; w[4 * i + 2] = u.z; w[4 * i + 3] = u.w;
        }
    } else if constexpr (W == 2 && sizeof(T) == 2) {
        const uint2 u = *reinterpret_cast<const uint2*>(p);
        w[0] = u.x; w[1] = u.y;
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
    }
}
template <int VEC, typename T>
__device__ __forceinline__ void bn_widen(const uint32_t (&w)[bn_raw_words<VEC, T>()], float (&v)[VEC]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = __uint_as_float(w[k]);
    } else if constexpr (VEC == 8) {
        bf16x8_to_f32(make_uint4(w[0], w[1], w[2], w[3]), v);
    } else if constexpr (VEC == 1) {
        v[0] = __uint_as_float(w[0] << 16);
    } else {
#pragma unroll
        for (int i = 0; i < VEC / 2; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    }
}
template <int VEC, typename T>
__device__ __forceinline__ void bn_ldr(const void* __restrict__ base, size_t at, float (&v)[VEC]) {
    uint32_t w[bn_raw_words<VEC, T>()];
    bn_ld_raw<VEC, T>(base, at, w);
    bn_widen<VEC, T>(w, v);
}
template <int VEC, typename T>
__device__ __forceinline__ void bn_str(void* __restrict__ base, size_t at, const float (&v)[VEC]) {
    if constexpr (sizeof(T) == 4) {
        float* p = static_cast<float*>(base) + at;
        if constexpr (VEC == 2) { p[0] = v[0]; p[1] = v[1]; }
        else bn_st<VEC>(p, v);
    } else {
        bn_bf16* p = static_cast<bn_bf16*>(base) + at;
        if constexpr (VEC == 8) {
            *reinterpret_cast<uint4*>(p) = f32x8_to_bf16(v);
        } else if constexpr (VEC == 4) {
            *reinterpret_cast<uint2*>(p) = make_uint2(f32x2_to_bf16(v[0], v[1]), f32x2_to_bf16(v[2], v[3]));
        } else if constexpr (VEC == 2) {
            *reinterpret_cast<unsigned*>(p) = f32x2_to_bf16(v[0], v[1]);
        } else {
            *p = (bn_bf16)(f32x2_to_bf16(v[0], 0.f) & 0xffffu);
        }
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

// The row loop of bn_slab_stats below for a thread of a typed-segment instantiation, T its segment's element type: K, the
// shift -- the slab's first row -- and the sums of (x - K) and (x - K)^2 over rows row0 + ry, + R, ... below row1; -> the rows
// taken. (A second copy of that loop on purpose: as a function called from bn_slab_stats it changes the code the compiler
// makes of the contiguous, f32-segment and cross-rank kernels, which keep theirs.)
template <int VEC, typename T>
__device__ __forceinline__ int bn_seg_rows_acc(const BnArgs& a, const BnCoord& t, const BnXCat& X, int row0, int row1, float (&K)[VEC],
                                               float (&s1)[VEC], float (&s2)[VEC]) {
    int rows = 0;
    bn_ldr<VEC, T>(X.x(a), X.at(a, t, (size_t)row0), K);
#pragma unroll kBnRowsAhead<VEC>
    for (int r = row0 + t.ry; r < row1; r += t.R) {
        float v[VEC];
        bn_ldr<VEC, T>(X.x(a), X.at(a, t, (size_t)r), v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float d = v[k] - K[k];
            s1[k] = s1[k] + d;
            s2[k] = s2[k] + d * d;
        }
        ++rows;
    }
    return rows;
}

// (count, mean, M2) of rows [row0, row1) of the thread's columns, merged over the row lanes
template <int VEC, typename XT, typename XS>
__device__ __forceinline__ void bn_slab_stats(const BnArgs& a, const BnCoord& t, const XS& X, int row0, int row1, float& cnt,
                                              float (&mean)[VEC], float (&m2)[VEC], float* lds) {
    float s1[VEC], s2[VEC], K[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { s1[k] = 0.f; s2[k] = 0.f; K[k] = 0.f; }
    int rows = 0;
    if (t.ok && row0 < row1) {
        if constexpr (kBnXSeg<XT>) {
            bn_seg_typed(X, [&](auto xt) { rows = bn_seg_rows_acc<VEC, decltype(xt)>(a, t, X, row0, row1, K, s1, s2); });
        } else {
            bn_ldr<VEC, XT>(X.x(a), X.at(a, t, (size_t)row0), K);   // the shift: the slab's first row
#pragma unroll kBnRowsAhead<VEC>
            for (int r = row0 + t.ry; r < row1; r += t.R) {
                float v[VEC];
                bn_ldr<VEC, XT>(X.x(a), X.at(a, t, (size_t)r), v);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float d = v[k] - K[k];
                    s1[k] = s1[k] + d;
                    s2[k] = s2[k] + d * d;
                }
                ++rows;
            }
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
    const size_t plane = (size_t)a.nparts * a.c;
    if (t.ok)
        for (int s = t.ry; s < a.nparts; s += t.R) {
            const float* p = a.part + (size_t)s * a.c + t.col;
            float mB[VEC], qB[VEC];
            bn_ld<VEC>(p + plane, mB);
            bn_ld<VEC>(p + 2 * plane, qB);
            bn_chan<VEC>(cnt, mean, m2, p[0], mB, qB);
        }
    bn_tree_merge<VEC>(a, t, cnt, mean, m2, lds);
}

// row lane 0: mean and rstd of the thread's columns into LDS for the workgroup; `first`: also saved and the moving statistics.
// fn: the rows in the statistics, looked at in row lane 0 only. Every thread of the workgroup calls it.
template <int VEC>
__device__ __forceinline__ void bn_finish_stats(const BnArgs& a, const BnCoord& t, float fn, const float (&mean)[VEC],
                                                const float (&m2)[VEC], bool first, float (*sm)[kBnTileCols]) {
    if (t.ry == 0 && t.ok) {
        const float keep = 1.0f - a.momentum;
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

// base: what the mask's row index has over the local one (statistics across ranks: the rows of the lower ranks)
template <int VEC, typename XT, typename YT, typename XS>
__device__ __forceinline__ void bn_apply_rows(const BnArgs& a, const BnCoord& t, const XS& X, int row0, int row1, const float (&mean)[VEC],
                                              const float (&rstd)[VEC], bool drop, int base = 0) {
    if (!t.ok) return;   // (no barrier follows)
    float g[VEC], b[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { g[k] = a.gamma[t.col + k]; b[k] = a.beta[t.col + k]; }
    // the loads of U rows go out before the first row is used and stored: y may be x's memory for all the compiler knows,
    // so behind a row's store it would hold the next row's load back, one memory latency per row
    constexpr int U = kBnRowsAhead<VEC>;
    for (long long r = row0 + t.ry; r < row1; r += U * t.R) {
        uint32_t wx[U][bn_raw_words<VEC, XT>()];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (r + u * t.R < row1) bn_ld_raw<VEC, XT>(X.x(a), X.at(a, t, (size_t)(r + u * t.R)), wx[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long ru = r + u * t.R;
            if (ru >= row1) break;
            float v[VEC], o[VEC];
            bn_widen<VEC, XT>(wx[u], v);
            const uint32_t rh = drop ? bn_drop_row(a.seed, base + (int)ru) : 0u;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float xh = (v[k] - mean[k]) * rstd[k];
                const float pre = xh * g[k] + b[k];
                float act = a.relu ? (pre > 0.f ? pre : 0.f) : pre;
                if (drop) act = bn_drop_keep(rh, (uint32_t)(t.col + k), a.T) ? act * a.keep_scale : 0.f;
                o[k] = act;
            }
            bn_str<VEC, YT>(a.out, (size_t)ru * a.c + t.col, o);
        }
    }
}

// forward, training, launch 1
// CAT (here and in the three kernels that read x below): nothing -- the contiguous op, the kernel's only argument is BnArgs --
// or BnCat, the segment table of the op over a concatenation (mccnn_bn_act_cat_fwd / _bwd and their _rows forms; XT float, or
// BnXSeg when a segment is bf16), an argument of those instantiations alone. The body is the same: it asks X where the
// thread's rows are.
template <int VEC, typename XT, typename... CAT>
__global__ __launch_bounds__(kBnThreads) void bn_stats_k(BnArgs a, CAT... s) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * (1 + 2 * VEC)];
    const BnCoord t = bn_coord<VEC>(a);
    const auto X = bn_x(a, t, s...);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float cnt, mean[VEC], m2[VEC];
    bn_slab_stats<VEC, XT>(a, t, X, row0, row1, cnt, mean, m2, lds);
    if (t.ry == 0 && t.ok) {
        const size_t plane = (size_t)a.nparts * a.c;
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
template <int VEC, typename XT, typename YT, int MODE, typename... CAT>
__global__ __launch_bounds__(kBnThreads) void bn_apply_k(BnArgs a, CAT... s) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * (1 + 2 * VEC)];
    __shared__ float sm[2][kBnTileCols];
    const BnCoord t = bn_coord<VEC>(a);
    const auto X = bn_x(a, t, s...);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float mean[VEC], rstd[VEC];
    if constexpr (MODE == 2) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            mean[k] = t.ok ? a.mov_mean[t.col + k] : 0.f;
            rstd[k] = t.ok ? 1.0f / sqrtf(a.mov_var[t.col + k] + a.eps) : 0.f;
        }
        if constexpr (kBnXSeg<XT>) bn_seg_typed(X, [&](auto xt) { bn_apply_rows<VEC, decltype(xt), YT>(a, t, X, row0, row1, mean, rstd, false); });
        else bn_apply_rows<VEC, XT, YT>(a, t, X, row0, row1, mean, rstd, false);
    } else {
        float cnt, m2[VEC];
        if constexpr (MODE == 0) bn_merge_partials<VEC>(a, t, cnt, mean, m2, lds);
        else bn_slab_stats<VEC, XT>(a, t, X, 0, a.n, cnt, mean, m2, lds);
        bn_finish_stats<VEC>(a, t, (float)a.n, mean, m2, slab == 0, sm);
#pragma unroll
        for (int k = 0; k < VEC; ++k) { mean[k] = sm[0][t.cx * VEC + k]; rstd[k] = sm[1][t.cx * VEC + k]; }
        if constexpr (kBnXSeg<XT>) bn_seg_typed(X, [&](auto xt) { bn_apply_rows<VEC, decltype(xt), YT>(a, t, X, row0, row1, mean, rstd, a.T < kBnDropAll); });
        else bn_apply_rows<VEC, XT, YT>(a, t, X, row0, row1, mean, rstd, a.T < kBnDropAll);
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
template <int VEC>
struct BnCols {
    float mean[VEC], rstd[VEC], g[VEC], b[VEC], c[VEC];
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
        q.c[k] = (t.ok && a.shift) ? a.shift[t.col + k] : 0.f;
    }
    return q;
}
// g = dy * mask * scale * gate and xhat of row r of the thread's columns from its x (v) and dy (d): the forward's
// arithmetic, operand for operand
template <int VEC>
__device__ __forceinline__ void bn_row_grad(const BnArgs& a, const BnCoord& t, const BnCols<VEC>& q, int r, bool drop,
                                            const float (&v)[VEC], const float (&d)[VEC], float (&g)[VEC], float (&xh)[VEC]) {
    const uint32_t rh = drop ? bn_drop_row(a.seed, r) : 0u;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        xh[k] = ((v[k] - q.mean[k]) - q.c[k]) * q.rstd[k];   // (c = 0 without a shift: x - 0 is x, bit for bit)
        const float pre = xh[k] * q.g[k] + q.b[k];
        float w = d[k];
        if (drop) w = bn_drop_keep(rh, (uint32_t)(t.col + k), a.T) ? w * a.keep_scale : 0.f;
        if (a.relu) w = pre > 0.f ? w : 0.f;
        g[k] = w;
    }
}
// f(r, g, xh) over rows row0 + ry, + R, ... below row1, in that order. The loads of U rows are issued before the first of
// them is used: behind the (uniform) relu and dropout branches of a row the compiler would otherwise hold the next row's
// loads back, one memory latency per row.
// base: what the mask's row index has over the local one (bn_apply_rows); f sees the local row.
template <int VEC, typename XT, typename YT, typename F, typename XS>
__device__ __forceinline__ void bn_grad_rows(const BnArgs& a, const BnCoord& t, const XS& X, const BnCols<VEC>& q, int row0, int row1,
                                             bool drop, F&& f, int base = 0) {
    if constexpr (kBnXSeg<XT>) {   // (bn_slab_sums; bn_dx_rows has branched already)
        if (X.s.bf16) bn_grad_rows<VEC, bn_bf16, YT>(a, t, X, q, row0, row1, drop, f, base);
        else bn_grad_rows<VEC, float, YT>(a, t, X, q, row0, row1, drop, f, base);
    } else {
        constexpr int U = 4;
        for (long long r = row0 + t.ry; r < row1; r += U * t.R) {
            uint32_t wx[U][bn_raw_words<VEC, XT>()], wd[U][bn_raw_words<VEC, YT>()];   // (as stored: widened where they are used)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long ru = r + u * t.R;
                if (ru < row1) {
                    bn_ld_raw<VEC, XT>(X.x(a), X.at(a, t, (size_t)ru), wx[u]);
                    bn_ld_raw<VEC, YT>(a.dy, (size_t)ru * a.c + t.col, wd[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long ru = r + u * t.R;
                if (ru < row1) {
                    float v[VEC], d[VEC], g[VEC], xh[VEC];
                    bn_widen<VEC, XT>(wx[u], v);
                    bn_widen<VEC, YT>(wd[u], d);
                    bn_row_grad<VEC>(a, t, q, base + (int)ru, drop, v, d, g, xh);
                    f((int)ru, g, xh);
                }
            }
        }
    }
}
template <int VEC, typename XT, typename YT, typename XS>
__device__ __forceinline__ void bn_slab_sums(const BnArgs& a, const BnCoord& t, const XS& X, const BnCols<VEC>& q, int row0, int row1,
                                             float (&sg)[VEC], float (&sx)[VEC], float (&sh)[VEC], float* lds, int base = 0) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) { sg[k] = 0.f; sx[k] = 0.f; sh[k] = 0.f; }
    const bool drop = a.T < kBnDropAll;
    if (t.ok)
        bn_grad_rows<VEC, XT, YT>(a, t, X, q, row0, row1, drop, [&](int, const float (&g)[VEC], const float (&xh)[VEC]) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) { sg[k] = sg[k] + g[k]; sx[k] = sx[k] + g[k] * xh[k]; sh[k] = sh[k] + xh[k]; }
        }, base);
    bn_tree_sum<VEC>(a, t, sg, sx, sh, lds);
}
// the slab partials of three plain sums of the thread's columns, summed: slabs ry, ry + R, ... in order per row lane, then
// the tree
template <int VEC>
__device__ __forceinline__ void bn_sum_partials(const BnArgs& a, const BnCoord& t, float (&sg)[VEC], float (&sx)[VEC],
                                                float (&sh)[VEC], float* lds) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) { sg[k] = 0.f; sx[k] = 0.f; sh[k] = 0.f; }
    const size_t plane = (size_t)a.nparts * a.c;
    if (t.ok)
        for (int s = t.ry; s < a.nparts; s += t.R) {
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

// the dx half of launch 2 of the backward: dx of rows [row0, row1) from the workgroup's (sum g, sum g * (xhat - mh), mh) in
// sm, fn rows in the statistics. base: what the mask's row index has over the local one (bn_apply_rows)
template <int VEC, typename XT, typename YT, typename XS>
__device__ __forceinline__ void bn_dx_rows(const BnArgs& a, const BnCoord& t, const XS& X, const BnCols<VEC>& q, int row0, int row1, float fn,
                                           const float (*sm)[kBnTileCols], int base) {
    if (!X.want(a) || !t.ok) return;
    const bool drop = a.T < kBnDropAll;
    float kb[VEC], kg[VEC], gr[VEC], mh[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        kb[k] = sm[0][t.cx * VEC + k] / fn;
        kg[k] = sm[1][t.cx * VEC + k] / fn;
        mh[k] = sm[2][t.cx * VEC + k];
        gr[k] = q.g[k] * q.rstd[k];
    }
    bn_grad_rows<VEC, XT, YT>(a, t, X, q, row0, row1, drop, [&](int r, const float (&g)[VEC], const float (&xh)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = gr[k] * (g[k] - kb[k] - (xh[k] - mh[k]) * kg[k]);
        bn_str<VEC, XT>(X.dx(a), X.at(a, t, (size_t)r), o);
    }, base);
}

// backward, launch 1: the partial (sum g, sum g * xhat, sum xhat) of a slab. sum xhat is zero for the exact mean; with the
// saved f32 mean it is -n * (mean's rounding error) * rstd, and launch 2 takes that shift out of xhat again -- on a column
// of few rows with |mean| >> std (var + eps barely above var) dx is the small remainder of cancelling terms, and the
// shift alone would cost it more than 1e-4
// SYNC (statistics across ranks): the mask at the global rows, meta[0] on
template <int VEC, typename XT, typename YT, int SYNC = 0, typename... CAT>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_sums_k(BnArgs a, CAT... s) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * 3 * VEC];
    const BnCoord t = bn_coord<VEC>(a);
    const auto X = bn_x(a, t, s...);
    const BnCols<VEC> q = bn_cols<VEC>(a, t);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float sg[VEC], sx[VEC], sh[VEC];
    if constexpr (SYNC) bn_slab_sums<VEC, XT, YT>(a, t, X, q, row0, row1, sg, sx, sh, lds, a.meta[0]);
    else bn_slab_sums<VEC, XT, YT>(a, t, X, q, row0, row1, sg, sx, sh, lds);
    if (t.ry == 0 && t.ok) {
        const size_t plane = (size_t)a.nparts * a.c;
        float* p = a.part + (size_t)slab * a.c + t.col;
        bn_st<VEC>(p, sg);
        bn_st<VEC>(p + plane, sx);
        bn_st<VEC>(p + 2 * plane, sh);
    }
}

// backward, launch 2 (SMALL = 0: partials from launch 1, merged per workgroup) or the one-launch form (SMALL = 1): dgamma and
// dbeta from slab 0, dx when wanted (without it the grid is one slab deep: the merge alone, in the same order)
template <int VEC, typename XT, typename YT, int SMALL, typename... CAT>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_dx_k(BnArgs a, CAT... s) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * 3 * VEC];
    __shared__ float sm[3][kBnTileCols];
    const BnCoord t = bn_coord<VEC>(a);
    const auto X = bn_x(a, t, s...);
    const BnCols<VEC> q = bn_cols<VEC>(a, t);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float sg[VEC], sx[VEC], sh[VEC];
    if constexpr (SMALL) {
        bn_slab_sums<VEC, XT, YT>(a, t, X, q, 0, a.n, sg, sx, sh, lds);
    } else {
        bn_sum_partials<VEC>(a, t, sg, sx, sh, lds);
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
    if constexpr (kBnXSeg<XT>) bn_seg_typed(X, [&](auto xt) { bn_dx_rows<VEC, decltype(xt), YT>(a, t, X, q, row0, row1, fn, sm, 0); });
    else bn_dx_rows<VEC, XT, YT>(a, t, X, q, row0, row1, fn, sm, 0);
}

// ---- batch statistics across the ranks of a process group (mccnn_bn_sync_*) ----------------------------------------------
// The op cut in two where the collective goes. The rank partials [world, 3, c] hold per rank and column what a slab
// partial holds per slab: (count, mean, M2) forward, (sum g, sum g * xhat, sum xhat) backward. A rank writes its own row
// and +0.0f into every other (an all-reduce(SUM) of the tensor is then an exact gather); behind the collective every
// workgroup merges the `world` rows of ITS columns in rank order, in the threads of row lane 0, once, ahead of its rows.
// These few values move as single floats: nothing is asked of the tensor's alignment.
template <int VEC>
__device__ __forceinline__ void bn_rank_put(const BnArgs& a, const BnCoord& t, const float (&p0)[VEC], const float (&p1)[VEC],
                                            const float (&p2)[VEC]) {
    if (t.ry != 0 || !t.ok) return;
    const size_t c = (size_t)a.c;
    for (int w = 0; w < a.world; ++w) {
        float* p = a.rparts + (size_t)w * 3 * c + t.col;
        const bool own = w == a.rank;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            p[k] = own ? p0[k] : 0.f;
            p[c + k] = own ? p1[k] : 0.f;
            p[2 * c + k] = own ? p2[k] : 0.f;
        }
    }
}

// this rank's (count, mean, M2) into its row of the rank partials. SMALL: from x (n <= 256, the only launch); otherwise
// from the slab partials of bn_stats_k, merged as launch 2 of the plain forward merges them. One slab deep.
template <int VEC, typename XT, int SMALL>
__global__ __launch_bounds__(kBnThreads) void bn_sync_stats_k(BnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * (1 + 2 * VEC)];
    const BnCoord t = bn_coord<VEC>(a);
    float cnt, mean[VEC], m2[VEC];
    if constexpr (SMALL) bn_slab_stats<VEC, XT>(a, t, BnXPlain(), 0, a.n, cnt, mean, m2, lds);
    else bn_merge_partials<VEC>(a, t, cnt, mean, m2, lds);
    float cv[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) cv[k] = cnt;
    bn_rank_put<VEC>(a, t, cv, mean, m2);
}

// the gathered rank partials merged by Chan's rule in rank order, then launch 2 of the plain forward with N rows in the
// statistics and the mask at the global rows. Slab 0 of a column tile writes saved and the moving statistics, the first
// workgroup meta = (rowBase, N).
template <int VEC, typename XT, typename YT>
__global__ __launch_bounds__(kBnThreads) void bn_sync_apply_k(BnArgs a) {
    __shared__ float sm[2][kBnTileCols];
    __shared__ int sbase;
    const BnCoord t = bn_coord<VEC>(a);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    float cnt = 0.f, mean[VEC], m2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { mean[k] = 0.f; m2[k] = 0.f; }
    int total = 0;   // N: valid in row lane 0, where the merge is
    if (t.ry == 0 && t.ok) {
        const size_t c = (size_t)a.c;
        int base = 0;
        for (int w = 0; w < a.world; ++w) {
            const float* p = a.rparts + (size_t)w * 3 * c + t.col;
            const float nB = p[0];   // (the columns of a rank share their count)
            float mB[VEC], qB[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) { mB[k] = p[c + k]; qB[k] = p[2 * c + k]; }
            if (w < a.rank) base += (int)nB;
            total += (int)nB;
            bn_chan<VEC>(cnt, mean, m2, nB, mB, qB);
        }
        if (t.tid == 0) {
            sbase = base;
            if (slab == 0 && blockIdx.x == 0) { a.meta[0] = base; a.meta[1] = total; }
        }
    }
    bn_finish_stats<VEC>(a, t, (float)total, mean, m2, slab == 0, sm);   // (its barrier also publishes sbase)
    float rstd[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { mean[k] = sm[0][t.cx * VEC + k]; rstd[k] = sm[1][t.cx * VEC + k]; }
    bn_apply_rows<VEC, XT, YT>(a, t, BnXPlain(), row0, row1, mean, rstd, a.T < kBnDropAll, sbase);
}

// this rank's (sum g, sum g * xhat, sum xhat) into its row of the rank partials, and as dbeta and dgamma. SMALL: from x and
// dy (n <= 256, the only launch); otherwise from the slab partials of bn_bwd_sums_k<.., 1>. One slab deep.
template <int VEC, typename XT, typename YT, int SMALL>
__global__ __launch_bounds__(kBnThreads) void bn_sync_bwd_sums_k(BnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kBnThreads * 3 * VEC];
    const BnCoord t = bn_coord<VEC>(a);
    float sg[VEC], sx[VEC], sh[VEC];
    if constexpr (SMALL) {
        const BnCols<VEC> q = bn_cols<VEC>(a, t);
        bn_slab_sums<VEC, XT, YT>(a, t, BnXPlain(), q, 0, a.n, sg, sx, sh, lds, a.meta[0]);
    } else {
        bn_sum_partials<VEC>(a, t, sg, sx, sh, lds);
    }
    bn_rank_put<VEC>(a, t, sg, sx, sh);
    if (t.ry == 0 && t.ok) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) { a.dbeta[t.col + k] = sg[k]; a.dgamma[t.col + k] = sx[k]; }
    }
}

// the gathered rank partials summed in rank order, then launch 2 of the plain backward with N rows. dgamma (when given):
// this rank's sum g * (xhat - mh) from its own row and the global mean of xhat, mh -- the shift the plain backward takes
// out of its dgamma; the ranks' values still add up to the whole batch's.
template <int VEC, typename XT, typename YT>
__global__ __launch_bounds__(kBnThreads) void bn_sync_bwd_dx_k(BnArgs a) {
    __shared__ float sm[3][kBnTileCols];
    const BnCoord t = bn_coord<VEC>(a);
    const BnCols<VEC> q = bn_cols<VEC>(a, t);
    const int slab = (int)blockIdx.y;
    const int row0 = slab * a.slab_rows, row1 = min(a.n, row0 + a.slab_rows);
    const int base = a.meta[0];
    const float fn = (float)a.meta[1];
    if (t.ry == 0 && t.ok) {
        const size_t c = (size_t)a.c;
        float sg[VEC], sx[VEC], sh[VEC], og[VEC], ox[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) { sg[k] = 0.f; sx[k] = 0.f; sh[k] = 0.f; og[k] = 0.f; ox[k] = 0.f; }
        for (int w = 0; w < a.world; ++w) {
            const float* p = a.rparts + (size_t)w * 3 * c + t.col;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float gB = p[k], xB = p[c + k];
                sg[k] = sg[k] + gB; sx[k] = sx[k] + xB; sh[k] = sh[k] + p[2 * c + k];
                if (w == a.rank) { og[k] = gB; ox[k] = xB; }
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float mh = sh[k] / fn;
            sm[0][t.cx * VEC + k] = sg[k];
            sm[1][t.cx * VEC + k] = sx[k] - mh * sg[k];
            sm[2][t.cx * VEC + k] = mh;
            if (slab == 0 && a.dgamma) a.dgamma[t.col + k] = ox[k] - mh * og[k];
        }
    }
    __syncthreads();
    bn_dx_rows<VEC, XT, YT>(a, t, BnXPlain(), q, row0, row1, fn, sm, base);
}

// a caller's row pointer allows the wide form: f32 x -> 4 columns per thread (f32 rows move as 16 bytes, bf16 rows as 8),
// bf16 x -> 8 columns per thread (16 bytes of bf16, two 16-byte pieces of f32)
inline bool bn_rows_aligned(const void* p, int bf16, int x_bf16) {
    return ((uintptr_t)p & ((bf16 && !x_bf16) ? 7u : 15u)) == 0;
}
inline bool bn_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// odd c or a pointer off a 32-bit word with bf16 storage: bf16 rows move as 32-bit words
inline bool bn_bf16_ok(const void* p, int bf16, int c) { return !bf16 || (c % 2 == 0 && ((uintptr_t)p & 3u) == 0); }

// one kernel family over (columns per thread, x's type, y's / dy's type): go(v, xt, yt) launches the member its tags name --
// v an integral constant, xt and yt a zero of the element type; 0 or the launch's hipError_t
template <int V>
using BnVec = std::integral_constant<int, V>;
template <typename F>
inline int bn_launch(int vec, int x_bf16, int y_bf16, F&& go) {
    if (!x_bf16) {
        if (!y_bf16) { if (vec == 4) go(BnVec<4>(), float(), float()); else go(BnVec<1>(), float(), float()); }
        else { if (vec == 4) go(BnVec<4>(), float(), bn_bf16()); else go(BnVec<1>(), float(), bn_bf16()); }
    } else {
        if (!y_bf16) { if (vec == 8) go(BnVec<8>(), bn_bf16(), float()); else go(BnVec<2>(), bn_bf16(), float()); }
        else { if (vec == 8) go(BnVec<8>(), bn_bf16(), bn_bf16()); else go(BnVec<2>(), bn_bf16(), bn_bf16()); }
    }
    MCCNN_LAUNCHED();
    return 0;
}

// what every mccnn_bn_sync_* entry checks of its shard before it looks at anything else; 0 or the error
inline int bn_sync_check(int n, int c, int rank, int world) {
    if (n < 1 || c < 1 || world < 1 || rank < 0 || rank >= world) return MCCNN_E_BADARG;
    if (n > (1 << 24)) return MCCNN_E_TOOLARGE;   // counts travel as f32
    return 0;
}

// a caller's rows and their type flag; the first of an entry's list is x (dx has x's type, and may be NULL: not wanted)
struct BnRows {
    const void* p;
    int bf16;
};

// What the entries share behind their own checks, in this order: the type flags, bf16 rows on 32-bit words, the workspace
// (need: its bytes, 0: the entry has none) -- 0 or the error -- then the plan from the row pointers and the workspace's, and
// what of `a` follows from it.
// wide: false takes the wide form away whatever the pointers of `rows` say (over a concatenation: a segment's width or pointer).
inline int bn_setup(BnArgs& a, BnPlan& p, int n, int c, std::initializer_list<BnRows> rows, size_t need = 0, void* ws = nullptr,
                    size_t ws_bytes = 0, bool wide = true) {
    const int x_bf16 = rows.begin()->bf16;
    int flags = 0;
    for (const BnRows& r : rows) flags |= r.bf16;
    if (flags & ~1) return MCCNN_E_BADARG;
    for (const BnRows& r : rows)
        if (!bn_bf16_ok(r.p, r.bf16, c)) return MCCNN_E_SHAPE;
    if (need && (!ws || ws_bytes < need)) return MCCNN_E_WORKSPACE;
    bool aligned = wide && (!need || bn_aligned16(ws));
    for (const BnRows& r : rows) aligned = aligned && bn_rows_aligned(r.p, r.bf16, x_bf16);
    p = bn_plan(n, c, aligned, x_bf16);
    a.part = (float*)ws;
    a.n = n; a.c = c; a.tw_log = p.tw_log; a.slab_rows = p.slab_rows; a.slabs = p.slabs; a.nparts = p.slabs;
    return 0;
}

}  // namespace mccnn

using namespace mccnn;

// The backward behind mccnn_bn_act_bwd_rows. shift (linear_bn.hip; NULL otherwise): [c], what the exact mean of a column has
// over saved's f32 one -- xhat is then ((x - mean) - shift) * rstd, the arithmetic of that file's forward
int mccnn::bn_act_bwd_impl(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, const float* gamma,
                           const float* beta, const float* saved, const float* shift, int relu, unsigned long long keep_threshold,
                           float keep_scale, unsigned seed, void* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                           mccnn_stream_t stream) {
    if (n < 1 || c < 1) return MCCNN_E_BADARG;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !dy || !gamma || !beta || !saved || !dgamma || !dbeta) return MCCNN_E_BADARG;
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_setup(a, p, n, c, {{x, x_bf16}, {dy, dy_bf16}, {dx, x_bf16}}, mccnn_bn_act_workspace_bytes(n, c), ws, ws_bytes))
        return e;
    a.x = x; a.dy = dy; a.out = dx; a.gamma = gamma; a.beta = beta; a.saved = const_cast<float*>(saved);
    a.dgamma = dgamma; a.dbeta = dbeta; a.shift = shift; a.relu = relu ? 1 : 0; a.want_dx = dx ? 1 : 0;
    a.keep_scale = keep_scale; a.seed = seed; a.T = keep_threshold;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs);
    if (n <= kBnSmallRows)
        return bn_launch(p.vec, x_bf16, dy_bf16, [&](auto v, auto xt, auto yt) {
            bn_bwd_dx_k<v(), decltype(xt), decltype(yt), 1><<<grid, kBnThreads, 0, st>>>(a);
        });
    if (const int e = bn_launch(p.vec, x_bf16, dy_bf16, [&](auto v, auto xt, auto yt) {
            bn_bwd_sums_k<v(), decltype(xt), decltype(yt)><<<grid, kBnThreads, 0, st>>>(a);
        }))
        return e;
    const dim3 grid2((unsigned)p.tiles, dx ? (unsigned)p.slabs : 1u);
    return bn_launch(p.vec, x_bf16, dy_bf16, [&](auto v, auto xt, auto yt) {
        bn_bwd_dx_k<v(), decltype(xt), decltype(yt), 0><<<grid2, kBnThreads, 0, st>>>(a);
    });
}

extern "C" {

size_t mccnn_bn_act_workspace_bytes(int n, int c) {
    if (n < 1 || c < 1 || n <= kBnSmallRows) return 0;
    return align_up((size_t)3 * (size_t)ceil_div(n, bn_slab_rows(n)) * (size_t)c * sizeof(float));
}

int mccnn_bn_act_fwd_rows(const void* x, int x_bf16, int n, int c, const float* gamma, const float* beta, float* moving_mean,
                          float* moving_var, float momentum, float eps, int training, int relu,
                          unsigned long long keep_threshold, float keep_scale, unsigned seed, void* y, int y_bf16,
                          float* saved, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || c < 1) return MCCNN_E_BADARG;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !gamma || !beta || !moving_mean || !moving_var || !y) return MCCNN_E_BADARG;
    if (training && !saved) return MCCNN_E_BADARG;
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_setup(a, p, n, c, {{x, x_bf16}, {y, y_bf16}}, training ? mccnn_bn_act_workspace_bytes(n, c) : 0, ws, ws_bytes))
        return e;
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.mov_mean = moving_mean; a.mov_var = moving_var; a.saved = saved;
    a.relu = relu ? 1 : 0; a.momentum = momentum; a.eps = eps; a.keep_scale = keep_scale; a.seed = seed;
    a.T = training ? keep_threshold : kBnDropAll;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs);
    if (!training)
        return bn_launch(p.vec, x_bf16, y_bf16, [&](auto v, auto xt, auto yt) {
            bn_apply_k<v(), decltype(xt), decltype(yt), 2><<<grid, kBnThreads, 0, st>>>(a);
        });
    if (n <= kBnSmallRows)
        return bn_launch(p.vec, x_bf16, y_bf16, [&](auto v, auto xt, auto yt) {
            bn_apply_k<v(), decltype(xt), decltype(yt), 1><<<grid, kBnThreads, 0, st>>>(a);
        });
    if (const int e = bn_launch(p.vec, x_bf16, 0, [&](auto v, auto xt, auto) {
            bn_stats_k<v(), decltype(xt)><<<grid, kBnThreads, 0, st>>>(a);
        }))
        return e;
    return bn_launch(p.vec, x_bf16, y_bf16, [&](auto v, auto xt, auto yt) {
        bn_apply_k<v(), decltype(xt), decltype(yt), 0><<<grid, kBnThreads, 0, st>>>(a);
    });
}

int mccnn_bn_act_bwd_rows(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, const float* gamma,
                          const float* beta, const float* saved, int relu, unsigned long long keep_threshold, float keep_scale,
                          unsigned seed, void* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                          mccnn_stream_t stream) {
    return bn_act_bwd_impl(x, x_bf16, dy, dy_bf16, n, c, gamma, beta, saved, nullptr, relu, keep_threshold, keep_scale, seed, dx,
                           dgamma, dbeta, ws, ws_bytes, stream);
}

// the float32 entries (ABI 18): the typed ones with both flags zero -- the same plan, kernels, launches and bytes
int mccnn_bn_act_fwd(const float* x, int n, int c, const float* gamma, const float* beta, float* moving_mean,
                     float* moving_var, float momentum, float eps, int training, int relu,
                     unsigned long long keep_threshold, float keep_scale, unsigned seed, float* y, float* saved, void* ws,
                     size_t ws_bytes, mccnn_stream_t stream) {
    return mccnn_bn_act_fwd_rows(x, 0, n, c, gamma, beta, moving_mean, moving_var, momentum, eps, training, relu, keep_threshold,
                                 keep_scale, seed, y, 0, saved, ws, ws_bytes, stream);
}

int mccnn_bn_act_bwd(const float* x, const float* dy, int n, int c, const float* gamma, const float* beta,
                     const float* saved, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                     float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    return mccnn_bn_act_bwd_rows(x, 0, dy, 0, n, c, gamma, beta, saved, relu, keep_threshold, keep_scale, seed, dx, dgamma, dbeta,
                                 ws, ws_bytes, stream);
}

// ---- over a column-wise concatenation (ABI 28; typed segments: ABI 30): the plan, launches and arithmetic of the f32-x
// entries at width C = sum c_s, whatever the segments' types; wherever that plan is the one the contiguous op takes on the
// concatenated (widened) tensor, the same bytes ----
}  // extern "C"

namespace mccnn {

// the family over (columns per thread, x's type -- float, or BnXSeg: the segment's, when one of them is bf16 -- and y's / dy's
// type): go(v, xt, yt) as in bn_launch
template <typename F>
inline int bn_cat_launch(int vec, bool typed, int y_bf16, F&& go) {
    if (!typed) {
        if (!y_bf16) { if (vec == 4) go(BnVec<4>(), float(), float()); else go(BnVec<1>(), float(), float()); }
        else { if (vec == 4) go(BnVec<4>(), float(), bn_bf16()); else go(BnVec<1>(), float(), bn_bf16()); }
    } else {
        if (!y_bf16) { if (vec == 4) go(BnVec<4>(), BnXSeg(), float()); else go(BnVec<1>(), BnXSeg(), float()); }
        else { if (vec == 4) go(BnVec<4>(), BnXSeg(), bn_bf16()); else go(BnVec<1>(), BnXSeg(), bn_bf16()); }
    }
    MCCNN_LAUNCHED();
    return 0;
}

// what the table of a call says beside the table itself
struct BnCatCall {
    int c;         // C
    bool wide;     // every width and every segment pointer allows 4 columns per thread (bn_cat_rows_wide)
    bool any_dx;   // some gradient is wanted
    bool typed;    // some segment is bf16: the BnXSeg instantiations
    bool odd;      // a bf16 x_s or wanted dx_s off a 2-byte boundary
};

// The segments of a call, checked, as the table the kernels take: 0 or the error. xs_bf16: NULL (all f32), or per segment
// whether its rows are bf16; dxs: NULL, or per segment where its gradient goes (NULL: not wanted).
inline int bn_cat_table(BnCat& s, BnCatCall& k, const void* const* xs, const int* xs_bf16, const int* cs, int nseg, int n,
                        void* const* dxs) {
    k = BnCatCall();
    if (nseg < 1 || nseg > kBnCatMax || n < 1 || !xs || !cs) return MCCNN_E_BADARG;
    for (int i = 0; i < nseg; ++i)
        if (cs[i] < 1 || !xs[i] || (xs_bf16 && (xs_bf16[i] & ~1))) return MCCNN_E_BADARG;
    if (bn_cat_fill(s, cs, nseg) > 0x7fffffffll) return MCCNN_E_TOOLARGE;
    k.c = s.col0[kBnCatMax];
    k.wide = bn_cat_rows_wide(xs, xs_bf16, cs, nseg, dxs);
    k.typed = bn_cat_set_types(s, xs_bf16, nseg);
    for (int i = 0; i < kBnCatMax; ++i) {
        const int from = i < nseg ? i : 0;
        s.x[i] = xs[from];
        s.dx[i] = dxs ? dxs[from] : nullptr;
        if (i < nseg) {
            k.any_dx = k.any_dx || s.dx[i];
            if ((s.bf16 >> i) & 1u) k.odd = k.odd || (((uintptr_t)s.x[i] | (uintptr_t)s.dx[i]) & 1u);
        }
    }
    return 0;
}

// the rest of what the two entries share: the plan at (n, C) from y's / dy's rows and the workspace, always the f32-x one
inline int bn_cat_setup(BnArgs& a, BnPlan& p, const BnCatCall& k, int n, const void* y, int y_bf16, size_t need, void* ws,
                        size_t ws_bytes) {
    const int e = bn_setup(a, p, n, k.c, {{nullptr, 0}, {y, y_bf16}}, need, ws, ws_bytes, k.wide);
    if (e == MCCNN_E_BADARG) return e;
    if (k.odd) return MCCNN_E_SHAPE;
    return e;
}

}  // namespace mccnn

extern "C" {

int mccnn_bn_act_cat_max_segments(void) { return kBnCatMax; }

int mccnn_bn_act_cat_fwd_rows(const void* const* xs, const int* xs_bf16, const int* cs, int nseg, int n, const float* gamma,
                              const float* beta, float* moving_mean, float* moving_var, float momentum, float eps, int training,
                              int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed, void* y, int y_bf16,
                              float* saved, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    BnCat s = {};
    BnCatCall k;
    const int table = bn_cat_table(s, k, xs, xs_bf16, cs, nseg, n, nullptr);
    if (table == MCCNN_E_BADARG) return table;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!gamma || !beta || !moving_mean || !moving_var || !y) return MCCNN_E_BADARG;
    if (training && !saved) return MCCNN_E_BADARG;
    if (table) return table;   // (C past 2^31 - 1: behind the other argument errors)
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_cat_setup(a, p, k, n, y, y_bf16, training ? mccnn_bn_act_workspace_bytes(n, k.c) : 0, ws, ws_bytes)) return e;
    a.out = y; a.gamma = gamma; a.beta = beta; a.mov_mean = moving_mean; a.mov_var = moving_var; a.saved = saved;
    a.relu = relu ? 1 : 0; a.momentum = momentum; a.eps = eps; a.keep_scale = keep_scale; a.seed = seed;
    a.T = training ? keep_threshold : kBnDropAll;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs);
    if (!training)
        return bn_cat_launch(p.vec, k.typed, y_bf16, [&](auto v, auto xt, auto yt) {
            bn_apply_k<v(), decltype(xt), decltype(yt), 2><<<grid, kBnThreads, 0, st>>>(a, s);
        });
    if (n <= kBnSmallRows)
        return bn_cat_launch(p.vec, k.typed, y_bf16, [&](auto v, auto xt, auto yt) {
            bn_apply_k<v(), decltype(xt), decltype(yt), 1><<<grid, kBnThreads, 0, st>>>(a, s);
        });
    if (const int e = bn_cat_launch(p.vec, k.typed, 0, [&](auto v, auto xt, auto) {
            bn_stats_k<v(), decltype(xt)><<<grid, kBnThreads, 0, st>>>(a, s);
        }))
        return e;
    return bn_cat_launch(p.vec, k.typed, y_bf16, [&](auto v, auto xt, auto yt) {
        bn_apply_k<v(), decltype(xt), decltype(yt), 0><<<grid, kBnThreads, 0, st>>>(a, s);
    });
}

int mccnn_bn_act_cat_bwd_rows(const void* const* xs, const int* xs_bf16, const int* cs, int nseg, const void* dy, int dy_bf16, int n,
                              const float* gamma, const float* beta, const float* saved, int relu,
                              unsigned long long keep_threshold, float keep_scale, unsigned seed, void* const* dxs, float* dgamma,
                              float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    BnCat s = {};
    BnCatCall k;
    const int table = bn_cat_table(s, k, xs, xs_bf16, cs, nseg, n, dxs);
    if (table == MCCNN_E_BADARG) return table;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!dy || !gamma || !beta || !saved || !dgamma || !dbeta) return MCCNN_E_BADARG;
    if (table) return table;
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_cat_setup(a, p, k, n, dy, dy_bf16, mccnn_bn_act_workspace_bytes(n, k.c), ws, ws_bytes)) return e;
    a.dy = dy; a.gamma = gamma; a.beta = beta; a.saved = const_cast<float*>(saved);
    a.dgamma = dgamma; a.dbeta = dbeta; a.relu = relu ? 1 : 0; a.want_dx = k.any_dx ? 1 : 0;
    a.keep_scale = keep_scale; a.seed = seed; a.T = keep_threshold;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs);
    if (n <= kBnSmallRows)
        return bn_cat_launch(p.vec, k.typed, dy_bf16, [&](auto v, auto xt, auto yt) {
            bn_bwd_dx_k<v(), decltype(xt), decltype(yt), 1><<<grid, kBnThreads, 0, st>>>(a, s);
        });
    if (const int e = bn_cat_launch(p.vec, k.typed, dy_bf16, [&](auto v, auto xt, auto yt) {
            bn_bwd_sums_k<v(), decltype(xt), decltype(yt)><<<grid, kBnThreads, 0, st>>>(a, s);
        }))
        return e;
    const dim3 grid2((unsigned)p.tiles, k.any_dx ? (unsigned)p.slabs : 1u);
    return bn_cat_launch(p.vec, k.typed, dy_bf16, [&](auto v, auto xt, auto yt) {
        bn_bwd_dx_k<v(), decltype(xt), decltype(yt), 0><<<grid2, kBnThreads, 0, st>>>(a, s);
    });
}

// the float32-segment entries (ABI 28): the typed ones without flags -- the same plan, kernels, launches and bytes
int mccnn_bn_act_cat_fwd(const float* const* xs, const int* cs, int nseg, int n, const float* gamma, const float* beta,
                         float* moving_mean, float* moving_var, float momentum, float eps, int training, int relu,
                         unsigned long long keep_threshold, float keep_scale, unsigned seed, void* y, int y_bf16, float* saved,
                         void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    return mccnn_bn_act_cat_fwd_rows((const void* const*)xs, nullptr, cs, nseg, n, gamma, beta, moving_mean, moving_var, momentum, eps,
                                     training, relu, keep_threshold, keep_scale, seed, y, y_bf16, saved, ws, ws_bytes, stream);
}

int mccnn_bn_act_cat_bwd(const float* const* xs, const int* cs, int nseg, const void* dy, int dy_bf16, int n, const float* gamma,
                         const float* beta, const float* saved, int relu, unsigned long long keep_threshold, float keep_scale,
                         unsigned seed, float* const* dxs, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                         mccnn_stream_t stream) {
    return mccnn_bn_act_cat_bwd_rows((const void* const*)xs, nullptr, cs, nseg, dy, dy_bf16, n, gamma, beta, saved, relu,
                                     keep_threshold, keep_scale, seed, (void* const*)dxs, dgamma, dbeta, ws, ws_bytes, stream);
}

// ---- statistics across ranks (ABI 22): the four stages around the caller's two collectives ----
int mccnn_bn_sync_stats(const void* x, int x_bf16, int n, int c, int rank, int world, float* parts, void* ws, size_t ws_bytes,
                        mccnn_stream_t stream) {
    if (const int e = bn_sync_check(n, c, rank, world)) return e;
    if (!x || !parts) return MCCNN_E_BADARG;
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_setup(a, p, n, c, {{x, x_bf16}}, mccnn_bn_act_workspace_bytes(n, c), ws, ws_bytes)) return e;
    a.x = x; a.rparts = parts; a.rank = rank; a.world = world;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs), one((unsigned)p.tiles, 1u);
    if (n <= kBnSmallRows)
        return bn_launch(p.vec, x_bf16, 0, [&](auto v, auto xt, auto) {
            bn_sync_stats_k<v(), decltype(xt), 1><<<one, kBnThreads, 0, st>>>(a);
        });
    if (const int e = bn_launch(p.vec, x_bf16, 0, [&](auto v, auto xt, auto) {
            bn_stats_k<v(), decltype(xt)><<<grid, kBnThreads, 0, st>>>(a);
        }))
        return e;
    return bn_launch(p.vec, x_bf16, 0, [&](auto v, auto xt, auto) {
        bn_sync_stats_k<v(), decltype(xt), 0><<<one, kBnThreads, 0, st>>>(a);
    });
}

int mccnn_bn_sync_apply(const void* x, int x_bf16, int n, int c, int rank, int world, const float* parts, const float* gamma,
                        const float* beta, float* moving_mean, float* moving_var, float momentum, float eps, int relu,
                        unsigned long long keep_threshold, float keep_scale, unsigned seed, void* y, int y_bf16, float* saved,
                        int* meta, mccnn_stream_t stream) {
    if (const int e = bn_sync_check(n, c, rank, world)) return e;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !parts || !gamma || !beta || !moving_mean || !moving_var || !y || !saved || !meta) return MCCNN_E_BADARG;
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_setup(a, p, n, c, {{x, x_bf16}, {y, y_bf16}})) return e;
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.mov_mean = moving_mean; a.mov_var = moving_var; a.saved = saved;
    a.rparts = const_cast<float*>(parts); a.meta = meta; a.relu = relu ? 1 : 0; a.rank = rank; a.world = world;
    a.momentum = momentum; a.eps = eps; a.keep_scale = keep_scale; a.seed = seed; a.T = keep_threshold;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs);
    return bn_launch(p.vec, x_bf16, y_bf16, [&](auto v, auto xt, auto yt) {
        bn_sync_apply_k<v(), decltype(xt), decltype(yt)><<<grid, kBnThreads, 0, st>>>(a);
    });
}

int mccnn_bn_sync_bwd_sums(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, int rank, int world,
                           const float* gamma, const float* beta, const float* saved, const int* meta, int relu,
                           unsigned long long keep_threshold, float keep_scale, unsigned seed, float* parts_b, float* dgamma,
                           float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (const int e = bn_sync_check(n, c, rank, world)) return e;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !dy || !gamma || !beta || !saved || !meta || !parts_b || !dgamma || !dbeta) return MCCNN_E_BADARG;
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_setup(a, p, n, c, {{x, x_bf16}, {dy, dy_bf16}}, mccnn_bn_act_workspace_bytes(n, c), ws, ws_bytes)) return e;
    a.x = x; a.dy = dy; a.gamma = gamma; a.beta = beta; a.saved = const_cast<float*>(saved);
    a.rparts = parts_b; a.meta = const_cast<int*>(meta); a.dgamma = dgamma; a.dbeta = dbeta;
    a.relu = relu ? 1 : 0; a.rank = rank; a.world = world; a.keep_scale = keep_scale; a.seed = seed; a.T = keep_threshold;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.slabs), one((unsigned)p.tiles, 1u);
    if (n <= kBnSmallRows)
        return bn_launch(p.vec, x_bf16, dy_bf16, [&](auto v, auto xt, auto yt) {
            bn_sync_bwd_sums_k<v(), decltype(xt), decltype(yt), 1><<<one, kBnThreads, 0, st>>>(a);
        });
    if (const int e = bn_launch(p.vec, x_bf16, dy_bf16, [&](auto v, auto xt, auto yt) {
            bn_bwd_sums_k<v(), decltype(xt), decltype(yt), 1><<<grid, kBnThreads, 0, st>>>(a);
        }))
        return e;
    return bn_launch(p.vec, x_bf16, dy_bf16, [&](auto v, auto xt, auto yt) {
        bn_sync_bwd_sums_k<v(), decltype(xt), decltype(yt), 0><<<one, kBnThreads, 0, st>>>(a);
    });
}

int mccnn_bn_sync_bwd_dx(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, int rank, int world,
                         const float* gamma, const float* beta, const float* parts_b, const float* saved, const int* meta,
                         int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed, void* dx, float* dgamma,
                         mccnn_stream_t stream) {
    if (const int e = bn_sync_check(n, c, rank, world)) return e;
    if (keep_threshold == 0 || keep_threshold > kBnDropAll) return MCCNN_E_BADARG;
    if (!x || !dy || !gamma || !beta || !parts_b || !saved || !meta || (!dx && !dgamma)) return MCCNN_E_BADARG;
    BnArgs a = {};
    BnPlan p;
    if (const int e = bn_setup(a, p, n, c, {{x, x_bf16}, {dy, dy_bf16}, {dx, x_bf16}})) return e;
    a.x = x; a.dy = dy; a.out = dx; a.gamma = gamma; a.beta = beta; a.saved = const_cast<float*>(saved);
    a.rparts = const_cast<float*>(parts_b); a.meta = const_cast<int*>(meta); a.dgamma = dgamma;
    a.relu = relu ? 1 : 0; a.want_dx = dx ? 1 : 0; a.rank = rank; a.world = world;
    a.keep_scale = keep_scale; a.seed = seed; a.T = keep_threshold;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, dx ? (unsigned)p.slabs : 1u);
    return bn_launch(p.vec, x_bf16, dy_bf16, [&](auto v, auto xt, auto yt) {
        bn_sync_bwd_dx_k<v(), decltype(xt), decltype(yt)><<<grid, kBnThreads, 0, st>>>(a);
    });
}

}  // extern "C"
