// The cosine-distance loss of normal estimation as one op (mccnn_cosine_loss_fwd / _bwd): over pred, target [n, c] float32,
//   sp = sum_j p_j^2, rp = 1 / sqrt(max(sp, eps)), u = p rp;   st, rt, v likewise from the target;   eps = 1e-12f
//   cos_i = sum_j u_j v_j,  l_i = 1 - cos_i,  a_i = 2 atan2(|u - v|, |u + v|)  (pi / 2 when both lengths are 0)
//   loss = sum_live rw_i l_i / D,  cosSum = sum_live cos_i,  angleSum = sum_live a_i,  D = max(live rows, 1)
// A row is live when its weight is not 0 (no weights: every row). Every sum over j runs ascending as one fmaf chain.
//   forward   one lane per row, kCosAhead rows of a lane in flight: a wave's lanes read neighbouring rows, so a wave reads
//             one contiguous run of 64 c floats whatever c is (rows of 12 bytes are never 16-byte aligned: plain dword
//             loads, no alignment rule). Rows of up to four columns live in registers (one body per width); wider rows are
//             read again per pass from L1. A lane adds its rows in row order, a wave adds its lanes in a butterfly, the
//             workgroup's four waves are added in wave order, the slabs in slab order by the second launch. One launch up
//             to 256 rows, two above.
//   backward  one launch, row-local: it recomputes sp, st and cos and writes
//             dpred_j = -s rp (v_j - cos u_j)  (sp >= eps),  -s 1e6 v_j  (sp < eps: the clamp makes u linear in p),  0 on
//             dead rows, with s = g rw_i / D and g read from a device word.
// No atomics, no tickets, no memset, fixed merge orders: the same inputs give the same bytes.
#include <type_traits>
#include "common.h"

namespace mccnn {

constexpr int kCosThreads = 256;
constexpr int kCosOneRows = 256;     // up to here one workgroup does the whole forward
constexpr int kCosMaxSlabs = 1024;   // forward workgroups (= partials the second launch merges)
constexpr int kCosAhead = 4;         // rows of a lane in flight
constexpr float kCosEps = 1e-12f;    // tf.nn.l2_normalize's epsilon
constexpr float kCosHalfPi = 1.57079632679489661923f;

struct CosFwdArgs {
    const float* p;
    const float* t;
    const float* rw;     // NULL: all 1
    float* loss;
    float* sums;         // cosSum, angleSum
    int* meta;           // D
    float* part;         // more than one slab: [slabs] sum rw l, [slabs] sum cos, [slabs] sum angle, [slabs] live rows as ints
    int n, c, slab_rows, slabs;
};

struct CosBwdArgs {
    const float* p;
    const float* t;
    const float* rw;
    const int* meta;
    const float* g;      // the gradient of loss: one device word
    float* dp;
    int n, c;
};

// A row of pred and of target: C columns in registers (C >= 1), or C == 0: c columns read where they lie.
template <int C>
struct CosRow {
    float p[C], t[C];
    __device__ __forceinline__ void load(const float* __restrict__ pp, const float* __restrict__ tp, int) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            p[j] = pp[j];
            t[j] = tp[j];
        }
    }
    __device__ __forceinline__ void none() {
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = t[j] = 0.f;
    }
    __device__ __forceinline__ float P(int j) const { return p[j]; }
    __device__ __forceinline__ float T(int j) const { return t[j]; }
    __device__ __forceinline__ int cols() const { return C; }
};
template <>
struct CosRow<0> {
    const float* p;
    const float* t;
    int c;
    __device__ __forceinline__ void load(const float* __restrict__ pp, const float* __restrict__ tp, int cc) {
        p = pp;
        t = tp;
        c = cc;
    }
    __device__ __forceinline__ void none() {
        p = t = nullptr;
        c = 0;
    }
    __device__ __forceinline__ float P(int j) const { return p[j]; }
    __device__ __forceinline__ float T(int j) const { return t[j]; }
    __device__ __forceinline__ int cols() const { return c; }
};

// rp, rt and sp of a row
template <int C>
__device__ __forceinline__ void cos_norms(const CosRow<C>& r, float& sp, float& rp, float& rt) {
    sp = 0.f;
    float st = 0.f;
    const int c = r.cols();
    constexpr int kU = C ? C : 1;   // (rows in registers: unrolled; read in place: a plain loop)
#pragma unroll kU
    for (int j = 0; j < c; ++j) {
        sp = __builtin_fmaf(r.P(j), r.P(j), sp);
        st = __builtin_fmaf(r.T(j), r.T(j), st);
    }
    rp = 1.0f / sqrtf(fmaxf(sp, kCosEps));
    rt = 1.0f / sqrtf(fmaxf(st, kCosEps));
}

template <int C>
__device__ __forceinline__ void cos_row_fwd(const CosRow<C>& r, float& cosv, float& ang) {
    float sp, rp, rt;
    cos_norms(r, sp, rp, rt);
    float cs = 0.f, sd = 0.f, ss = 0.f;
    const int c = r.cols();
    constexpr int kU = C ? C : 1;   // (rows in registers: unrolled; read in place: a plain loop)
#pragma unroll kU
    for (int j = 0; j < c; ++j) {
        const float u = r.P(j) * rp, v = r.T(j) * rt;
        const float d = u - v, s = u + v;
        cs = __builtin_fmaf(u, v, cs);
        sd = __builtin_fmaf(d, d, sd);
        ss = __builtin_fmaf(s, s, ss);
    }
    cosv = cs;
    ang = (sd == 0.f && ss == 0.f) ? kCosHalfPi : 2.0f * atan2f(sqrtf(sd), sqrtf(ss));
}

__device__ __forceinline__ void cos_finish(float wl, float cs, float as, int live, float* loss, float* sums, int* meta) {
    const int D = live > 1 ? live : 1;
    loss[0] = wl / (float)D;   // (no live row: +0 / 1)
    sums[0] = cs;
    sums[1] = as;
    meta[0] = D;
}

// the 64 lanes of a wave: a butterfly (an IEEE sum does not depend on the side a term stands on, so every lane ends with
// the same bytes)
__device__ __forceinline__ float cos_wave_sum(float v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int cos_wave_sum(int v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

template <int C>
__global__ __launch_bounds__(kCosThreads) void cos_fwd_k(CosFwdArgs a) {
    __shared__ float red_f[3][kCosThreads / 64];
    __shared__ int red_n[kCosThreads / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = (int)blockIdx.x;
    const long long row0 = (long long)slab * a.slab_rows;
    const long long row1 = row0 + a.slab_rows < (long long)a.n ? row0 + a.slab_rows : (long long)a.n;
    float wl = 0.f, cs = 0.f, as = 0.f;
    int live = 0;
    for (long long base = row0; base < row1; base += (long long)kCosAhead * kCosThreads) {
        CosRow<C> r[kCosAhead];
        float rw[kCosAhead];
#pragma unroll
        for (int k = 0; k < kCosAhead; ++k) {
            const long long row = base + (long long)k * kCosThreads + tid;
            rw[k] = 0.f;   // (a row past the slab's end is a dead row: neither computed nor added)
            if (row < row1) {
                rw[k] = a.rw ? a.rw[row] : 1.0f;
                r[k].load(a.p + (size_t)row * a.c, a.t + (size_t)row * a.c, a.c);
            } else {
                r[k].none();
            }
        }
#pragma unroll
        for (int k = 0; k < kCosAhead; ++k) {
            const long long row = base + (long long)k * kCosThreads + tid;
            if (row < row1 && rw[k] != 0.f) {
                float cv, av;
                cos_row_fwd(r[k], cv, av);
                wl = __builtin_fmaf(rw[k], 1.0f - cv, wl);
                cs = cs + cv;
                as = as + av;
                ++live;
            }
        }
    }
    wl = cos_wave_sum(wl);
    cs = cos_wave_sum(cs);
    as = cos_wave_sum(as);
    live = cos_wave_sum(live);
    if (lane == 0) {
        red_f[0][wave] = wl;
        red_f[1][wave] = cs;
        red_f[2][wave] = as;
        red_n[wave] = live;
    }
    __syncthreads();
    if (tid == 0) {
        wl = cs = as = 0.f;
        live = 0;
        for (int k = 0; k < kCosThreads / 64; ++k) {
            wl = wl + red_f[0][k];
            cs = cs + red_f[1][k];
            as = as + red_f[2][k];
            live += red_n[k];
        }
        if (a.slabs == 1) {
            cos_finish(wl, cs, as, live, a.loss, a.sums, a.meta);
        } else {
            a.part[slab] = wl;
            a.part[a.slabs + slab] = cs;
            a.part[2 * a.slabs + slab] = as;
            reinterpret_cast<int*>(a.part + 3 * a.slabs)[slab] = live;
        }
    }
}

// forward, launch 2 (more than one slab): one workgroup; thread t adds its run of consecutive slabs, then the waves' lanes
// and the four waves as the first launch does
__global__ __launch_bounds__(kCosThreads) void cos_merge_k(const float* __restrict__ part, int slabs, float* __restrict__ loss,
                                                           float* __restrict__ sums, int* __restrict__ meta) {
    __shared__ float red_f[3][kCosThreads / 64];
    __shared__ int red_n[kCosThreads / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* pi = reinterpret_cast<const int*>(part + 3 * slabs);
    const int per = (slabs + kCosThreads - 1) / kCosThreads;
    const int s0 = min(slabs, tid * per), s1 = min(slabs, s0 + per);
    float wl = 0.f, cs = 0.f, as = 0.f;
    int live = 0;
    for (int s = s0; s < s1; ++s) {
        wl = wl + part[s];
        cs = cs + part[slabs + s];
        as = as + part[2 * slabs + s];
        live += pi[s];
    }
    wl = cos_wave_sum(wl);
    cs = cos_wave_sum(cs);
    as = cos_wave_sum(as);
    live = cos_wave_sum(live);
    if (lane == 0) {
        red_f[0][wave] = wl;
        red_f[1][wave] = cs;
        red_f[2][wave] = as;
        red_n[wave] = live;
    }
    __syncthreads();
    if (tid == 0) {
        wl = cs = as = 0.f;
        live = 0;
        for (int k = 0; k < kCosThreads / 64; ++k) {
            wl = wl + red_f[0][k];
            cs = cs + red_f[1][k];
            as = as + red_f[2][k];
            live += red_n[k];
        }
        cos_finish(wl, cs, as, live, loss, sums, meta);
    }
}

// backward: one lane per row
template <int C>
__global__ __launch_bounds__(kCosThreads) void cos_bwd_k(CosBwdArgs a) {
    const long long row = (long long)blockIdx.x * kCosThreads + (int)threadIdx.x;
    if (row >= a.n) return;
    const float rw = a.rw ? a.rw[row] : 1.0f;
    float* __restrict__ dp = a.dp + (size_t)row * a.c;
    CosRow<C> r;
    r.load(a.p + (size_t)row * a.c, a.t + (size_t)row * a.c, a.c);
    const int c = r.cols();
    constexpr int kU = C ? C : 1;   // (rows in registers: unrolled; read in place: a plain loop)
    if (rw == 0.f) {
#pragma unroll kU
        for (int j = 0; j < c; ++j) dp[j] = 0.f;
        return;
    }
    const float s = a.g[0] * rw / (float)a.meta[0];
    float sp, rp, rt;
    cos_norms(r, sp, rp, rt);
    if (sp >= kCosEps) {
        float cs = 0.f;
#pragma unroll kU
        for (int j = 0; j < c; ++j) cs = __builtin_fmaf(r.P(j) * rp, r.T(j) * rt, cs);
        const float k = -s * rp;
#pragma unroll kU
        for (int j = 0; j < c; ++j) {
            const float u = r.P(j) * rp, v = r.T(j) * rt;
            dp[j] = k * (v - cs * u);
        }
    } else {
        const float k = -s * 1e6f;
#pragma unroll kU
        for (int j = 0; j < c; ++j) dp[j] = k * (r.T(j) * rt);
    }
}

inline bool cos_sizes_ok(int n, int c) { return (long long)n * (long long)c < (1ll << 31); }
inline int cos_slab_rows(int n) {
    if (n <= kCosOneRows) return kCosOneRows;
    return kCosThreads * ceil_div(ceil_div(n, kCosThreads), kCosMaxSlabs);
}
inline size_t cos_part_bytes(int n) {
    const int slabs = ceil_div(n, cos_slab_rows(n));
    if (slabs == 1) return 0;
    return align_up((size_t)4 * (size_t)slabs * sizeof(float));
}

template <typename F>
inline void cos_by_width(int c, F&& go) {
    switch (c) {
        case 1: go(std::integral_constant<int, 1>()); break;
        case 2: go(std::integral_constant<int, 2>()); break;
        case 3: go(std::integral_constant<int, 3>()); break;
        case 4: go(std::integral_constant<int, 4>()); break;
        default: go(std::integral_constant<int, 0>()); break;
    }
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

size_t mccnn_cosine_loss_workspace_bytes(int n, int c) {
    if (n < 1 || c < 1 || !cos_sizes_ok(n, c)) return 0;
    return cos_part_bytes(n);
}

int mccnn_cosine_loss_fwd(const float* pred, const float* target, int n, int c, const float* row_weights, float* loss, float* sums,
                          int* meta, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (n < 1 || c < 1) return MCCNN_E_BADARG;
    if (!pred || !target || !loss || !sums || !meta) return MCCNN_E_BADARG;
    if (!cos_sizes_ok(n, c)) return MCCNN_E_TOOLARGE;
    const size_t need = cos_part_bytes(n);
    if (need && (!ws || ws_bytes < need)) return MCCNN_E_WORKSPACE;
    CosFwdArgs a = {};
    a.p = pred; a.t = target; a.rw = row_weights; a.loss = loss; a.sums = sums; a.meta = meta; a.part = (float*)ws;
    a.n = n; a.c = c;
    a.slab_rows = cos_slab_rows(n);
    a.slabs = ceil_div(n, a.slab_rows);
    if (a.slabs > kCosMaxSlabs) return MCCNN_E_TOOLARGE;   // (the slab rule keeps to it for every n an int holds)
    hipStream_t st = (hipStream_t)stream;
    cos_by_width(c, [&](auto w) { cos_fwd_k<decltype(w)::value><<<(unsigned)a.slabs, kCosThreads, 0, st>>>(a); });
    MCCNN_LAUNCHED();
    if (a.slabs > 1) {
        cos_merge_k<<<1, kCosThreads, 0, st>>>(a.part, a.slabs, loss, sums, meta);
        MCCNN_LAUNCHED();
    }
    return 0;
}

int mccnn_cosine_loss_bwd(const float* pred, const float* target, int n, int c, const float* row_weights, const int* meta,
                          const float* loss_grad, float* dpred, mccnn_stream_t stream) {
    if (n < 1 || c < 1) return MCCNN_E_BADARG;
    if (!pred || !target || !meta || !loss_grad || !dpred) return MCCNN_E_BADARG;
    if (!cos_sizes_ok(n, c)) return MCCNN_E_TOOLARGE;
    CosBwdArgs a = {};
    a.p = pred; a.t = target; a.rw = row_weights; a.meta = meta; a.g = loss_grad; a.dp = dpred;
    a.n = n; a.c = c;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)ceil_div(n, kCosThreads);
    cos_by_width(c, [&](auto w) { cos_bwd_k<decltype(w)::value><<<blocks, kCosThreads, 0, st>>>(a); });
    MCCNN_LAUNCHED();
    return 0;
}

}  // extern "C"
