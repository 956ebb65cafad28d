// What linear_bn.hip and linear_xent.hip share: the GEMM body on the f32-input matrix cores (lin_tile: a 64 x 64 output tile of
// a workgroup of 4 waves, A and B through LDS in chunks of 32 k, a fixed k order per element), the kernel around it for
// dx = dz W^T and dW = x^T dz (lin_mm_k), the merge of the dW / db slabs and the plan that splits them.
#pragma once
#include "common.h"

namespace mccnn {

constexpr int kLinThreads = 256;
constexpr int kLinTile = 64;        // rows and columns of a workgroup's output tile
constexpr int kLinKC = 32;          // k of a chunk in LDS
constexpr int kLinAS = 36;          // row stride of the A chunk [64][32]: 16-byte rows, the 64 reads of a wave on 64 banks
constexpr int kLinBS = 80;          // row stride of the B chunk [32][64]: the four k rows of a read 16 banks apart
constexpr int kLinDwSlabRows = 512; // rows of a dW slab ...
constexpr int kLinDwMaxSlabs = 64;  // ... until there would be more slabs than this ...
constexpr long long kLinDwMaxFloats = 4ll << 20;   // ... or more partial planes than 16 MiB

typedef float lin_f32x4 __attribute__((ext_vector_type(4)));

// acc += A[m0 .. m0 + 64, k0 .. k1) * B[k0 .. k1, c0 .. c0 + 64). TA: A[m][k] is a[k * lda + m], else a[m * lda + k];
// TB: B[k][c] is b[c * ldb + k], else b[k * ldb + c]. AV (only without TA): the rows of A move as 16-byte pieces -- a is on
// 16 bytes, lda % 4 == 0 and k1 % 4 == 0. after(kc): every thread calls it with the chunk in LDS.
template <bool TA, bool TB, bool AV, typename F>
__device__ __forceinline__ void lin_tile(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, int M, int N,
                                         int m0, int c0, int k0, int k1, float* as, float* bs, lin_f32x4 (&acc)[4], F&& after) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int kc = k0; kc < k1; kc += kLinKC) {
        __syncthreads();   // the chunk before this one has been read
        if constexpr (!TA && AV) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + kLinThreads * i, kq = e & 7, m = e >> 3;
                const int gm = m0 + m, gk = kc + 4 * kq;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gm < M && gk < k1) v = *reinterpret_cast<const float4*>(a + (size_t)gm * lda + gk);
                *reinterpret_cast<float4*>(as + m * kLinAS + 4 * kq) = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = tid + kLinThreads * i;
                const int m = TA ? (e & 63) : (e >> 5), k = TA ? (e >> 6) : (e & 31);
                const int gm = m0 + m, gk = kc + k;
                float v = 0.f;
                if (gm < M && gk < k1) v = TA ? a[(size_t)gk * lda + gm] : a[(size_t)gm * lda + gk];
                as[m * kLinAS + k] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + kLinThreads * i;
            const int c = TB ? (e >> 5) : (e & 63), k = TB ? (e & 31) : (e >> 6);
            const int gc = c0 + c, gk = kc + k;
            float v = 0.f;
            if (gc < N && gk < k1) v = TB ? b[(size_t)gc * ldb + gk] : b[(size_t)gk * ldb + gc];
            bs[k * kLinBS + c] = v;
        }
        __syncthreads();
        after(kc);
        const float* ar = as + (wave * 16 + (lane & 15)) * kLinAS + (lane >> 4);
        const float* br = bs + (lane >> 4) * kLinBS + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < kLinKC; kk += 4) {
            const float av = ar[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, br[kk * kLinBS + t * 16], acc[t], 0, 0, 0);
        }
    }
}

struct LinMmArgs {
    const float* a;
    const float* b;
    float* out;        // plane s at out + s * plane, [M, N] row-major
    float* colsum;     // DB: plane s at colsum + s * N
    int lda, ldb, M, N, K, kper;
    size_t plane;
};

// out[s] = A[:, k-slab s] * B[k-slab s, :]; grid (column tiles, row tiles, k slabs). DB: the first row of workgroups also
// writes the column sums of B over its k slab.
template <bool TA, bool TB, bool AV, bool DB>
__global__ __launch_bounds__(kLinThreads) void lin_mm_k(LinMmArgs a) {
    __shared__ __attribute__((aligned(16))) float as[kLinTile * kLinAS];
    __shared__ __attribute__((aligned(16))) float bs[kLinKC * kLinBS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)blockIdx.x * kLinTile, m0 = (int)blockIdx.y * kLinTile, s = (int)blockIdx.z;
    const int k0 = s * a.kper, k1 = min(a.K, k0 + a.kper);
    lin_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = lin_f32x4{0.f, 0.f, 0.f, 0.f};
    float cs = 0.f;
    const bool sums = DB && blockIdx.y == 0 && tid < kLinTile;
    lin_tile<TA, TB, AV>(a.a, a.lda, a.b, a.ldb, a.M, a.N, m0, c0, k0, k1, as, bs, acc, [&](int) {
        if constexpr (DB) {
            if (sums)
                for (int k = 0; k < kLinKC; ++k) cs = cs + bs[k * kLinBS + tid];   // (rows past k1 are zeros)
        }
    });
    float* o = a.out + (size_t)s * a.plane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + wave * 16 + 4 * (lane >> 4) + i;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = c0 + t * 16 + (lane & 15);
            if (row < a.M && c < a.N) o[(size_t)row * a.N + c] = acc[t][i];
        }
    }
    if constexpr (DB) {
        if (sums && c0 + tid < a.N) a.colsum[(size_t)s * a.N + c0 + tid] = cs;
    }
}

// dW and db: the partial planes added in slab order (static: a kernel of each file that includes this header)
static __global__ __launch_bounds__(kLinThreads) void lin_dw_merge_k(const float* __restrict__ pw, const float* __restrict__ pb,
                                                                     float* __restrict__ dw, float* __restrict__ db, int wn,
                                                                     int cout, int slabs) {
    const long long i = (long long)blockIdx.x * kLinThreads + threadIdx.x;
    if (i < wn) {
        float v = 0.f;
        for (int s = 0; s < slabs; ++s) v = v + pw[(size_t)s * wn + i];
        dw[i] = v;
    } else if (i < (long long)wn + cout) {
        const int j = (int)(i - wn);
        float v = 0.f;
        for (int s = 0; s < slabs; ++s) v = v + pb[(size_t)s * cout + j];
        db[j] = v;
    }
}

struct LinDwPlan {
    int slabs, kper;
};
inline LinDwPlan lin_dw_plan(int n, int cin, int cout) {
    const long long per = (long long)cin * cout + cout;
    long long s = ceil_div(n, kLinDwSlabRows);
    if (s > kLinDwMaxSlabs) s = kLinDwMaxSlabs;
    const long long fit = kLinDwMaxFloats / per;
    if (s > fit) s = fit;
    if (s < 1) s = 1;
    LinDwPlan p;
    p.kper = ceil_div(ceil_div(n, s), kLinKC) * kLinKC;
    p.slabs = ceil_div(n, p.kper);
    return p;
}
inline size_t lin_dz_bytes(int n, int cout) { return align_up((size_t)n * (size_t)cout * sizeof(float)); }
inline size_t lin_dw_bytes(int n, int cin, int cout) {
    const LinDwPlan p = lin_dw_plan(n, cin, cout);
    if (p.slabs == 1) return 0;
    return align_up((size_t)p.slabs * ((size_t)cin * cout + cout) * sizeof(float));
}
inline bool lin_sizes_ok(int n, int cin, int cout) {
    return ceil_div(n, kLinTile) <= 65535 && ceil_div(cin, kLinTile) <= 65535 && (long long)cin * cout + cout < (1ll << 31);
}
inline bool lin_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace mccnn
