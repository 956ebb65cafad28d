// The optimiser step as one op (mccnn_adam_step): Adam with L2 decay in the gradient over many small tensors. Per element, in
// float32, with the tensor's step_size, bc2_sqrt, weight_decay and the call's beta1, beta2, eps, grad_scale:
//   g   = grad_scale * grad                      (skipped when grad_scale == 1.0f)
//   g   = weight_decay * p + g                   (skipped when weight_decay == 0.0f)
//   m'  = m + (1 - beta1) * (g - m)
//   v'  = beta2 * v + ((1 - beta2) * g) * g
//   den = sqrt(v') / bc2_sqrt + eps
//   p'  = p - step_size * (m' / den)
// p, m, v in place, grad only read. The library is compiled with -ffp-contract=off and correctly rounded divide / sqrt, so every
// operation above rounds once, in this order.
//   records   the tensors' records travel BY VALUE in the kernel arguments (the idiom of BatchBlocks / batch_item in common.h):
//             up to kAdamMax per launch, nothing is uploaded and no pointer table has to stay valid between steps.
//   mapping   a workgroup owns one chunk of kAdamChunk elements of one tensor and finds the tensor from the prefix of the
//             tensors' workgroup counts with an unrolled compare-and-add: the index is uniform, the record is read with
//             scalar loads from the kernel arguments.
//   accesses  16 bytes per lane where ALL FOUR pointers of the tensor are 16-byte aligned (a chunk starts a multiple of 16 bytes
//             behind them), one float per lane otherwise and for the last n % 4 elements: slices of one gradient buffer mostly
//             start on a 4-byte boundary only, and a neighbour begins right behind the last element.
// No atomics, no workspace, no memset, nothing read back: the same inputs give the same bytes.
//
// Clipping by the global gradient norm and the non-finite skip (mccnn_grad_norm, mccnn_adam_step_clipped) stand in front of it:
//   grad_sumsq_k        the record table and workgroup mapping of adam_k over g and n alone; a workgroup writes the sum of
//                       (grad_scale * g)^2 over its chunk as ONE float64 partial at partials[first chunk of the launch + block].
//   grad_clip_finish_k  one workgroup sums the partials in index order and writes the 16-byte record {norm, coef, skipped,
//                       skips + skipped} on the device (grad_clip.h has the scalar rule, which the host compiles too).
//   adam_k<true>        one wave-uniform 16-byte load of the record in the prologue; skipped: the whole grid returns before
//                       its first access to p, m, v; otherwise grad_scale' = float32(grad_scale * coef) takes grad_scale's place.
// Every partial is written before it is read (launch boundaries order them), nothing is zeroed, nothing is added atomically:
// the same inputs give the same bytes, record included.
//
// Accuracy of S = sum (grad_scale * g)^2, e = 2^-23, every rounding a factor (1 + d), |d| <= e / 2, all terms >= 0:
//   term      fl(fl(gs g)^2): the product's rounding counts twice in the square, the square's once            3 roundings
//   lane      a lane adds its terms in order, starting from the first term itself: at most 16 terms of the 16-byte or the
//             scalar sweep and, in the 16-byte sweep, one of the n % 4 tail elements behind them              16 roundings
//   tree      a fixed butterfly over the 64 lanes of a wave (6 levels), then (w0 + w1) + (w2 + w3)            8 roundings
//   partials  float64 from there on: 2^-53 per add, nothing beside the above
// so S is within 27 * e / 2 = 13.5 e, norm = float32(sqrt(S)) within 6.75 e + e / 2 (its own rounding) = 7.25 e of the exact
// value: under the 16 e the tests ask for. A square above FLT_MAX (|gs g| > 1.8e19) or a chunk sum above it is inf: the step
// reads as non-finite, nothing is rescaled. Squares below 2^-126 (|gs g| < 1.1e-19) are subnormal and carry absolute, not
// relative, accuracy: 2^-149 each.
#include <cmath>
#include "common.h"
#include "grad_clip.h"

namespace mccnn {

constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = 4096;   // elements of a workgroup (mccnn_amd.optim.CHUNK)
constexpr int kAdamMax = 76;       // records of a launch: 76 * 48 + 77 * 4 + 20 = 3976 bytes of kernel arguments

struct AdamArgs {
    mccnn_adam_tensor t[kAdamMax];
    int first[kAdamMax + 1];   // first[k] = first workgroup of record k; first[k] = the grid size from k = count on
    float omb1, beta2, omb2, eps, grad_scale;   // omb = 1 - beta (exact in float32 for beta >= 0.5)
    const mccnn_grad_record* record;            // adam_k<true> only: what mccnn_grad_norm left on the device
};
static_assert(sizeof(mccnn_adam_tensor) == 48, "the record is 48 bytes on both sides of the ABI");
static_assert(sizeof(AdamArgs) < 4096, "kernel arguments");
static_assert(sizeof(mccnn_grad_record) == 16, "the record is one 16-byte load");

struct AdamScalars {
    float step_size, bc2_sqrt, weight_decay, omb1, beta2, omb2, eps, grad_scale;
    bool scale, decay;
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamScalars& s) {
    if (s.scale) g = s.grad_scale * g;
    if (s.decay) g = s.weight_decay * p + g;
    m = m + s.omb1 * (g - m);
    v = s.beta2 * v + (s.omb2 * g) * g;
    const float den = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p - s.step_size * (m / den);
}

// REC: the call has a record (mccnn_adam_step_clipped). Without one the kernel is the plain step, argument for argument.
template <bool REC>
__global__ __launch_bounds__(kAdamThreads) void adam_k(AdamArgs a) {
    const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
    float grad_scale = a.grad_scale;
    if (REC) {
        const int4 r = *reinterpret_cast<const int4*>(a.record);   // the same address in every lane of the grid
        if (__builtin_amdgcn_readfirstlane(r.z) != 0) return;      // skipped: before the first access to p, m, v
        grad_scale = grad_scale * __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(r.y));
    }
    int k = 0;
#pragma unroll
    for (int i = 1; i < kAdamMax; ++i) k += blk >= a.first[i] ? 1 : 0;
    const mccnn_adam_tensor& t = a.t[k];
    const size_t base = (size_t)(blk - a.first[k]) * kAdamChunk;
    const int len = (int)min((size_t)kAdamChunk, (size_t)t.n - base);
    float* __restrict__ p = t.p + base;
    const float* __restrict__ g = t.g + base;
    float* __restrict__ m = t.m + base;
    float* __restrict__ v = t.v + base;
    AdamScalars s;
    s.step_size = t.step_size; s.bc2_sqrt = t.bc2_sqrt; s.weight_decay = t.weight_decay;
    s.omb1 = a.omb1; s.beta2 = a.beta2; s.omb2 = a.omb2; s.eps = a.eps; s.grad_scale = grad_scale;
    s.scale = grad_scale != 1.0f;
    s.decay = t.weight_decay != 0.0f;
    // every 16-byte access to a caller's pointer looks at the pointer's low bits first
    const bool wide = (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15u) == 0;
    int done = 0;
    if (wide) {
        const int quads = len >> 2;
        for (int q = tid; q < quads; q += kAdamThreads) {
            float4 pp = reinterpret_cast<const float4*>(p)[q];
            const float4 gg = reinterpret_cast<const float4*>(g)[q];
            float4 mm = reinterpret_cast<const float4*>(m)[q];
            float4 vv = reinterpret_cast<const float4*>(v)[q];
            adam_element(pp.x, gg.x, mm.x, vv.x, s);
            adam_element(pp.y, gg.y, mm.y, vv.y, s);
            adam_element(pp.z, gg.z, mm.z, vv.z, s);
            adam_element(pp.w, gg.w, mm.w, vv.w, s);
            reinterpret_cast<float4*>(p)[q] = pp;
            reinterpret_cast<float4*>(m)[q] = mm;
            reinterpret_cast<float4*>(v)[q] = vv;
        }
        done = quads << 2;
    }
    for (int i = done + tid; i < len; i += kAdamThreads) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_element(pp, g[i], mm, vv, s);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
}

// ---------------------------------------------------------------------------------------------------- the norm in front
struct GradArgs {
    const float* g[kAdamMax];
    int n[kAdamMax];
    int first[kAdamMax + 1];   // as AdamArgs::first
    float grad_scale;
    double* partials;          // of THIS launch: partials[blockIdx.x]
};
static_assert(sizeof(GradArgs) < 4096, "kernel arguments");

__device__ __forceinline__ float grad_sq(float g, float grad_scale) {
    const float x = grad_scale * g;
    return x * x;
}

__global__ __launch_bounds__(kAdamThreads) void grad_sumsq_k(GradArgs a) {
    __shared__ float waves[kAdamThreads / 64];
    const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
    int k = 0;
#pragma unroll
    for (int i = 1; i < kAdamMax; ++i) k += blk >= a.first[i] ? 1 : 0;
    const size_t base = (size_t)(blk - a.first[k]) * kAdamChunk;
    const int len = (int)min((size_t)kAdamChunk, (size_t)a.n[k] - base);
    const float* __restrict__ g = a.g[k] + base;
    const float gs = a.grad_scale;
    float acc = 0.0f;   // (0 + x is exact: the first term costs no rounding)
    int done = 0;
    if ((((uintptr_t)a.g[k]) & 15u) == 0) {   // a chunk starts a multiple of 16 bytes behind it
        const int quads = len >> 2;
        for (int q = tid; q < quads; q += kAdamThreads) {
            const float4 gg = reinterpret_cast<const float4*>(g)[q];
            acc += grad_sq(gg.x, gs);
            acc += grad_sq(gg.y, gs);
            acc += grad_sq(gg.z, gs);
            acc += grad_sq(gg.w, gs);
        }
        done = quads << 2;
    }
    for (int i = done + tid; i < len; i += kAdamThreads) acc += grad_sq(g[i], gs);
    // the fixed lane tree: a butterfly over the wave (every lane ends with the same bits), then the four waves
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((tid & 63) == 0) waves[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) a.partials[blk] = (double)((waves[0] + waves[1]) + (waves[2] + waves[3]));
}

__global__ __launch_bounds__(kAdamThreads) void grad_clip_finish_k(const double* __restrict__ partials, int count, float max_norm,
                                                                   int skip_nonfinite, mccnn_grad_record* record) {
    __shared__ double sums[kAdamThreads];
    const int tid = (int)threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < count; i += kAdamThreads) acc += partials[i];
    sums[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = kAdamThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) sums[tid] += sums[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const float norm = (float)sqrt(sums[0]);
        const int skipped = clip_skipped(norm, skip_nonfinite);
        int4 r;
        r.x = __builtin_bit_cast(int, norm);
        r.y = __builtin_bit_cast(int, clip_coef(norm, max_norm));
        r.z = skipped;
        r.w = record->skips + skipped;
        *reinterpret_cast<int4*>(record) = r;   // one 16-byte vector store
    }
}

inline bool adam_finite(float x) { return std::isfinite(x); }

// mccnn_adam_step and mccnn_adam_step_clipped: the same checks, the same launches; `record` selects the instantiation
static int adam_step(const mccnn_adam_tensor* tensors, int count, float beta1, float beta2, float eps, float grad_scale,
                     const mccnn_grad_record* record, hipStream_t st) {
    if (count < 0 || (count > 0 && !tensors)) return MCCNN_E_BADARG;
    if (!adam_finite(beta1) || !adam_finite(beta2) || !adam_finite(eps) || !adam_finite(grad_scale)) return MCCNN_E_BADARG;
    if (beta1 < 0.f || beta1 >= 1.f || beta2 < 0.f || beta2 >= 1.f || eps < 0.f) return MCCNN_E_BADARG;
    // pass 1: every record and every launch's grid, before anything is launched
    int live = 0;
    long long grid = 0;
    for (int i = 0; i < count; ++i) {
        const mccnn_adam_tensor& t = tensors[i];
        if (t.n < 0) return MCCNN_E_BADARG;
        if (t.n == 0) continue;   // (not part of any launch: its pointers and scalars are not looked at)
        if (!t.p || !t.g || !t.m || !t.v) return MCCNN_E_BADARG;
        if ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 3u) != 0) return MCCNN_E_BADARG;
        if (!adam_finite(t.step_size) || !adam_finite(t.bc2_sqrt) || !adam_finite(t.weight_decay)) return MCCNN_E_BADARG;
        if (t.bc2_sqrt <= 0.f) return MCCNN_E_BADARG;
        if (live % kAdamMax == 0) grid = 0;
        grid += ceil_div(t.n, kAdamChunk);
        if (grid >= (1ll << 31)) return MCCNN_E_TOOLARGE;
        ++live;
    }
    // pass 2: kAdamMax live records per launch
    AdamArgs a;
    a.omb1 = 1.0f - beta1; a.beta2 = beta2; a.omb2 = 1.0f - beta2; a.eps = eps; a.grad_scale = grad_scale;
    a.record = record;
    int have = 0;
    a.first[0] = 0;
    for (int i = 0; i <= count; ++i) {
        if (i < count && tensors[i].n > 0) {
            a.t[have] = tensors[i];
            a.first[have + 1] = a.first[have] + ceil_div(tensors[i].n, kAdamChunk);
            ++have;
        }
        if (have == kAdamMax || (i == count && have > 0)) {
            const int blocks = a.first[have];
            for (int k = have; k < kAdamMax; ++k) {
                a.t[k] = a.t[0];   // (never selected: no workgroup reaches first[k])
                a.first[k + 1] = blocks;
            }
            if (record) adam_k<true><<<(unsigned)blocks, kAdamThreads, 0, st>>>(a);
            else adam_k<false><<<(unsigned)blocks, kAdamThreads, 0, st>>>(a);
            MCCNN_LAUNCHED();
            have = 0;
        }
    }
    return MCCNN_OK;
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

int mccnn_adam_max_tensors(void) { return kAdamMax; }

int mccnn_adam_step(const mccnn_adam_tensor* tensors, int count, float beta1, float beta2, float eps, float grad_scale,
                    mccnn_stream_t stream) {
    return adam_step(tensors, count, beta1, beta2, eps, grad_scale, nullptr, (hipStream_t)stream);
}

int mccnn_adam_step_clipped(const mccnn_adam_tensor* tensors, int count, float beta1, float beta2, float eps, float grad_scale,
                            const mccnn_grad_record* record, mccnn_stream_t stream) {
    if (!record || (((uintptr_t)record) & 15u) != 0) return MCCNN_E_BADARG;
    return adam_step(tensors, count, beta1, beta2, eps, grad_scale, record, (hipStream_t)stream);
}

// the chunks of the live records, or -1 for a bad record (n < 0; n > 0 with a NULL or not 4-byte aligned g), -2 for 2^31 or more
static long long grad_chunks(const mccnn_adam_tensor* tensors, int count) {
    long long chunks = 0;
    for (int i = 0; i < count; ++i) {
        const mccnn_adam_tensor& t = tensors[i];
        if (t.n < 0) return -1;
        if (t.n == 0) continue;   // (nothing of it is looked at)
        if (!t.g || (((uintptr_t)t.g) & 3u) != 0) return -1;
        chunks += ceil_div(t.n, kAdamChunk);
        if (chunks >= (1ll << 31)) return -2;
    }
    return chunks;
}

size_t mccnn_grad_norm_ws(const mccnn_adam_tensor* tensors, int count) {
    if (count <= 0 || !tensors) return 0;
    const long long chunks = grad_chunks(tensors, count);
    return chunks > 0 ? (size_t)chunks * sizeof(double) : 0;
}

int mccnn_grad_norm(const mccnn_adam_tensor* tensors, int count, float grad_scale, float max_norm, int skip_nonfinite,
                    mccnn_grad_record* record, void* ws, size_t ws_bytes, mccnn_stream_t stream) {
    if (count < 0 || (count > 0 && !tensors)) return MCCNN_E_BADARG;
    if (!adam_finite(grad_scale) || !adam_finite(max_norm) || max_norm < 0.f) return MCCNN_E_BADARG;
    if (!record || (((uintptr_t)record) & 15u) != 0) return MCCNN_E_BADARG;
    const long long chunks = grad_chunks(tensors, count);
    if (chunks == -1) return MCCNN_E_BADARG;
    if (chunks == -2) return MCCNN_E_TOOLARGE;
    if (chunks == 0) return MCCNN_OK;   // no live tensor: nothing launched, the record stays
    if (!ws || ws_bytes < (size_t)chunks * sizeof(double)) return MCCNN_E_WORKSPACE;
    if ((((uintptr_t)ws) & 7u) != 0) return MCCNN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    double* partials = (double*)ws;
    GradArgs a;
    a.grad_scale = grad_scale;
    int have = 0;
    long long first_chunk = 0;
    a.first[0] = 0;
    for (int i = 0; i <= count; ++i) {
        if (i < count && tensors[i].n > 0) {
            a.g[have] = tensors[i].g;
            a.n[have] = tensors[i].n;
            a.first[have + 1] = a.first[have] + ceil_div(tensors[i].n, kAdamChunk);
            ++have;
        }
        if (have == kAdamMax || (i == count && have > 0)) {
            const int blocks = a.first[have];
            for (int k = have; k < kAdamMax; ++k) {
                a.g[k] = a.g[0];   // (never selected: no workgroup reaches first[k])
                a.n[k] = a.n[0];
                a.first[k + 1] = blocks;
            }
            a.partials = partials + first_chunk;
            grad_sumsq_k<<<(unsigned)blocks, kAdamThreads, 0, st>>>(a);
            MCCNN_LAUNCHED();
            first_chunk += blocks;
            have = 0;
        }
    }
    grad_clip_finish_k<<<1, kAdamThreads, 0, st>>>(partials, (int)chunks, max_norm, skip_nonfinite, record);
    MCCNN_LAUNCHED();
    return MCCNN_OK;
}

}  // extern "C"
