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
#include <cmath>
#include "common.h"

namespace mccnn {

constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = 4096;   // elements of a workgroup (mccnn_amd.optim.CHUNK)
constexpr int kAdamMax = 76;       // records of a launch: 76 * 48 + 77 * 4 + 20 = 3976 bytes of kernel arguments

struct AdamArgs {
    mccnn_adam_tensor t[kAdamMax];
    int first[kAdamMax + 1];   // first[k] = first workgroup of record k; first[k] = the grid size from k = count on
    float omb1, beta2, omb2, eps, grad_scale;   // omb = 1 - beta (exact in float32 for beta >= 0.5)
};
static_assert(sizeof(mccnn_adam_tensor) == 48, "the record is 48 bytes on both sides of the ABI");
static_assert(sizeof(AdamArgs) < 4096, "kernel arguments");

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

__global__ __launch_bounds__(kAdamThreads) void adam_k(AdamArgs a) {
    const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
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
    s.omb1 = a.omb1; s.beta2 = a.beta2; s.omb2 = a.omb2; s.eps = a.eps; s.grad_scale = a.grad_scale;
    s.scale = a.grad_scale != 1.0f;
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

inline bool adam_finite(float x) { return std::isfinite(x); }

}  // namespace mccnn

using namespace mccnn;

extern "C" {

int mccnn_adam_max_tensors(void) { return kAdamMax; }

int mccnn_adam_step(const mccnn_adam_tensor* tensors, int count, float beta1, float beta2, float eps, float grad_scale,
                    mccnn_stream_t stream) {
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
    hipStream_t st = (hipStream_t)stream;
    AdamArgs a;
    a.omb1 = 1.0f - beta1; a.beta2 = beta2; a.omb2 = 1.0f - beta2; a.eps = eps; a.grad_scale = grad_scale;
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
            adam_k<<<(unsigned)blocks, kAdamThreads, 0, st>>>(a);
            MCCNN_LAUNCHED();
            have = 0;
        }
    }
    return MCCNN_OK;
}

}  // extern "C"
