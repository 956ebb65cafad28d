// Segmentation scores on the device (mccnn_seg_counts_add): per cloud b and class c three int64 counts, added to by every call,
//   counts[b, c, 0] = I  rows with label c and prediction c             (intersection)
//   counts[b, c, 1] = U  rows with label c or prediction c              (union)
//   counts[b, c, 2] = G  rows with label c                              (ground truth)
// over the LIVE rows: 0 <= label < C, label != ignore_label, weight != 0 (the live rule of linear_xent.hip: -0.0f is 0, a NaN
// is not), 0 <= batch id < B. A dead row changes nothing; a bad batch id is a dead row, never clamped into another cloud. A
// prediction outside [0, C) on a live row is a miss of its label and touches nothing else.
//   one launch, grid-stride, kSegRows rows per workgroup and trip, the grid sized from n up to kSegMaxBlocks workgroups.
//   LDS table  B C 3 words <= kSegLdsBytes: a workgroup counts into its own uint32 [B, C, 3] table in LDS (a workgroup sees
//              fewer than 2^31 rows, so a word cannot wrap) and adds its non-zero words to counts at the end, one 64-bit
//              global atomic each. Clouds are contiguous in every loader, so a workgroup flushes few words.
//   no table   above that: every live row adds straight to counts with 64-bit global atomics.
//   loads      four rows per lane as one 16-byte load per input where every input pointer is 16-byte aligned; else (a view
//              that starts 4 bytes into its buffer) one row per lane and load, a wave reading 256 contiguous bytes. Rows past
//              n are never read: the last group of a vector lane is read row by row under a predicate.
// Integer atomics only: any arrival order gives the same bytes. No workspace, no memset.
#include "common.h"

namespace mccnn {

constexpr int kSegThreads = 256;
constexpr int kSegPerLane = 4;                             // rows of a lane per trip
constexpr int kSegRows = kSegThreads * kSegPerLane;        // rows of a workgroup per trip
constexpr int kSegMaxBlocks = 1024;                        // 4 workgroups per CU (four tables of 32 KB fit a CU's 160 KiB of LDS)
constexpr size_t kSegLdsBytes = 32 * 1024;                 // the table's budget

struct SegArgs {
    const int* pred;
    const int* labels;
    const float* rw;        // NULL: all 1
    const int* bid;         // NULL: every row is cloud 0
    unsigned long long* counts;
    int n, B, C, ignore, words;
};

// one row into the table (LDS: uint32 words) or into counts (global: uint64 words)
template <bool LDS>
__device__ __forceinline__ void seg_row(const SegArgs& a, unsigned* __restrict__ tab, int p, int l, float w, int b) {
    const bool live = (unsigned)l < (unsigned)a.C && l != a.ignore && w != 0.f && (unsigned)b < (unsigned)a.B;
    if (!live) return;
    const int row = b * a.C;                 // (b < B, l < C: every index below is < B C 3 < 2^31)
    const int at = (row + l) * 3;
    const bool hit = p == l;
    const bool other = !hit && (unsigned)p < (unsigned)a.C;
    if (LDS) {
        atomicAdd(&tab[at + 2], 1u);
        atomicAdd(&tab[at + 1], 1u);
        if (hit) atomicAdd(&tab[at], 1u);
        if (other) atomicAdd(&tab[(row + p) * 3 + 1], 1u);
    } else {
        atomicAdd(&a.counts[at + 2], 1ull);
        atomicAdd(&a.counts[at + 1], 1ull);
        if (hit) atomicAdd(&a.counts[at], 1ull);
        if (other) atomicAdd(&a.counts[(row + p) * 3 + 1], 1ull);
    }
}

template <bool LDS, bool VEC>
__global__ __launch_bounds__(kSegThreads) void seg_counts_k(SegArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned seg_tab[];
    const int tid = (int)threadIdx.x;
    if (LDS) {
        for (int k = tid; k < a.words; k += kSegThreads) seg_tab[k] = 0u;
        __syncthreads();
    }
    const long long n = a.n;
    const long long step = (long long)gridDim.x * kSegRows;
    for (long long base = (long long)blockIdx.x * kSegRows; base < n; base += step) {
        int p[kSegPerLane], l[kSegPerLane], b[kSegPerLane];
        float w[kSegPerLane];
        long long row[kSegPerLane];
        if (VEC) {
            // rows 4 t .. 4 t + 3 of the trip: base is a multiple of 1024 rows, so a 16-byte aligned pointer stays aligned
            const long long r0 = base + (long long)tid * kSegPerLane;
#pragma unroll
            for (int k = 0; k < kSegPerLane; ++k) row[k] = r0 + k;
            if (r0 + kSegPerLane <= n) {
                const int4 pv = *reinterpret_cast<const int4*>(a.pred + r0);
                const int4 lv = *reinterpret_cast<const int4*>(a.labels + r0);
                p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
                l[0] = lv.x; l[1] = lv.y; l[2] = lv.z; l[3] = lv.w;
                if (a.bid) {
                    const int4 bv = *reinterpret_cast<const int4*>(a.bid + r0);
                    b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w;
                } else {
                    b[0] = b[1] = b[2] = b[3] = 0;
                }
                if (a.rw) {
                    const float4 wv = *reinterpret_cast<const float4*>(a.rw + r0);
                    w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
                } else {
                    w[0] = w[1] = w[2] = w[3] = 1.0f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < kSegPerLane; ++k) {
                    const bool in = row[k] < n;
                    p[k] = in ? a.pred[row[k]] : 0;
                    l[k] = in ? a.labels[row[k]] : -1;
                    b[k] = (in && a.bid) ? a.bid[row[k]] : 0;
                    w[k] = (in && a.rw) ? a.rw[row[k]] : 1.0f;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kSegPerLane; ++k) {
                row[k] = base + (long long)k * kSegThreads + tid;
                const bool in = row[k] < n;
                p[k] = in ? a.pred[row[k]] : 0;
                l[k] = in ? a.labels[row[k]] : -1;
                b[k] = (in && a.bid) ? a.bid[row[k]] : 0;
                w[k] = (in && a.rw) ? a.rw[row[k]] : 1.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < kSegPerLane; ++k)
            if (row[k] < n) seg_row<LDS>(a, seg_tab, p[k], l[k], w[k], b[k]);
    }
    if (LDS) {
        __syncthreads();
        for (int k = tid; k < a.words; k += kSegThreads) {
            const unsigned v = seg_tab[k];
            if (v) atomicAdd(&a.counts[k], (unsigned long long)v);
        }
    }
}

// B C 3 < 2^31 (B, C >= 1; B C itself is below 2^62)
inline bool seg_sizes_ok(int B, int C) { return (long long)B * (long long)C <= ((1ll << 31) - 1) / 3; }
inline size_t seg_lds_bytes(int B, int C) {
    if (B < 1 || C < 1 || !seg_sizes_ok(B, C)) return 0;
    const size_t bytes = (size_t)B * (size_t)C * 3 * sizeof(unsigned);
    return bytes <= kSegLdsBytes ? bytes : 0;
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

size_t mccnn_seg_counts_lds_bytes(int num_clouds, int num_classes) { return seg_lds_bytes(num_clouds, num_classes); }

int mccnn_seg_counts_add(const int* pred, const int* labels, const float* row_weights, const int* batch_ids, int n, int num_clouds,
                         int num_classes, int ignore_label, long long* counts, mccnn_stream_t stream) {
    if (num_clouds < 1 || num_classes < 1 || n < 0) return MCCNN_E_BADARG;
    if (!pred || !labels || !counts) return MCCNN_E_BADARG;
    if (!seg_sizes_ok(num_clouds, num_classes)) return MCCNN_E_TOOLARGE;
    if (n == 0) return 0;
    SegArgs a = {};
    a.pred = pred; a.labels = labels; a.rw = row_weights; a.bid = batch_ids;
    a.counts = reinterpret_cast<unsigned long long*>(counts);   // (two's complement: an unsigned add is the signed add)
    a.n = n; a.B = num_clouds; a.C = num_classes;
    a.ignore = ignore_label < 0 ? -1 : ignore_label;
    a.words = num_clouds * num_classes * 3;
    const size_t lds = seg_lds_bytes(num_clouds, num_classes);
    const uintptr_t low = (uintptr_t)pred | (uintptr_t)labels | (uintptr_t)row_weights | (uintptr_t)batch_ids;   // (NULL: no bits)
    const bool vec = (low & 15u) == 0;
    const int trips = ceil_div(n, kSegRows);
    const unsigned blocks = (unsigned)(trips < kSegMaxBlocks ? trips : kSegMaxBlocks);
    hipStream_t st = (hipStream_t)stream;
    if (lds) {
        if (vec) seg_counts_k<true, true><<<blocks, kSegThreads, lds, st>>>(a);
        else seg_counts_k<true, false><<<blocks, kSegThreads, lds, st>>>(a);
    } else {
        if (vec) seg_counts_k<false, true><<<blocks, kSegThreads, 0, st>>>(a);
        else seg_counts_k<false, false><<<blocks, kSegThreads, 0, st>>>(a);
    }
    MCCNN_LAUNCHED();
    return 0;
}

}  // extern "C"
