// Voxel accuracy on the device (mccnn_voxel_acc_add): the per-voxel majority vote of ScanNet's own metric. Every live row
// belongs to the voxel (b, v_x, v_y, v_z) of a grid of `resolution` over its cloud's box minimum (voxel_key.h: v =
// ceilf((p - min) / res), dropped outside [0, 65535]); per occupied voxel the labels and the predictions of its rows are
// counted, ul / up are the lowest classes with the most labels / predictions, and a VALID voxel (the ignore label's share
// (double) g / (double) s below max_ignore_share, and ul != ignore_label) adds
//   counts[b, ul, 1] += 1  (G)      and, where ul == up,      counts[b, ul, 0] += 1  (V).
// A device hash table in the caller's workspace: cap slots (a power of two), per slot one uint64 key (0: empty) and a uint32
// [2, C] histogram; keys[cap] first, the histograms behind them.
//   vox_vote_k   grid-stride over the rows. A live row claims or finds its slot with a 64-bit atomicCAS(&keys[s], 0, key)
//                from the home slot hash & (cap - 1) on, linear probing: only the value the CAS returns decides (0 or key:
//                the slot is the row's; anything else: the next slot), so no thread ever waits for another thread's store
//                and every probe step is its own progress. A slot never empties within the launch, so a key settles in ONE
//                slot whatever the arrival order. Then one 32-bit atomicAdd for the label and one for a prediction in range.
//                The table is touched through agent-scope atomics only (the per-XCD L2s are not coherent for plain loads);
//                the kernel boundary is the only hand-off. Rows dropped for their coordinates are counted per workgroup, one
//                atomic each to `dropped`.
//   vox_score_k  one thread per slot and trip, grid-stride over the table: 8 trips per workgroup, 128 to 2048 workgroups. An
//                empty slot costs one 8-byte load; an occupied one reads its 2 C words, applies the rule, adds at most two
//                counts and writes zeros back over its key and histogram: the op leaves the workspace as the empty table it
//                needs next time (ws_clean = 1). Where B C 2 words fit 32 KB the counts of a workgroup are merged in LDS
//                first and its non-zero words go to counts with one 64-bit atomic each; above that every valid voxel issues
//                its (at most two) 64-bit atomics to counts itself.
// Integer atomics only; no float enters a decision but the per-row ceilf and the per-voxel double quotient: the same inputs
// give the same bytes in every run and in any arrival order. cap > n >= the occupied voxels: an empty slot always exists.
#include "common.h"
#include "voxel_key.h"

namespace mccnn {

constexpr int kVoxThreads = 256;
constexpr int kVoxMaxBlocks = 2048;   // grid-stride beyond: 8 workgroups of 4 waves per CU
// the score pass: few workgroups, so that each one merges many voxels before it flushes -- up to 128 of one trip each, beyond
// that 8 trips (2048 slots) per workgroup, up to 2048 workgroups
constexpr int kVoxScoreBlocks = 128;
constexpr int kVoxScoreTrips = 8;
constexpr size_t kVoxLdsBytes = 32 * 1024;   // the score pass's table of counts in LDS

struct VoxArgs {
    const float* pts;       // [n, 3]
    const int* pred;
    const int* labels;
    const int* bid;         // NULL: every row is cloud 0
    const float* mn;        // [B, 3]
    unsigned long long* keys;   // [cap]
    unsigned* hist;             // [cap, 2, C]
    unsigned long long* counts; // [B, C, 2]
    int* dropped;           // NULL: not counted
    unsigned long long mask;    // cap - 1
    double share;
    float res;
    int n, B, C, ignore, words;   // words = B C 2
};

__global__ __launch_bounds__(kVoxThreads) void vox_vote_k(VoxArgs a) {
    __shared__ unsigned wg_dropped;
    if (threadIdx.x == 0) wg_dropped = 0u;
    __syncthreads();
    const long long n = a.n;
    const long long step = (long long)gridDim.x * kVoxThreads;
    const size_t row_words = 2 * (size_t)a.C;
    for (long long i = (long long)blockIdx.x * kVoxThreads + threadIdx.x; i < n; i += step) {
        const int l = a.labels[i];
        const int b = a.bid ? a.bid[i] : 0;
        if ((unsigned)l >= (unsigned)a.C || (unsigned)b >= (unsigned)a.B) continue;
        const float* p = a.pts + 3 * i;
        const float* m = a.mn + 3 * (size_t)b;
        uint32_t vx, vy, vz;
        const bool inx = voxel_coord(p[0], m[0], a.res, vx), iny = voxel_coord(p[1], m[1], a.res, vy), inz = voxel_coord(p[2], m[2], a.res, vz);
        if (!(inx && iny && inz)) {
            atomicAdd(&wg_dropped, 1u);
            continue;
        }
        const unsigned long long key = voxel_key((uint32_t)b, vx, vy, vz);
        unsigned long long s = voxel_hash(key) & a.mask;
        // at most cap probes: an empty table of cap > n slots ends every chain long before; the bound only keeps a workspace
        // that was NOT the empty table (a caller's wrong ws_clean = 1) from looping for ever -- its rows are then lost
        bool found = false;
        for (unsigned long long tries = 0; tries <= a.mask; ++tries) {
            const unsigned long long prev = atomicCAS(&a.keys[s], 0ull, key);
            if (prev == 0ull || prev == key) {
                found = true;
                break;
            }
            s = (s + 1ull) & a.mask;
        }
        if (!found) continue;
        unsigned* h = a.hist + (size_t)s * row_words;
        atomicAdd(&h[l], 1u);
        const int q = a.pred[i];
        if ((unsigned)q < (unsigned)a.C) atomicAdd(&h[a.C + q], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.dropped && wg_dropped) atomicAdd(a.dropped, (int)wg_dropped);
}

// LDS: where B C 2 words fit kVoxLdsBytes a workgroup counts its valid voxels into a uint32 [B, C, 2] table in LDS and adds the
// non-zero words to counts at its end, one 64-bit global atomic each -- a room's ~20 000 valid voxels fall on the ~40 words of
// one cloud's classes, and that many global atomics on so few addresses queue up behind one another. A workgroup sees fewer
// than 2^31 slots, so a word cannot wrap.
template <bool LDS>
__global__ __launch_bounds__(kVoxThreads) void vox_score_k(VoxArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned vox_tab[];
    const int tid = (int)threadIdx.x;
    if (LDS) {
        for (int k = tid; k < a.words; k += kVoxThreads) vox_tab[k] = 0u;
        __syncthreads();
    }
    const unsigned long long step = (unsigned long long)gridDim.x * kVoxThreads;
    for (unsigned long long s = (unsigned long long)blockIdx.x * kVoxThreads + tid; s <= a.mask; s += step) {
        const unsigned long long key = a.keys[s];
        if (key == 0ull) continue;
        unsigned* h = a.hist + (size_t)s * 2 * (size_t)a.C;
        unsigned best_l = 0u, best_p = 0u, sum = 0u, g = 0u;
        int ul = 0, up = 0;
        for (int c = 0; c < a.C; ++c) {
            const unsigned L = h[c], P = h[a.C + c];
            sum += L;
            if (c == a.ignore) g = L;
            if (L > best_l) { best_l = L; ul = c; }      // (strictly greater: the lowest class of a tie stays)
            if (P > best_p) { best_p = P; up = c; }
            h[c] = 0u;
            h[a.C + c] = 0u;
        }
        a.keys[s] = 0ull;
        const unsigned b = voxel_key_cloud(key);
        if (b >= (unsigned)a.B || !voxel_valid(g, sum, ul, a.ignore, a.share)) continue;
        const size_t at = ((size_t)b * (size_t)a.C + (size_t)ul) * 2;      // (< B C 2 < 2^31)
        if (LDS) {
            atomicAdd(&vox_tab[at + 1], 1u);
            if (ul == up) atomicAdd(&vox_tab[at], 1u);
        } else {
            atomicAdd(&a.counts[at + 1], 1ull);
            if (ul == up) atomicAdd(&a.counts[at], 1ull);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int k = tid; k < a.words; k += kVoxThreads) {
            const unsigned v = vox_tab[k];
            if (v) atomicAdd(&a.counts[k], (unsigned long long)v);
        }
    }
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

size_t mccnn_voxel_acc_workspace_bytes(int n, int num_classes) {
    if (n < 0 || num_classes < 1 || n >= (1 << 30)) return 0;
    return (size_t)(voxel_cap_rec((uint64_t)n) * voxel_slot_bytes((uint64_t)num_classes));
}

int mccnn_voxel_acc_add(const float* pts, const int* pred, const int* labels, const int* batch_ids, const float* aabb_min, int n,
                        int num_clouds, int num_classes, int ignore_label, float resolution, double max_ignore_share,
                        long long* counts, int* dropped, void* ws, size_t ws_bytes, int ws_clean, mccnn_stream_t stream) {
    if (!pts || !pred || !labels || !aabb_min || !counts || !ws) return MCCNN_E_BADARG;
    if (n < 0 || num_clouds < 1 || num_classes < 1) return MCCNN_E_BADARG;
    if (!(resolution > 0.0f) || !std::isfinite(resolution)) return MCCNN_E_BADARG;
    if (((uintptr_t)ws & 15u) != 0) return MCCNN_E_BADARG;                // (cleared 16 bytes at a time, 8-byte atomics)
    if (num_clouds > MCCNN_VOXEL_MAX_CLOUDS || n >= (1 << 30)) return MCCNN_E_TOOLARGE;
    if ((long long)num_clouds * (long long)num_classes > ((1ll << 31) - 1) / 2) return MCCNN_E_TOOLARGE;   // B C 2 < 2^31
    if (n == 0) return 0;
    const uint64_t slot = voxel_slot_bytes((uint64_t)num_classes), cap_min = voxel_cap_min((uint64_t)n);
    uint64_t cap = voxel_cap_rec((uint64_t)n);
    while (cap > cap_min && cap * slot > (uint64_t)ws_bytes) cap >>= 1;   // the largest power of two that fits, up to cap_rec
    if (cap * slot > (uint64_t)ws_bytes) return MCCNN_E_WORKSPACE;
    VoxArgs a = {};
    a.pts = pts; a.pred = pred; a.labels = labels; a.bid = batch_ids; a.mn = aabb_min;
    a.keys = reinterpret_cast<unsigned long long*>(ws);
    a.hist = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws) + cap * 8);
    a.counts = reinterpret_cast<unsigned long long*>(counts);   // (two's complement: an unsigned add is the signed add)
    a.dropped = dropped;
    a.mask = cap - 1;
    a.share = max_ignore_share;
    a.res = resolution;
    a.n = n; a.B = num_clouds; a.C = num_classes;
    a.ignore = ignore_label < 0 ? -1 : ignore_label;
    a.words = num_clouds * num_classes * 2;
    hipStream_t st = (hipStream_t)stream;
    if (!ws_clean) {   // (cap >= 2 slots of a multiple of 8 bytes: whole 16-byte units)
        const int rc = launch_clear_spans(clear_span(ws, (size_t)(cap * slot)), no_span(), no_span(), st);
        if (rc) return rc;
    }
    const int trips = ceil_div(n, kVoxThreads);
    vox_vote_k<<<(unsigned)(trips < kVoxMaxBlocks ? trips : kVoxMaxBlocks), kVoxThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    const uint64_t sweeps = (cap + kVoxThreads - 1) / kVoxThreads;
    uint64_t sb = sweeps / kVoxScoreTrips;
    if (sb > (uint64_t)kVoxMaxBlocks) sb = kVoxMaxBlocks;
    if (sb < (uint64_t)kVoxScoreBlocks) sb = sweeps < (uint64_t)kVoxScoreBlocks ? sweeps : (uint64_t)kVoxScoreBlocks;
    const unsigned sblocks = (unsigned)sb;
    const size_t lds = (size_t)a.words * sizeof(unsigned);
    if (lds <= kVoxLdsBytes) vox_score_k<true><<<sblocks, kVoxThreads, lds, st>>>(a);
    else vox_score_k<false><<<sblocks, kVoxThreads, 0, st>>>(a);
    MCCNN_LAUNCHED();
    return 0;
}

}  // extern "C"
