// The edge budget of a neighbour search (mccnn_find_neighbors_count_budget): between the count pass, which leaves the
// uncapped row lengths kfull[0..m), and the fill pass, which reads the cap from a device word,
//     selection   kfull -> K* = the largest cap whose list has at most B rows (neigh_budget.h has the rule and its scalar
//                 half), in one launch for lists of up to MCCNN_NB_SMALL_M centres and in MCCNN_NB_LEVELS otherwise;
//     prefix sum  of min(kfull[i], K*) -- the clamp rides in the scan's load, there is no pass over m for it alone.
// Nothing returns to the host. Histograms are merged with integer atomics only: the order of arrival changes no bit.
#include "batch.h"
#include "chain.h"
#include "neigh_budget.h"

namespace mccnn {

#define MCCNN_NB_SMALL_M 4096  // lists of up to this many centres: all levels of the selection in ONE workgroup
#define MCCNN_NB_MAX_BLOCKS 256
constexpr int NB_HIST = 2048 + 1024 + 1024;   // buckets of all levels, one after the other
__host__ __device__ constexpr int nb_level_offset(int level) { return level == 0 ? 0 : (level == 1 ? 2048 : 3072); }
// the words behind the histograms (uint32): a ticket per level, the longest row, "K* is written", the range of the next level
enum { NB_TICKET = 0, NB_KMAX = 3, NB_DONE = 4, NB_RANGE = 6, NB_MISC_WORDS = 16 };

// what the selection and the scan need zero on entry -- status words of the scan (tiles + 1), histograms, misc words --
// is ONE run of 8-byte words: the count pass clears it on its way (NeighItem::zeroWords), no launch of its own
struct BudgetWs {
    unsigned long long* status;
    uint32_t* rows;
    unsigned long long* sums;
    uint32_t* misc;
};
static size_t budget_zero_words(int m) {
    const size_t tiles = (size_t)ceil_div(m > 0 ? m : 1, SCAN_TILE);
    return (tiles + 1) + NB_HIST / 2 + NB_HIST + NB_MISC_WORDS / 2;
}
static BudgetWs budget_ws(void* region, int m) {
    const size_t tiles = (size_t)ceil_div(m > 0 ? m : 1, SCAN_TILE);
    BudgetWs w;
    w.status = reinterpret_cast<unsigned long long*>(region);
    w.sums = w.status + tiles + 1;
    w.rows = reinterpret_cast<uint32_t*>(w.sums + NB_HIST);
    w.misc = w.rows + NB_HIST;
    return w;
}
size_t budget_region_bytes(int m) { return align_up(budget_zero_words(m) * sizeof(unsigned long long)); }
void budget_region_zero(void* region, int m, unsigned long long** words, int* count) {
    *words = reinterpret_cast<unsigned long long*>(region);
    *count = (int)budget_zero_words(m);
}

// One level's histogram of the rows [first, m) in steps of `stride`, into LDS (zero on entry): rows whose k lies in
// [lo, lo + (nb << shift)) add (1, k) to their bucket. Returns the longest row this thread has seen.
__device__ __forceinline__ uint32_t budget_hist(const int* __restrict__ kfull, int m, int first, int stride, uint32_t lo, int shift, int nb,
                                                uint32_t* hr, unsigned long long* hs) {
    // four rows per trip, all four loads in flight before the first LDS atomic: one memory latency per trip, not four (a
    // level is latency bound: it reads 4 m bytes once). NONE marks a slot past the end (no row has 2^32 - 1 hits).
    constexpr uint32_t NONE = 0xffffffffu;
    uint32_t kmax = 0;
    for (long long i0 = first; i0 < m; i0 += 4LL * stride) {
        uint32_t kv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = i0 + (long long)u * stride;
            kv[u] = i < m ? (uint32_t)max(kfull[i], 0) : NONE;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t k = kv[u];
            if (k == NONE) continue;
            kmax = max(kmax, k);
            if (k >= lo) {
                const uint32_t d = (k - lo) >> shift;
                if (d < (uint32_t)nb) {
                    atomicAdd(&hr[d], 1u);
                    atomicAdd(&hs[d], (unsigned long long)k);
                }
            }
        }
    }
    return kmax;
}

// The scalar step of a level (one thread; the histogram of the level complete in hr / hs): -> true when K* is decided
__device__ __forceinline__ bool budget_step(int level, const uint32_t* hr, const unsigned long long* hs, BudgetRange& r,
                                            unsigned long long budget, int Ku, int kmax, int* cap) {
    const int nb = budget_level_buckets(level), shift = budget_level_shift(level);
    const int b = budget_pick(hr, reinterpret_cast<const uint64_t*>(hs), nb, shift, r, budget);
    if (b < 0) {
        // level 0: S never exceeds the budget, the list fits. (Deeper levels always hit -- the end of the range IS the end of
        // the bucket that was hit above; were they not to, the crossing would lie at the end of the range.)
        *cap = level == 0 ? budget_cap(0, 0u, Ku, kmax) : budget_cap(1, r.lo + ((uint32_t)nb << shift) - 1u, Ku, kmax);
        return true;
    }
    if (level == MCCNN_NB_LEVELS - 1) {
        *cap = budget_cap(1, r.lo, Ku, kmax);
        return true;
    }
    return false;
}

// All levels in one workgroup (no global atomics, no tickets)
__device__ __forceinline__ void budget_select_small_body(const int* __restrict__ kfull, int m, unsigned long long budget, int Ku,
                                                         int* __restrict__ capDev) {
    __shared__ uint32_t hr[MCCNN_NB_BUCKETS];
    __shared__ unsigned long long hs[MCCNN_NB_BUCKETS];
    __shared__ BudgetRange sR;
    __shared__ uint32_t sMax;
    __shared__ int sDone;
    if (threadIdx.x == 0) {
        sR = BudgetRange{0ull, (uint32_t)m, 0u};
        sMax = 0u;
        sDone = 0;
    }
    for (int level = 0; level < MCCNN_NB_LEVELS; ++level) {
        const int nb = budget_level_buckets(level), shift = budget_level_shift(level);
        for (int b = threadIdx.x; b < nb; b += 256) { hr[b] = 0u; hs[b] = 0ull; }
        __syncthreads();
        const uint32_t kmax = budget_hist(kfull, m, (int)threadIdx.x, 256, sR.lo, shift, nb, hr, hs);
        if (level == 0) atomicMax(&sMax, kmax);
        __syncthreads();
        if (threadIdx.x == 0) {
            BudgetRange r = sR;
            int cap = 1;
            if (budget_step(level, hr, hs, r, budget, Ku, (int)sMax, &cap)) {
                *capDev = cap;
                sDone = 1;
            }
            sR = r;
        }
        __syncthreads();
        if (sDone) return;
    }
}
__global__ __launch_bounds__(256) void budget_select_small(const int* __restrict__ kfull, int m, unsigned long long budget, int Ku,
                                                           int* __restrict__ capDev) {
    budget_select_small_body(kfull, m, budget, Ku, capDev);
}
// The same for the small lists of a BATCH of searches (mccnn_geometry_build_batch_budget): one workgroup per list, the lists'
// arguments by value in the kernel arguments
struct BudgetSmallItem { const int* kfull; int* capDev; unsigned long long B; int m, Ku; };
struct BudgetSmallBatch { BudgetSmallItem it[MCCNN_BATCH_MAX]; };
__global__ __launch_bounds__(256) void budget_select_small_batch(BudgetSmallBatch sb) {
    const BudgetSmallItem& g = sb.it[blockIdx.x];
    budget_select_small_body(g.kfull, g.m, g.B, g.Ku, g.capDev);
}

// One level over the whole chip: per-workgroup histograms in LDS, merged into the level's global histogram with integer
// atomics; the workgroup that draws the last ticket reads the merged histogram back and takes the scalar step.
// (workgroup `blk` of the `nblk` that share the list: the single launch, and one list's share of a batch launch -- "last"
// is the last of THIS list, its ticket and histograms are the list's own)
template <int LEVEL>
__device__ __forceinline__ void budget_select_level_body(const int* __restrict__ kfull, int m, const BudgetWs& w, unsigned long long budget,
                                                         int Ku, int* __restrict__ capDev, const unsigned blk, const unsigned nblk) {
    __shared__ uint32_t hr[MCCNN_NB_BUCKETS];
    __shared__ unsigned long long hs[MCCNN_NB_BUCKETS];
    __shared__ uint32_t sMax;
    __shared__ int sLast;
    constexpr int nb = LEVEL == 0 ? 2048 : 1024, shift = LEVEL == 0 ? 20 : (LEVEL == 1 ? 10 : 0), off = nb_level_offset(LEVEL);
    BudgetRange r{0ull, (uint32_t)m, 0u};
    if (LEVEL > 0) {
        if (w.misc[NB_DONE]) return;   // (the same word for every workgroup: written by the level before)
        r = *reinterpret_cast<const BudgetRange*>(w.misc + NB_RANGE);
    }
    for (int b = threadIdx.x; b < nb; b += 256) { hr[b] = 0u; hs[b] = 0ull; }
    if (threadIdx.x == 0) sMax = 0u;
    __syncthreads();
    const uint32_t kmax = budget_hist(kfull, m, (int)(blk * 256 + threadIdx.x), (int)(nblk * 256), r.lo, shift, nb, hr, hs);
    if (LEVEL == 0) atomicMax(&sMax, kmax);
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += 256) {
        const uint32_t c = hr[b];
        if (c) {
            __hip_atomic_fetch_add(w.rows + off + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(w.sums + off + b, hs[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (LEVEL == 0 && threadIdx.x == 0) __hip_atomic_fetch_max(w.misc + NB_KMAX, sMax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0)
        sLast = __hip_atomic_fetch_add(w.misc + NB_TICKET + LEVEL, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1u;
    __syncthreads();
    if (!sLast) return;
    __threadfence();
    {   // (all loads of a thread in flight at once: one round trip to L2, not nb / 256)
        constexpr int PER = nb / 256;
        uint32_t c[PER];
        unsigned long long s[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            c[u] = __hip_atomic_load(w.rows + off + u * 256 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s[u] = __hip_atomic_load(w.sums + off + u * 256 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            hr[u * 256 + threadIdx.x] = c[u];
            hs[u * 256 + threadIdx.x] = s[u];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int longest = (int)__hip_atomic_load(w.misc + NB_KMAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int cap = 1;
        if (budget_step(LEVEL, hr, hs, r, budget, Ku, longest, &cap)) {
            *capDev = cap;
            w.misc[NB_DONE] = 1u;
        } else {
            *reinterpret_cast<BudgetRange*>(w.misc + NB_RANGE) = r;
        }
    }
}
template <int LEVEL>
__global__ __launch_bounds__(256) void budget_select_level(const int* __restrict__ kfull, int m, BudgetWs w, unsigned long long budget,
                                                           int Ku, int* __restrict__ capDev) {
    budget_select_level_body<LEVEL>(kfull, m, w, budget, Ku, capDev, blockIdx.x, gridDim.x);
}
// One level of the larger lists of a batch: their workgroups share one grid (BatchBlocks), every list keeps its own region
struct BudgetLevelItem { const int* kfull; int* capDev; BudgetWs w; unsigned long long B; int m, Ku; };
struct BudgetLevelBatch { BudgetLevelItem it[MCCNN_BATCH_MAX]; };
static_assert(sizeof(BudgetLevelBatch) + sizeof(BatchBlocks) < 4096, "the kernel arguments of a batched selection level: < 4 KB");
template <int LEVEL>
__global__ __launch_bounds__(256) void budget_select_level_batch(BudgetLevelBatch lb, BatchBlocks bb) {
    int local, blocks;
    const BudgetLevelItem& g = lb.it[batch_item(bb, (int)blockIdx.x, local, blocks)];
    budget_select_level_body<LEVEL>(g.kfull, g.m, g.w, g.B, g.Ku, g.capDev, (unsigned)local, (unsigned)blocks);
}

// scan_chained (scan.hip) over min(in[i], *capDev): the prefix sum of the capped row lengths; one tile or many (a single
// tile is tile 0 of a chain of one). status: tiles + 1 words, zero on entry.
// (tile taken from the ticket behind the `nblk` status words of THIS array: the look-back never waits for a tile that is not
// scheduled, in a launch of its own and as one array's share of a batch launch alike)
__device__ __forceinline__ void scan_clamp_body(const int* __restrict__ in, const int* __restrict__ capDev, int* __restrict__ out, int n,
                                                unsigned long long* status, int* __restrict__ total, int* __restrict__ total2,
                                                const int nblk) {
    __shared__ int lds[4];
    __shared__ int sOff;
    __shared__ int sTile;
    if (threadIdx.x == 0)
        sTile = (int)__hip_atomic_fetch_add(status + nblk, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int cap = __builtin_amdgcn_readfirstlane(*capDev);
    __syncthreads();
    const int tile = sTile;
    const long long base = (long long)tile * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    int s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = (base + k < n) ? min(in[base + k], cap) : 0;
        s += v[k];
    }
    int tot;
    const int ex = block_excl_scan(s, tot, lds);
    if (threadIdx.x < 64) {
        const int excl = chain_lookback(status, tile, tot, (int)threadIdx.x);
        if (threadIdx.x == 0) sOff = excl;
    }
    __syncthreads();
    int run = ex + sOff;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (tile == nblk - 1 && threadIdx.x == SCAN_THREADS - 1) {
        *total = run;
        if (total2) *total2 = run;   // (a geometry's pinned host word)
    }
}
__global__ __launch_bounds__(SCAN_THREADS) void scan_chained_clamp(const int* __restrict__ in, const int* __restrict__ capDev,
                                                                   int* __restrict__ out, int n, unsigned long long* status,
                                                                   int* __restrict__ total, int* __restrict__ total2) {
    scan_clamp_body(in, capDev, out, n, status, total, total2, (int)gridDim.x);
}
// ... of the budgeted lists of a batch: a launch of their own beside scan_chained_batch, which keeps its arguments and its
// code. clamp[k]: the cap word of item k.
struct ClampBatch { const int* cap[MCCNN_BATCH_MAX]; };
__global__ __launch_bounds__(SCAN_THREADS) void scan_chained_clamp_batch(ScanBatch sb, ClampBatch cb, BatchBlocks bb) {
    int local, blocks;
    const int k = batch_item(bb, (int)blockIdx.x, local, blocks);
    const ScanItem& it = sb.it[k];
    scan_clamp_body(it.in, cb.cap[k], it.out, it.n, it.status, it.total, it.total2, blocks);
}

// m == 0: an empty list and the floor of the cap
__global__ void budget_empty(int* __restrict__ total, int* __restrict__ capDev) {
    if (threadIdx.x == 0) {
        *total = 0;
        *capDev = 1;
    }
}
int launch_budget_empty(int* total_dev, int* cap_dev, hipStream_t s) {
    budget_empty<<<1, 64, 0, s>>>(total_dev, cap_dev);
    MCCNN_LAUNCHED();
    return 0;
}

// the selection over the row lengths the count pass left (which also cleared `region`): 1 or 3 launches
int budget_select(const int* kfull, int m, void* region, int max_edges, int max_neighbors, int* cap_dev, hipStream_t s) {
    const int tiles = ceil_div(m, SCAN_TILE);
    if (m <= 0 || tiles > 1024) return MCCNN_E_TOOLARGE;   // (the chained scan: up to 2 M centres)
    const BudgetWs w = budget_ws(region, m);
    const unsigned long long B = (unsigned long long)max_edges;
    if (m <= MCCNN_NB_SMALL_M && small_kernels_on()) {   // (mccnn_debug_small_kernels(0): the chip-wide levels at every size)
        budget_select_small<<<1, 256, 0, s>>>(kfull, m, B, max_neighbors, cap_dev);
        MCCNN_LAUNCHED();
    } else {
        const int blocks = min(ceil_div(m, 4 * 256), MCCNN_NB_MAX_BLOCKS);   // four rows per thread up to 262 144 centres
        budget_select_level<0><<<blocks, 256, 0, s>>>(kfull, m, w, B, max_neighbors, cap_dev);
        MCCNN_LAUNCHED();
        budget_select_level<1><<<blocks, 256, 0, s>>>(kfull, m, w, B, max_neighbors, cap_dev);
        MCCNN_LAUNCHED();
        budget_select_level<2><<<blocks, 256, 0, s>>>(kfull, m, w, B, max_neighbors, cap_dev);
        MCCNN_LAUNCHED();
    }
    return 0;
}
// the prefix sum of min(kfull, *cap_dev) behind it: one launch
int budget_scan(const int* kfull, int m, void* region, const int* cap_dev, int* start_idx, int* total_dev, int* total_host, hipStream_t s) {
    const int tiles = ceil_div(m, SCAN_TILE);
    if (m <= 0 || tiles > 1024) return MCCNN_E_TOOLARGE;
    scan_chained_clamp<<<tiles, SCAN_THREADS, 0, s>>>(kfull, cap_dev, start_idx, m, budget_ws(region, m).status, total_dev, total_host);
    MCCNN_LAUNCHED();
    return 0;
}
// selection + prefix sum (mccnn_find_neighbors_count_budget): 2 or 4 launches
int budget_select_scan(const int* kfull, int m, void* region, int max_edges, int max_neighbors, int* cap_dev, int* start_idx,
                       int* total_dev, hipStream_t s) {
    int rc = budget_select(kfull, m, region, max_edges, max_neighbors, cap_dev, s);
    if (rc) return rc;
    return budget_scan(kfull, m, region, cap_dev, start_idx, total_dev, nullptr, s);
}

// ---- batch form (exec.hip: a chunk of mccnn_geometry_build_batch_budget). The count pass of the chunk has left every item's
// row lengths and cleared its region. Selection: ONE launch over the small items (one workgroup each) and three over the
// larger ones (the levels; their workgroups share a grid) -- each only when items of its size class are present.
int launch_budget_select_batch(const BudgetItem* items, int count, hipStream_t s) {
    if (count < 0 || count > MCCNN_BATCH_MAX) return MCCNN_E_BADARG;
    BudgetSmallBatch sb;
    BudgetLevelBatch lb;
    BatchBlocks bb;
    int nS = 0, nL = 0, run = 0;
    for (int k = 0; k < count; ++k) {
        const BudgetItem& b = items[k];
        if (b.m <= 0 || ceil_div(b.m, SCAN_TILE) > 1024) return MCCNN_E_TOOLARGE;
        if (b.m <= MCCNN_NB_SMALL_M && small_kernels_on()) {
            sb.it[nS++] = BudgetSmallItem{b.kfull, b.cap_dev, (unsigned long long)b.max_edges, b.m, b.max_neighbors};
        } else {
            lb.it[nL] = BudgetLevelItem{b.kfull, b.cap_dev, budget_ws(b.region, b.m), (unsigned long long)b.max_edges, b.m, b.max_neighbors};
            bb.first[nL++] = run;
            run += min(ceil_div(b.m, 4 * 256), MCCNN_NB_MAX_BLOCKS);
        }
    }
    if (nS) {
        for (int k = nS; k < MCCNN_BATCH_MAX; ++k) sb.it[k] = sb.it[0];   // (never addressed: defined bytes)
        budget_select_small_batch<<<nS, 256, 0, s>>>(sb);
        MCCNN_LAUNCHED();
    }
    if (nL) {
        for (int k = nL; k < MCCNN_BATCH_MAX; ++k) lb.it[k] = lb.it[0];
        for (int k = nL; k <= MCCNN_BATCH_MAX; ++k) bb.first[k] = run;
        bb.count = nL;
        budget_select_level_batch<0><<<run, 256, 0, s>>>(lb, bb);
        MCCNN_LAUNCHED();
        budget_select_level_batch<1><<<run, 256, 0, s>>>(lb, bb);
        MCCNN_LAUNCHED();
        budget_select_level_batch<2><<<run, 256, 0, s>>>(lb, bb);
        MCCNN_LAUNCHED();
    }
    return 0;
}
// ... and the prefix sums of min(kfull, K*) of all of them: one launch
int launch_budget_scan_batch(const BudgetItem* items, int count, hipStream_t s) {
    if (count < 0 || count > MCCNN_BATCH_MAX) return MCCNN_E_BADARG;
    if (count == 0) return 0;
    ScanBatch sc;
    ClampBatch cb;
    for (int k = 0; k < count; ++k) {
        const BudgetItem& b = items[k];
        const int tiles = ceil_div(b.m, SCAN_TILE);
        if (b.m <= 0 || tiles > 1024) return MCCNN_E_TOOLARGE;
        sc.it[k] = ScanItem{b.kfull, b.start_idx, budget_ws(b.region, b.m).status, b.total_dev, b.total_host, b.m, tiles};
        cb.cap[k] = b.cap_dev;
    }
    for (int k = count; k < MCCNN_BATCH_MAX; ++k) { sc.it[k] = sc.it[0]; cb.cap[k] = cb.cap[0]; }
    BatchBlocks bb;
    const int run = batch_blocks(bb, count, [&](int k) { return sc.it[k].tiles; });
    scan_chained_clamp_batch<<<run, SCAN_THREADS, 0, s>>>(sc, cb, bb);
    MCCNN_LAUNCHED();
    return 0;
}

}  // namespace mccnn
