// Batch form of a step's geometries (exec.hip: mccnn_geometry_build_batch): ONE launch per kernel kind over up to
// MCCNN_BATCH_MAX geometries. The per-geometry arguments of every kind travel by value in the kernel arguments (BatchBlocks,
// ScanBatch, SpanBatch: common.h); kernels and item builders live next to their single forms (grid.hip, neighbors.hip, scan.hip).
#pragma once
#include "common.h"
#include <cmath>
#include <cstring>

namespace mccnn {

// sqrt_threshold (common.h) on the host: the same float operations, both square roots correctly rounded. An absolute radius
// has ONE threshold, computed once per call (the search, the per-point density and its gradients: NeighItem / PointPdfItem::Tabs).
inline float sqrt_threshold_host(float R) {
    auto prev = [](float v) { uint32_t u; memcpy(&u, &v, 4); --u; memcpy(&v, &u, 4); return v; };
    auto next = [](float v) { uint32_t u; memcpy(&u, &v, 4); ++u; memcpy(&v, &u, 4); return v; };
    float t = R * R;
    for (int it = 0; it < 8 && t > 0.0f && sqrtf(prev(t)) >= R; ++it) t = prev(t);
    for (int it = 0; it < 8 && sqrtf(t) < R; ++it) t = next(t);
    return t;
}

// Members per wave of a window kernel (cell_window.h) that runs beside others -- background searches, every batch item, the
// per-point density and, up to 4, its gradients: 8 consecutive members of a cell-coherent order share most of their windows on
// a large list (~8 points per cell), but a list with few members needs the waves -- 6 344 pooling centres with ~900
// candidates each ran 139 us per pass on 793 waves (BASELINE cfg2 Pool_1), the coarse levels of a hierarchy 20 us on a handful.
#ifndef MCCNN_NW_G
#define MCCNN_NW_G 8
#endif
inline int window_group(long long m) { return m >= 32768 ? MCCNN_NW_G : (m >= 16384 ? 4 : (m >= 8192 ? 2 : 1)); }

// one counting sort: the grid build of a geometry, or the visiting order of its foreign centres (newIdx == nullptr)
struct GridItem {
    const float* pts; const int* bids; const float* mn; const float* mx;
    int* keys; int* cnt; int* arrival; int* start; int* slot;
    int* newIdx; float* oPts; int* oBids; int* inv; int2* cells;
    int n, B, nc, C, ldsHist;
};
struct GridBatch { GridItem it[MCCNN_BATCH_MAX]; };

// one neighbour search (count pass / fill pass)
struct NeighItem {
    const float* centres; const int* cb; const float* pts; const int* cells; const float* mn; const float* mx; const int* order;
    int* cnt; unsigned long long* masks; int* startIdx; int* packed; unsigned long long* zeroWords;
    int m, B, nc, scaleInv, capacity, G, numZero;
    float radius, Tabs;
};
struct NeighBatch { NeighItem it[MCCNN_BATCH_MAX]; };
// the cap of a search: beside NeighItem (in a batch: NeighCapBatch, item k of one belongs to item k of the other).
// capK == 0: no cap; sampled: the fill pass draws the stratified sample of `seed` (neigh_sample.h). capDev (an edge budget;
// nullptr: none): the device word the selection leaves the cap in -- the count pass of such a search runs unclamped (capK =
// 0x7fffffff), its fill pass reads capK from the word
struct NeighCapItem { int* kfull; const int* capDev; int capK; unsigned seed; int sampled; };
struct NeighCapBatch { NeighCapItem it[MCCNN_BATCH_MAX]; };
// the prefix sum of the counts inside the fill pass of a small list (single launches; all null in a batch)
struct NeighScan { const int* scanCnt; int* startOut; int* totalDev; int* totalHost; };
// the kind of a search's kernels: which of the three records above an instantiation reads
// (the two budget kinds are fill passes of a batch only: the capped / sampled body with the cap read from NeighCapItem::capDev)
enum { NEIGH_PLAIN = 0, NEIGH_CAPPED = 1, NEIGH_SAMPLED = 2, NEIGH_BUDGET = 3, NEIGH_BUDGET_SAMPLED = 4 };
static_assert(sizeof(NeighBatch) + sizeof(NeighCapBatch) + sizeof(BatchBlocks) < 4096, "the kernel arguments of a batched search: < 4 KB");

// one kernel-density estimate
struct PdfItem {
    const float* pts; const int* bids; const int2* packed; const int* startIdx; const float* mn; const float* mx; float* pdfs;
    const int* eDev;
    int m, e, B, scaleInv, rowsPerWave;
    float window, radius;
    // the per-edge records of the convolution kernels, written beside the PDFs (rec == nullptr: PDFs alone): the centres the
    // rows belong to, the records in edge order, and whether their weight carries the row length (the layers' `avg`)
    const float* centres; float4* rec; int avg;
};
struct PdfBatch { PdfItem it[MCCNN_BATCH_MAX]; };
static_assert(sizeof(PdfBatch) + sizeof(BatchBlocks) < 4096, "the kernel arguments of a batched KDE: < 4 KB");
// one per-point density sweep (pdf_points.hip): the sorted points of a grid, its cell table and boxes -> density, counts
struct PointPdfItem {
    const float* pts; const int* bids; const int* cells; const float* mn; const float* mx; float* density; int* counts;
    int n, B, nc, scaleInv;
    float window, radius, Tabs;
};
struct PointPdfBatch { PointPdfItem it[MCCNN_BATCH_MAX]; };
// one expansion of a density over a list whose edge total lives in a device word: pdfs[e] = density[j] / len_i, e < min(*totalDev, eCap)
struct ExpandItem {
    const float* density; const int* startIdx; const int2* packed; const int* totalDev; float* pdfs;
    int n, m, eCap;
};
struct ExpandBatch { ExpandItem it[MCCNN_BATCH_MAX]; };
static_assert(sizeof(PointPdfBatch) + sizeof(BatchBlocks) < 4096, "the kernel arguments of a batched density sweep: < 4 KB");
static_assert(sizeof(ExpandBatch) + sizeof(BatchBlocks) < 4096, "the kernel arguments of a batched expansion: < 4 KB");

// ---- small row plans of a step (mccnn_geometry_prebuild_batch): transposition, layout and fill of every small list as one
// launch each. (12 items per launch: the fill's item carries the geometry an inline record is evaluated from.)
#define MCCNN_PLAN_BATCH_MAX 12
struct TrSmallItem { const int2* packed; int* cnt; int* slot; int* tmp; int* startT; int* permT; int e, n; };
struct TrSmallBatch { TrSmallItem it[MCCNN_BATCH_MAX]; };
struct PlanSmallItem { const int* rowStart; const int* order; int* vrow; int* vcode; int* sliceOff; int* vposRow; int rows, e, L, S; };
struct PlanSmallBatch { PlanSmallItem it[MCCNN_BATCH_MAX]; };
struct SellFillItem {
    // the list and its geometry (records are evaluated inline: conv_mfma.h edge_record)
    const float* pts; const int* bids; const float* pdfs; const float* samples; const int* start; const int2* packed;
    const float* mn; const float* mx;
    const int* rowStart; const int* permT;
    // the plan
    const int* vrow; const int* vcode; const int* sliceOff; const int* vposRow; float4* rec; int* oth;
    long long cap;
    int n, m, e, B, scaleInv, avg, rows, S, L, chunks;
    float radius;
};
struct SellFillBatch { SellFillItem it[MCCNN_PLAN_BATCH_MAX]; };
// the transposition of a list too long for one workgroup: count -> prefix sum (scan.hip's batch form) -> fill -> rank
struct TrChainItem { const int2* packed; int* cnt; int* slot; int* tmp; int* startT; int* permT; int e, n, lds, norank /* ranked by the plan's scatter */; };
struct TrChainBatch { TrChainItem it[MCCNN_BATCH_MAX]; };
int tr_chain_item(TrChainItem& t, ScanItem& sc, ClearSpan& head, const int* packed, int e, int n, int* start_t, int* perm_t, void* ws,
                  size_t ws_bytes);                                                                 // conv.hip (ws: mccnn_transpose_neighbors_workspace_bytes)
int launch_tr_chain_batch(const TrChainBatch& tb, int count, int phase, hipStream_t s);            // 0 count, 1 fill, 2 rank
// a LARGE row plan (every plan plan_small does not lay out): layout (vr_count -> vr_scan_expand -> sell_sort), then the
// forward plan's tile fill or the transposed plan's bases + scatter (conv_rows.hip build_large has the single-plan chain)
#define MCCNN_LARGE_BATCH_MAX 8
struct LargeItem {
    const int* rowStart; const int* order;
    int* vcnt; unsigned long long* st1; unsigned long long* st2; int* vlistRow; int* vTotal;
    int* vrow; int* vcode; int* sliceOff; int* vposRow; int* oth; float4* rec;
    long long cap;
    const float* pts; const int* bids; const float* pdfs; const float* samples; const int* start; const int2* packed;
    const float* mn; const float* mx;
    float4* recE;                                    // per-edge records in edge order (evaluated here when `eval`)
    int2* vinfo; const int* startT; const int* tmp; int* permT;   // transposed plans
    int rows, e, n, m, B, L, S, windows, tiles, scaleInv, avg;
    int tr, eval /* 0 records ready, 1 evaluate (fwd: in the fill; tr: a pass of its own) */, rank /* tr: the list is ranked in the scatter */;
    float radius;
};
struct LargeBatch { LargeItem it[MCCNN_LARGE_BATCH_MAX]; };
bool plan_large_batchable(int rows, int e, int n, int transposed, int tlist_ready);                 // conv_rows.hip
size_t plan_large_ws_bytes(int rows, int e, int n, int transposed, int tlist_ready);
// -> item + (transposed, list not ready) the chain item of its transposition (*use_chain) + the spans its head has to clear
int plan_large_item(int transposed, const float* sorted_pts, const int* sorted_batch_ids, const float* pdfs, const float* samples,
                    const int* start_idx, const int* packed, const float* aabb_min, const float* aabb_max, int n, int m, int e,
                    int batch_size, float radius, int scale_inv, int avg, const int* order, void* rec_edges, int rec_ready, int* start_t,
                    int* perm_t, int tlist_ready, void* plan_buffer, void* ws, size_t ws_bytes, LargeItem& it, TrChainItem* tc,
                    ScanItem* sc, bool* use_chain, SpanBatch& spans);
enum { LARGE_VR_COUNT = 0, LARGE_VR_SCAN, LARGE_SELL_SORT, LARGE_BASES, LARGE_RECORDS, LARGE_FILL, LARGE_SCATTER };
int launch_plan_large_batch(const LargeBatch& lb, int count, int phase, hipStream_t s);

int launch_tr_small_batch(const TrSmallBatch& tb, int count, hipStream_t s);                       // conv.hip
int launch_plan_small_batch(const PlanSmallBatch& pb, int count, hipStream_t s);                   // conv_rows.hip
int launch_sell_fill_batch(const SellFillBatch& fb, int count, int transposed, hipStream_t s);     // conv_rows.hip

bool grid_batch_eligible(int n, int batch_size, int num_cells);
int grid_batch_item(GridItem& g, ScanItem& sc, ClearSpan& head, const float* pts, const int* batch_ids, const float* aabb_min,
                    const float* aabb_max, int n, int batch_size, int num_cells, int* new_idx, float* out_pts,
                    int* out_batch_ids, int* cell_indexs, int* inv_idx, void* ws, size_t ws_bytes);
int order_batch_item(GridItem& g, ScanItem& sc, ClearSpan& head, const float* pts, const int* batch_ids, const float* aabb_min,
                     const float* aabb_max, int m, int batch_size, int num_cells, int* order, void* ws, size_t ws_bytes);
int launch_grid_batch_phase(const GridBatch& gb, int count, int phase, hipStream_t s);   // 0 keys + histogram, 1 park, 2 rank + move + cells
// One search as the host describes it: what the mccnn_find_neighbors_* entries take as parameters and exec.hip reads from
// a geometry. Every host function of the search takes this; neigh_item (neighbors.hip) turns it into the kernels' records.
struct NeighSearch {
    const float* centres; const int* cbids; int m;      // the centres and their batch ids
    const float* pts; int n; const int* cells;           // the sorted points and the cell table
    const float* mn; const float* mx; int B, nc;          // the boxes
    float radius; int scale_inv;
    const int* order;                                     // visiting order of the centres (nullptr: by index)
    int* start_idx; int capacity; int* packed;
    int* total_dev; int* total_host;                      // the edge total: device word, pinned host word (or nullptr)
    void* ws; size_t ws_bytes;
    int max_neighbors, sampled; unsigned seed;            // the cap: 0 = none; sampled: the draw of `seed`
    int max_edges; int* cap_dev;                          // the edge budget: 0 = none; the device word its cap K* goes to
};
int find_neighbors_chain(const NeighSearch& q, hipStream_t s);   // count (scan) fill, back to back
// neigh_budget.hip: the edge budget of a search (mccnn_find_neighbors_count_budget). `region`: budget_region_bytes(m) behind
// the capped workspace, one run of 8-byte words the count pass clears (budget_region_zero names them)
size_t budget_region_bytes(int m);
void budget_region_zero(void* region, int m, unsigned long long** words, int* count);
int budget_select_scan(const int* kfull, int m, void* region, int max_edges, int max_neighbors, int* cap_dev, int* start_idx,
                       int* total_dev, hipStream_t s);
int budget_select(const int* kfull, int m, void* region, int max_edges, int max_neighbors, int* cap_dev, hipStream_t s);
int budget_scan(const int* kfull, int m, void* region, const int* cap_dev, int* start_idx, int* total_dev, int* total_host, hipStream_t s);
// one budgeted search of a batch, between its count and its fill pass: the row lengths, the region the count pass cleared, the
// budget and the caller's cap, and where the cap, the prefix sum and the edge total go
struct BudgetItem {
    const int* kfull; void* region; int m, max_edges, max_neighbors;
    int* cap_dev; int* start_idx; int* total_dev; int* total_host;
};
int launch_budget_select_batch(const BudgetItem* items, int count, hipStream_t s);   // <= 1 + 3 launches
int launch_budget_scan_batch(const BudgetItem* items, int count, hipStream_t s);     // 1 launch
int launch_budget_empty(int* total_dev, int* cap_dev, hipStream_t s);
bool neigh_batch_eligible(int m, int n);
// (a budgeted search: `sc` is left alone -- its prefix sum is the clamped one -- and `bud` describes what runs between its passes)
int neigh_batch_item(NeighItem& it, NeighCapItem& cap, ScanItem& sc, const NeighSearch& q, BudgetItem* bud = nullptr);
int launch_neigh_batch(const NeighBatch& nbt, const NeighCapBatch& caps, int count, int mode, hipStream_t s);   // 0 count, 1 fill
void pdf_batch_item(PdfItem& it, const float* sorted_pts, const int* sorted_batch_ids, const int* start_idx, int m, const int* packed,
                    int e_capacity, const int* e_dev, const float* aabb_min, const float* aabb_max, int batch_size, float window,
                    float radius, int scale_inv, float* pdfs, const float* centres = nullptr, void* rec = nullptr, int avg = 0);
int launch_pdf(const PdfItem& it, hipStream_t s);   // one list: 4 or 16 waves per workgroup by its row count
int launch_pdf_batch(const PdfBatch& pb, int count, hipStream_t s);
// pdf_points.hip: the per-point density and its expansion as items (single launches take the same records)
int point_pdf_item(PointPdfItem& it, const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                   const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window, float radius,
                   int scale_inv, float* density, int* counts);
int launch_point_pdf(const PointPdfItem& it, hipStream_t s);
int launch_point_pdf_batch(const PointPdfBatch& pb, int count, hipStream_t s);
int expand_item(ExpandItem& it, const float* density, int n, const int* start_idx, int m, const int* packed, int e_capacity,
                const int* total_dev, float* pdfs);
int launch_expand_dn(const ExpandItem& it, hipStream_t s);
int launch_expand_batch(const ExpandBatch& eb, int count, hipStream_t s);

}  // namespace mccnn
