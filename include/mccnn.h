/*
 * mccnn.h -- C-ABI of the MI355X-native Monte-Carlo convolution library
 * (libmccnn_hip.so, built from mccnn_amd/csrc/ by hipcc for gfx950).
 *
 * This is the drop-in boundary for the reference's tf_ops operators
 * (viscom-ulm/MCCNN, tf_ops .cc/.cu files behind tf_ops/MCConvModuleSrc). One entry
 * point (or a count/fill pair where the output size is data dependent) replaces
 * one registered TF op; each declaration cites the reference interface it
 * replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host;
 *  - the library never allocates, frees or synchronises, except where a
 *    function documents a host read-back (num_cells with scale_inv == 0);
 *    scratch memory is caller-provided (`ws`, size from the matching
 *    *_workspace_bytes query) -- the reference instead cudaMalloc/cudaFree'd
 *    inside its launchers (find_neighbors.cu:298-309, sort_gpu.cu:410-418,
 *    poisson_sampling.cu:202-223);
 *  - every launch goes to the explicit `stream` (a hipStream_t passed as void*;
 *    the reference used the legacy default stream);
 *  - return value: 0 = ok, < 0 = argument error (MCCNN_E_*), > 0 = hipError_t.
 *    The reference aborted the process on CUDA errors (cuda_kernel_utils.h:17-24);
 *    this library never does;
 *  - data layout is the reference's flattened ragged batch:
 *    points [N,3] f32, batch ids [N] i32 (the [N,1] tensor, flat), features
 *    [N,F] f32 row-major, aabb [B,3] f32, cell table [B,nc,nc,nc,2] i32,
 *    start indices [M] i32, packed neighbours [E,2] i32 rows (j, i);
 *  - kernel-MLP weights are addressed FLAT exactly like the reference kernels
 *    (spatial_conv.cu:172): w1[nu*3+d], b1[nu], w2[q*64+n*8+m], b2[nu],
 *    w3[q*64+n*8+m], b3[nu], nu = 8q+n -- although the Python variables are
 *    declared [3,8nb] / [8,8nb] (MCConvBuilder.py:407-419) there is no transpose.
 *  - canonical order: inside a grid cell points keep ascending original index;
 *    Poisson samples are emitted batch -> phase -> cell (launch-linear) -> point.
 *    Both are one valid outcome of the reference's atomics (sort_gpu.cu:170,
 *    poisson_sampling.cu:115) and are reproducible.
 */
#ifndef MCCNN_H_
#define MCCNN_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mccnn_stream_t; /* hipStream_t */

#define MCCNN_OK 0
#define MCCNN_E_BADARG (-1)     /* null pointer / non-positive size            */
#define MCCNN_E_BATCHID (-2)    /* batch id outside [0,B): raised by the binding from mccnn_check_batch_ids */
#define MCCNN_E_TOOLARGE (-3)   /* B*nc^3 or E does not fit int32              */
#define MCCNN_E_WORKSPACE (-4)  /* workspace smaller than *_workspace_bytes    */
#define MCCNN_E_SHAPE (-5)      /* MLP shape rules of spatial_conv.cc:258-300  */

/* generated get_block_size(), genCompileScript.py:46-47 (BLOCK_MLP_SIZE = 8) */
int mccnn_block_size(void);
/* library/ABI version, arch string ("gfx950") */
int mccnn_abi_version(void);
const char* mccnn_arch(void);
const char* mccnn_error_string(int code);

/* Batch ids index per-cloud tables (boxes, cell grids) in every op. The reference never checks them
 * (an id outside [0, batch_size) reads / writes out of bounds: sort_gpu.cu:46-59, aabb_gpu.cu:97-103). Here
 * every kernel clamps the id before it indexes (memory-safe, result unspecified for invalid input) and this
 * asynchronous check counts the invalid ids into *bad_count_dev, for a binding that wants to raise
 * MCCNN_E_BATCHID (costs the caller one 4-byte read-back; mccnn_amd.MCConvModule.CHECK_BATCH_IDS). */
int mccnn_check_batch_ids(const int* batch_ids, int n, int batch_size, int* bad_count_dev,
                          mccnn_stream_t stream);

/* ComputeAabb -- aabb_gpu.cc:22-86, aabb_gpu.cu:57-140.
 * scale_inv == 0: every row receives the whole-batch box (aabb_gpu.cu:104-114). */
size_t mccnn_compute_aabb_workspace_bytes(int batch_size);
int mccnn_compute_aabb(const float* pts, const int* batch_ids, int n, int batch_size, int scale_inv,
                       float* aabb_min, float* aabb_max, void* ws, size_t ws_bytes,
                       mccnn_stream_t stream);

/* determineNumCells -- sort_gpu.cu:374-420. scale_inv != 0: pure host arithmetic.
 * scale_inv == 0: reads the box of batch 0 back to the host (one stream sync,
 * like the reference's cudaMemcpy D2H at sort_gpu.cu:417). */
int mccnn_num_cells(const float* aabb_min, const float* aabb_max, int batch_size, float cell_size,
                    int scale_inv, int* num_cells_host, mccnn_stream_t stream);
/* The box extent mccnn_num_cells(scale_inv = 0) divides by -- max over the axes of aabb_max[0] - aabb_min[0] (batch 0:
 * with scale_inv = 0 every row holds the whole-batch box, aabb_gpu.cu:104-114) -- read back ONCE (24 bytes, this call
 * synchronises the stream). A binding that builds several grids over the same boxes (every level of a PointHierarchy,
 * every convolution radius) computes num_cells = max(1, (int)(extent / cell_size)) in float on the host from it
 * instead of paying the reference's read-back (sort_gpu.cu:410-419) per grid. */
int mccnn_aabb_extent(const float* aabb_min, const float* aabb_max, float* extent_host,
                      mccnn_stream_t stream);

/* SortPointsStep1 -- sort_gpu.cc:23,184-268, sort_gpu.cu:35-174,436-471.
 * keys[i] = b*nc^3 + x*nc^2 + y*nc + z; new_idx[i] = destination of point i in
 * the cell-sorted list (stable: ascending i inside a cell). */
size_t mccnn_sort_step1_workspace_bytes(int n, int batch_size, int num_cells);
int mccnn_sort_step1(const float* pts, const int* batch_ids, const float* aabb_min,
                     const float* aabb_max, int n, int batch_size, int num_cells, int* keys,
                     int* new_idx, void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* SortPointsStep2 -- sort_gpu.cc:40,270-378, sort_gpu.cu:192-248,473-497.
 * Applies the permutation and builds the (first,last+1) cell table; empty cell = (0,0).
 * inv_idx: optional [n] output, inv_idx[new_idx[i]] = i -- the cell-coherent visiting order
 * mccnn_find_neighbors_* take as centre_order for same-level searches; may be NULL. */
size_t mccnn_sort_step2_workspace_bytes(int n);
int mccnn_sort_step2(const float* pts, const int* batch_ids, const float* feats, const int* keys,
                     const int* new_idx, int n, int num_feats, int batch_size, int num_cells,
                     float* out_pts, int* out_batch_ids, float* out_feats, int* cell_indexs,
                     int* inv_idx, void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* out[i,:] = in[idx[i],:], i < n_idx.  Replaces SortPointsStep2Grad (sort_gpu.cu:260),
 * SortFeaturesBack (:288) and GetSampledFeatures (poisson_sampling.cu:135). */
int mccnn_permute_gather(const float* in, const int* idx, int n_idx, int num_feats, float* out,
                         mccnn_stream_t stream);
/* out[idx[i],:] = in[i,:], i < n_idx; zero_fill != 0 first clears out[0:n_out,:].
 * Replaces SortFeaturesBackGrad (sort_gpu.cu:311; this is Python's sort_features(),
 * MCConvModuleSrc:35-36) and GetSampledFeaturesGrad (poisson_sampling.cu:158,262-274). */
int mccnn_permute_scatter(const float* in, const int* idx, int n_idx, int num_feats, float* out,
                          int n_out, int zero_fill, mccnn_stream_t stream);

/* TransformIndexs -- sort_gpu.cc:96,496-533, sort_gpu.cu:332-362.
 * out[s] = inv[in_idx[s]] with inv[new_idx[i]] = i.  ws: n ints. */
size_t mccnn_transform_indexs_workspace_bytes(int n);
int mccnn_transform_indexs(const int* in_idx, int s, const int* new_idx, int n, int* out_idx,
                           void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* FindNeighbors -- find_neighbors.cc:25,80-185, find_neighbors.cu:40-372.
 * count: start_idx[i] = exclusive prefix of the per-centre neighbour counts and
 * *total_dev = E.  total_dev is any DEVICE-ACCESSIBLE int: device memory, or a pinned host
 * word (hipHostMalloc) -- then no device-to-host copy is needed and a host that polls the
 * word sees E as soon as the count retires (the Python layer does this).  The caller reads
 * E, allocates packed[E,2] and calls fill with the same arguments.  Row order: centre ascending; inside a
 * centre the 27-cell table order of find_neighbors.cu:282-291, then ascending j.
 * centre_order (optional, may be NULL): a permutation of 0..m-1 giving the order in
 * which threads visit the centres. It never changes the result; a spatially coherent
 * order (e.g. the inverse of new_idx when the centres are the gridded points) makes
 * neighbouring lanes walk the same cells, which is several times faster. */
size_t mccnn_find_neighbors_workspace_bytes(int m, int n);
int mccnn_find_neighbors_count(const float* centres, const int* centre_batch_ids, int m,
                               const float* sorted_pts, int n, const int* cell_indexs,
                               const float* aabb_min, const float* aabb_max, int batch_size,
                               int num_cells, float radius, int scale_inv, const int* centre_order,
                               int* start_idx, int* total_dev, void* ws, size_t ws_bytes,
                               mccnn_stream_t stream);
/* e: capacity of `packed` in rows. Normally the total the count call produced; a caller that wants
 * to launch the fill before it has read that total back (to hide the read-back behind the kernel)
 * may pass a guess: rows beyond the capacity are simply not written, and if the total turns out
 * larger the call is repeated with a big enough buffer. ws: the workspace of the count call,
 * UNTOUCHED in between -- the count pass leaves the hit masks of every (centre, 64-candidate round)
 * there and the fill pass only compacts them (one traversal of the candidate windows, not two as in
 * find_neighbors.cu:268-372). */
/* The same count with a SECOND destination of the total (extension): total_dev stays on the device for
 * mccnn_compute_pdf_dn, total_host is a pinned host word the caller polls -- no device-to-host copy is enqueued. */
int mccnn_find_neighbors_count2(const float* centres, const int* centre_batch_ids, int m,
                                const float* sorted_pts, int n, const int* cell_indexs,
                                const float* aabb_min, const float* aabb_max, int batch_size, int num_cells,
                                float radius, int scale_inv, const int* centre_order, int* start_idx,
                                int* total_dev, int* total_host, void* ws, size_t ws_bytes,
                                mccnn_stream_t stream);
int mccnn_find_neighbors_fill(const float* centres, const int* centre_batch_ids, int m,
                              const float* sorted_pts, int n, const int* cell_indexs,
                              const float* aabb_min, const float* aabb_max, int batch_size,
                              int num_cells, float radius, int scale_inv, const int* centre_order,
                              const int* start_idx, int e, int* packed, void* ws, size_t ws_bytes,
                              mccnn_stream_t stream);
/* The search with a cap on the neighbours per centre (extension; no counterpart in the reference).
 * max_neighbors = K > 0; 0 makes both calls the uncapped ones above, a negative value is
 * MCCNN_E_BADARG. A centre with k <= K hits keeps its row; one with k > K keeps exactly K of them,
 * those at the canonical ranks floor(t * k / K), t = 0 .. K-1 (64-bit integer arithmetic), in that
 * order -- a stride over the whole row, so every cell of the 27-cell window stays represented in
 * proportion. start_idx = exclusive prefix of min(k, K), *total_dev = E = their total, rows (j, i)
 * at start_idx[i]: the capped list is a subsequence of the uncapped one, row by row, and the same
 * bytes in every run (no atomics, no arrival order). Everything downstream takes the list as it is.
 * Argument lists and protocol of mccnn_find_neighbors_count / _fill (e may be a guess; ws untouched
 * between the calls; the same max_neighbors in both), but the workspace is the larger one of
 * mccnn_find_neighbors_capped_workspace_bytes whenever K > 0: the count pass leaves the true row
 * lengths there for the fill pass. */
size_t mccnn_find_neighbors_capped_workspace_bytes(int m, int n);
int mccnn_find_neighbors_count_capped(const float* centres, const int* centre_batch_ids, int m,
                                      const float* sorted_pts, int n, const int* cell_indexs,
                                      const float* aabb_min, const float* aabb_max, int batch_size,
                                      int num_cells, float radius, int scale_inv,
                                      const int* centre_order, int* start_idx, int* total_dev,
                                      void* ws, size_t ws_bytes, mccnn_stream_t stream,
                                      int max_neighbors);
int mccnn_find_neighbors_fill_capped(const float* centres, const int* centre_batch_ids, int m,
                                     const float* sorted_pts, int n, const int* cell_indexs,
                                     const float* aabb_min, const float* aabb_max, int batch_size,
                                     int num_cells, float radius, int scale_inv,
                                     const int* centre_order, const int* start_idx, int e,
                                     int* packed, void* ws, size_t ws_bytes, mccnn_stream_t stream,
                                     int max_neighbors);
/* The capped fill pass with a fresh stratified sample instead of the canonical ranks (extension).
 * After mccnn_find_neighbors_count_capped with the same max_neighbors = K > 0, over the same
 * workspace; the count pass, start_idx and the total do not depend on the seed. The strata of a row
 * of k > K hits are the canonical ranks [lo_t, lo_{t+1}), lo_t = floor(t * k / K), t = 0 .. K-1
 * (mccnn_find_neighbors_fill_capped keeps offset 0 of each). Slot t holds the hit at rank
 * lo_t + off_t with, all in uint32 arithmetic modulo 2^32,
 *     mix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 *     h = mix(mix(seed + 0x9E3779B9 * (i + 1)) + t)       i = the centre's index in `centres`
 *     off_t = (h * (lo_{t+1} - lo_t)) >> 32               a 64-bit product
 * Rows of k <= K hits are untouched. The list is a subsequence of the uncapped one in canonical
 * order; no atomics and no generator state: the same (inputs, K, seed) give the same bytes in
 * every run. max_neighbors <= 0 is MCCNN_E_BADARG. */
int mccnn_find_neighbors_fill_sampled(const float* centres, const int* centre_batch_ids, int m,
                                      const float* sorted_pts, int n, const int* cell_indexs,
                                      const float* aabb_min, const float* aabb_max, int batch_size,
                                      int num_cells, float radius, int scale_inv,
                                      const int* centre_order, const int* start_idx, int e,
                                      int* packed, void* ws, size_t ws_bytes, mccnn_stream_t stream,
                                      int max_neighbors, unsigned seed);
/* The search with a budget on the EDGES of its list (extension). max_edges = B > 0; max_neighbors =
 * Ku >= 0 (0 = no cap of the caller's). With k_i the uncapped row lengths, kmax = max(max_i k_i, 1)
 * and S(K) = sum_i min(k_i, K) in 64-bit integers, the search picks on the device
 *     K* = max{ K : 1 <= K <= min(Ku, kmax), S(K) <= B }   if S(1) <= B,   K* = 1 otherwise
 * and its output is byte for byte that of the capped pair at max_neighbors = K* (fill: sampled != 0,
 * that of mccnn_find_neighbors_fill_sampled at K* and `seed`). E = S(K*) <= max(B, non-empty rows):
 * every non-empty row keeps one hit, so a budget below m is a floor, not an error; a packed buffer
 * of max(B, m) rows cannot overflow. count: count pass (the capped one, no clamp) -> selection (one
 * launch up to 4096 centres, three above) -> prefix sum of min(k_i, K*); *cap_dev = K*, a
 * device-accessible word the fill pass reads -- nothing returns to the host in between. Integer
 * atomics only: the same inputs give the same K* and the same bytes in every run. Protocol of the
 * capped pair (ws of mccnn_find_neighbors_budget_workspace_bytes untouched between the calls, e may
 * be a guess). max_edges <= 0, max_neighbors < 0, cap_dev == NULL: MCCNN_E_BADARG; m == 0 writes
 * total 0 and cap 1; m > 2^21: MCCNN_E_TOOLARGE. */
size_t mccnn_find_neighbors_budget_workspace_bytes(int m, int n);
int mccnn_find_neighbors_count_budget(const float* centres, const int* centre_batch_ids, int m,
                                      const float* sorted_pts, int n, const int* cell_indexs,
                                      const float* aabb_min, const float* aabb_max, int batch_size,
                                      int num_cells, float radius, int scale_inv,
                                      const int* centre_order, int* start_idx, int* total_dev,
                                      void* ws, size_t ws_bytes, mccnn_stream_t stream,
                                      int max_neighbors, int max_edges, int* cap_dev);
int mccnn_find_neighbors_fill_budget(const float* centres, const int* centre_batch_ids, int m,
                                     const float* sorted_pts, int n, const int* cell_indexs,
                                     const float* aabb_min, const float* aabb_max, int batch_size,
                                     int num_cells, float radius, int scale_inv,
                                     const int* centre_order, const int* start_idx, int e,
                                     int* packed, void* ws, size_t ws_bytes, mccnn_stream_t stream,
                                     const int* cap_dev, int sampled, unsigned seed);
/* inv[new_idx[i]] = i -- the visiting order above for same-level searches (sort_gpu.cu:332-345). */
int mccnn_invert_permutation(const int* new_idx, int n, int* inv, mccnn_stream_t stream);

/* ComputePDF -- compute_pdf.cc:25,57-142, compute_pdf.cu:40-119.
 * mode 0: the reference's arithmetic (double exp per axis, float rounding per
 *         statement, compute_pdf.cu:72-92);
 * mode 1: single precision, the pair sums of a row as 16 x 16 Gram-matrix tiles on the
 *         matrix cores (coordinates relative to the row's first point); agrees with
 *         mode 0 to ~1e-5 relative per value, inside the 1e-4 tolerance of the feature
 *         path; needs no workspace beyond the 256-byte minimum;
 * mode 2: single precision on the VALU (subtract-first pair loop, ~1e-6 relative);
 *         workspace: 16 bytes per edge. */
size_t mccnn_compute_pdf_workspace_bytes(int e, int mode);
int mccnn_compute_pdf(const float* sorted_pts, const int* sorted_batch_ids, const int* start_idx,
                      int m, const int* packed, int e, const float* aabb_min, const float* aabb_max,
                      int batch_size, float window, float radius, int scale_inv, int mode,
                      float* pdfs, void* ws, size_t ws_bytes, mccnn_stream_t stream);
/* ComputePDF with the edge count read from DEVICE memory (single-precision KDE only): packed / pdfs hold
 * e_capacity rows, *e_dev (<= e_capacity expected) of them are valid. Lets a caller that guessed the size of
 * the neighbour list enqueue search and KDE back to back without waiting for the count
 * (ConvolutionBuilder.prefetch_geometry); if *e_dev turns out larger than e_capacity the rows are cut and
 * the caller repeats with the exact size. Workspace: mccnn_compute_pdf_workspace_bytes(e_capacity, 1). */
int mccnn_compute_pdf_dn(const float* sorted_pts, const int* sorted_batch_ids, const int* start_idx, int m,
                         const int* packed, int e_capacity, const int* e_dev, const float* aabb_min,
                         const float* aabb_max, int batch_size, float window, float radius, int scale_inv,
                         float* pdfs, void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* The per-POINT kernel density estimate (extension, pdfMode = 'point'; pdf_points.hip). For every sorted point j of
 * cloud b, over its own ball N(j) = { l of the same cloud : sqrt(d2) < R_b }, R_b = radius * maxExtent_b (scale_inv)
 * or radius -- exactly the row find_neighbors gives with the sorted points as their own centres (the same f32
 * predicate, d2 without FMA against the same threshold):
 *   counts[j]  = |N(j)|
 *   density[j] = sum over l in N(j) of prod_a (1/h) 0.39894228 exp(-0.5 ((p_l,a - p_j,a) / (R_b h))^2),  h = window
 * (single precision, one exp per pair like modes 1 and 2 of mccnn_compute_pdf; 0 for an empty set, which only a cloud
 * of zero extent under a relative radius has). cell_indexs is the grid of sorted_pts (num_cells per axis, built at this
 * radius). ONE launch, no workspace, no memset, no atomics; the kernel writes every element of density[n] and counts[n],
 * the same bytes in every run. Batch ids are clamped to [0, batch_size). n == 0 returns 0 without a launch; n < 0,
 * batch_size <= 0, num_cells <= 0, radius <= 0, window <= 0 or a null pointer: MCCNN_E_BADARG. */
int mccnn_compute_pdf_points(const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                             const float* aabb_min, const float* aabb_max, int batch_size, int num_cells,
                             float window, float radius, int scale_inv, float* density, int* counts,
                             mccnn_stream_t stream);
/* The per-point density spread over the edges of an UNCAPPED neighbour list over the same grid:
 *   pdfs[t] = density[packed[2t]] / float(len_i),  i = packed[2t + 1],
 * len_i = start_idx[i + 1] - start_idx[i] (e - start_idx[m - 1] for the last centre) -- the reference's division by
 * the row length (compute_pdf.cu:92), one correctly rounded f32 divide. On a cloud that lies inside every one of its
 * balls this is mccnn_compute_pdf. One launch, one thread per edge. e == 0 returns 0 without a launch; m < 0, e < 0,
 * m == 0 with e > 0 or a null pointer: MCCNN_E_BADARG. */
int mccnn_expand_pdf(const float* density, const int* start_idx, int m, const int* packed, int e,
                     float* pdfs, mccnn_stream_t stream);
/* Gradients of the two with respect to positions (extension). Every discrete decision of the forward is held fixed:
 * cells, sort order, membership d2 < T, row lengths, the longest box axis. With s_b = 1 / (R_b h),
 * norm = ((1/h) 0.39894228)^3 and w_jl = exp(-0.5 s_b^2 d2_jl):
 *   dpts[j]    = -s_b^2 norm sum_{l in N(j)} (density_grad[j] + density_grad[l]) w_jl (p_j - p_l)
 *   dradius[b] = sum over the points j of cloud b of density_grad[j] norm (s_b^2 / R_b) sum_{l in N(j)} w_jl d2_jl
 * -- the forward's sweep again in gather form (the ball relation is symmetric inside a cloud, so the wave that owns j sums
 * everything that depends on p_j): one launch, no atomics, no per-edge rows, no transposed list; dpts [n, 3] is written
 * whole, a point with an empty ball gets zeros. dradius [batch_size] (dL/dR_b) may be null; non-null needs scale_inv and
 * a workspace of mccnn_compute_pdf_points_bwd_workspace_bytes(n, batch_size) bytes (one float per point, summed per cloud
 * in a fixed order by a second launch; sorted_batch_ids must be non-decreasing, as a sorted list's are). The same bytes
 * in every run. n == 0 returns 0 without a launch; otherwise the argument checks of mccnn_compute_pdf_points
 * (MCCNN_E_BADARG), dradius without scale_inv: MCCNN_E_BADARG, a missing or short workspace: MCCNN_E_WORKSPACE. */
size_t mccnn_compute_pdf_points_bwd_workspace_bytes(int n, int batch_size);
int mccnn_compute_pdf_points_bwd(const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs,
                                 const float* aabb_min, const float* aabb_max, int batch_size, int num_cells,
                                 float window, float radius, int scale_inv, const float* density_grad, float* dpts,
                                 float* dradius, void* ws, size_t ws_bytes, mccnn_stream_t stream);
/* density_grad[j] = sum over the edges t whose point is j of pdfs_grad[t] / float(len_i), i the centre of t, gathered
 * through the transposed list (start_t [n + 1], perm_t [e]: mccnn_transpose_neighbors) in its order: no float atomics,
 * the same bytes in every run. Every density_grad[j], j < n, is written; a point that no edge names gets 0.f. One launch.
 * n == 0 or e == 0 returns 0 without a launch (nothing is written); m < 0, e < 0, n < 0, m == 0 with e > 0 or a null
 * pointer: MCCNN_E_BADARG. */
int mccnn_expand_pdf_bwd(float* density_grad, const float* pdfs_grad, const int* start_idx, int m, const int* packed,
                         int e, const int* start_t, const int* perm_t, int n, mccnn_stream_t stream);

/* PoissonSampling -- poisson_sampling.cc:26,109-211, poisson_sampling.cu:51-230.
 * count: runs the 27 colour phases, leaves the selection in ws and writes the
 * number of samples S to *total_dev.  fill: emits pts[S,3], batch ids[S] and
 * indices[S] (into the SORTED list) in canonical order.  ws must be preserved
 * between the two calls.
 * mode 0: one launch per phase (27 grid-wide barriers).  mode 1: all phases in one launch, cells
 * wait on per-cell flags of the earlier-phase cells of their window (same samples, same order).
 * The waits are bounded; if one times out *total_dev is set to -1 and the caller repeats the
 * count with mode 0. */
size_t mccnn_poisson_sampling_workspace_bytes(int n, int batch_size, int num_cells);
int mccnn_poisson_sampling_count(const float* sorted_pts, const int* sorted_batch_ids, int n,
                                 const int* cell_indexs, const float* aabb_min,
                                 const float* aabb_max, int batch_size, int num_cells, float radius,
                                 int scale_inv, int mode, int* total_dev, void* ws, size_t ws_bytes,
                                 mccnn_stream_t stream);
int mccnn_poisson_sampling_fill(const float* sorted_pts, int n, const int* cell_indexs,
                                int batch_size, int num_cells, int s, float* out_pts,
                                int* out_batch_ids, int* out_indexs, void* ws, size_t ws_bytes,
                                mccnn_stream_t stream);

/* SpatialConv -- spatial_conv.cc:24,159-321, spatial_conv.cu:24-325,796-871.
 * out[M, combin ? num_out_feats : num_in_feats].  Every output row is written
 * (no pre-zeroing needed).
 * state: optional device buffer of mccnn_spatial_conv_state_bytes() bytes (0 = this layer shape
 * keeps no state). The forward pass leaves there what it has computed anyway and the backward pass
 * needs again: one 16-byte record (delta, 1 / (pdf K)) per edge and, for combin layers with one
 * input feature, the per-centre sums of the factored algorithm; handing the same buffer to
 * mccnn_spatial_conv_bwd saves it its pre-pass over the edges (and, for those layers, one more).
 * NULL is always allowed (the reference op has no such output: SpatialConvGrad then recomputes).
 * Shapes: the six MLP tensors hold 8 * ceil(neurons / 8) neurons, neurons = num_in_feats *
 * num_out_feats (combin; the padded count must be a multiple of num_in_feats, spatial_conv.cc:290) or
 * num_in_feats (depth-wise, num_out_feats == num_in_feats). A depth-wise layer may have ANY width:
 * the reference's op wrapper asks for num_in_feats % 8 == 0 (spatial_conv.cc:292-296), its kernels do
 * not, and neither do these -- the last block's neurons beyond num_in_feats are padding. Feature rows,
 * outputs and out-gradients need 4-byte alignment only (16-byte aligned rows of a multiple of 8
 * features take the vector kernels). MCCNN_E_SHAPE otherwise. */
size_t mccnn_spatial_conv_state_bytes(int m, int e, int num_in_feats, int num_out_feats, int combin);
size_t mccnn_spatial_conv_fwd_workspace_bytes(int m, int e, int num_in_feats, int num_out_feats,
                                              int combin);
int mccnn_spatial_conv_fwd(const float* sorted_pts, const float* sorted_feats,
                           const int* sorted_batch_ids, const float* pdfs, const float* samples,
                           const int* start_idx, const int* packed, const float* aabb_min,
                           const float* aabb_max, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* w3, const float* b3, int n, int m, int e,
                           int num_in_feats, int num_out_feats, int combin, int batch_size,
                           float radius, int scale_inv, int avg, float* out, void* state,
                           void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* SpatialConvGrad -- spatial_conv.cc:56,323-519, spatial_conv.cu:327-792,873-966.
 * Gradients w.r.t. the features and the six MLP tensors only
 * (MCConvModuleSrc:74-81).  All seven outputs are fully written; gradients of
 * padded output neurons (nu >= neuronsOut), which the reference leaves
 * uninitialised (spatial_conv.cu:921,924), are zero. state: the buffer the forward call of the
 * SAME inputs filled, or NULL. start_t / perm_t: optional transposed neighbour list (see
 * mccnn_transpose_neighbors): depth-wise layers need it (built internally when NULL); combin layers
 * with 2..4 input features use it IF supplied -- their feature gradient is then gathered in a fixed
 * order instead of added with float atomics (bit-reproducible); NULL keeps the atomics. */
size_t mccnn_spatial_conv_bwd_workspace_bytes(int n, int m, int e, int num_in_feats,
                                              int num_out_feats, int combin);
int mccnn_spatial_conv_bwd(const float* sorted_pts, const float* sorted_feats,
                           const int* sorted_batch_ids, const float* pdfs, const float* samples,
                           const int* start_idx, const int* packed, const float* aabb_min,
                           const float* aabb_max, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* w3, const float* b3, const float* out_grad,
                           int n, int m, int e, int num_in_feats, int num_out_feats, int combin,
                           int batch_size, float radius, int scale_inv, int avg, const void* state,
                           const int* start_t, const int* perm_t, float* feat_grad, float* dw1, float* db1, float* dw2,
                           float* db2, float* dw3, float* db3, void* ws, size_t ws_bytes,
                           mccnn_stream_t stream);

/* bf16 FEATURE STORAGE for depth-wise layers (extension, BASELINE cfg3; the reference is f32-only).
 * Same operators as mccnn_spatial_conv_fwd / _bwd with combin == 0, but the gathered rows -- features
 * [n, num_feats], outputs [m, num_feats], out-gradients and feature gradients -- are stored as bf16
 * (two-byte elements, round-to-nearest-even on store, widened exactly on load); the kernel-MLP
 * tensors, every product and every accumulation stay f32. These layers are bound by the gather of
 * 4 * Fin bytes per edge and direction: bf16 rows halve that. Requirements: num_feats % 8
 * == 0, (num_feats + 7) / 8 <= 64 blocks, 16-byte aligned row buffers; otherwise MCCNN_E_SHAPE.
 * Workspace sizes: the f32 queries with num_in_feats = num_out_feats = num_feats, combin = 0. */
int mccnn_spatial_conv_fwd_bf16(const float* sorted_pts, const void* sorted_feats_bf16,
                                const int* sorted_batch_ids, const float* pdfs, const float* samples,
                                const int* start_idx, const int* packed, const float* aabb_min,
                                const float* aabb_max, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, int n, int m, int e,
                                int num_feats, int batch_size, float radius, int scale_inv, int avg,
                                void* out_bf16, void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_spatial_conv_bwd_bf16(const float* sorted_pts, const void* sorted_feats_bf16,
                                const int* sorted_batch_ids, const float* pdfs, const float* samples,
                                const int* start_idx, const int* packed, const float* aabb_min,
                                const float* aabb_max, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3,
                                const void* out_grad_bf16, int n, int m, int e, int num_feats,
                                int batch_size, float radius, int scale_inv, int avg, const int* start_t,
                                const int* perm_t, void* feat_grad_bf16, float* dw1, float* db1, float* dw2,
                                float* db2, float* dw3, float* db3, void* ws, size_t ws_bytes,
                                mccnn_stream_t stream);

/* Transposed neighbour list (CSR by neighbour index j): start_t[n+1] and perm_t[e] = edge ids
 * grouped by j, ascending inside a row. Depth-wise SpatialConvGrad needs it to compute the
 * feature gradient without float atomics; pass the pair to mccnn_spatial_conv_bwd (start_t /
 * perm_t, both may be NULL -> built internally on every call) to amortise it over the layers
 * that share one neighbour list, as ConvolutionBuilder's caches do (MCConvBuilder.py:366-376). */
size_t mccnn_transpose_neighbors_workspace_bytes(int n, int e);
int mccnn_transpose_neighbors(const int* packed, int e, int n, int* start_t, int* perm_t, void* ws,
                              size_t ws_bytes, mccnn_stream_t stream);

/* GRADIENTS WITH RESPECT TO POSITIONS (extension, no TF counterpart: the reference differentiates spatial_conv w.r.t.
 * the features and the six kernel-MLP tensors only). Every discrete decision of the forward pass -- cells, sort order,
 * neighbour sets, the K of `avg`, the longest box axis -- is held fixed; the results are the exact f32 derivatives of
 * the forward arithmetic. No float atomics: two calls give bit-identical results.
 *
 * mccnn_spatial_conv_bwd_points: the derivative of spatial_conv through delta = (p_j - c_i) / R_b and the 1 / (pdf K)
 * factor, for out_grad [m, out_feats] (f32 even when the feature rows are bf16 storage, feats_bf16 = 1). Outputs:
 *   dpts_edge [e, 3]  per-edge gradient of the neighbour point (sum it per point with mccnn_edge_grad_reduce);
 *   dsamples  [m, 3]  gradient of the centres;
 *   dpdfs     [e]     gradient of the PDFs (optional: NULL skips it);
 *   dradius   [B]     gradient of R_b (optional, scale_inv only; its chain to the box is R_b = radius * maxExtent_b).
 * Every layer shape of mccnn_spatial_conv_bwd (combin and depth-wise, any Fin, avg on / off). Workspace (only with
 * dradius): mccnn_spatial_conv_bwd_points_workspace_bytes(m, batch_size).
 *
 * mccnn_compute_pdf_bwd_points: the derivative of compute_pdf (any mode: the analytic f32 derivative of the KDE sum)
 * for pdf_grad [e]: every pair of a centre's row contributes to both of its points. Writes (accumulate = 0) or adds
 * to (accumulate = 1) dpts_edge [e, 3]; dradius [B] as above (optional, scale_inv only; workspace then
 * mccnn_compute_pdf_bwd_points_workspace_bytes(m, batch_size)).
 *
 * mccnn_edge_grad_reduce: dpts[j] = sum of dpts_edge[t] over the edges t whose neighbour is j, in the order of the
 * transposed list of mccnn_transpose_neighbors (start_t [n + 1], perm_t [e]). Every row of dpts is written. */
size_t mccnn_spatial_conv_bwd_points_workspace_bytes(int m, int batch_size);
int mccnn_spatial_conv_bwd_points(const float* sorted_pts, const void* sorted_feats, int feats_bf16,
                                  const int* sorted_batch_ids, const float* pdfs, const float* samples,
                                  const int* start_idx, const int* packed, const float* aabb_min,
                                  const float* aabb_max, const float* w1, const float* b1, const float* w2,
                                  const float* b2, const float* w3, const float* b3, const float* out_grad, int n,
                                  int m, int e, int num_in_feats, int num_out_feats, int combin, int batch_size,
                                  float radius, int scale_inv, int avg, float* dpts_edge, float* dsamples,
                                  float* dpdfs, float* dradius, void* ws, size_t ws_bytes, mccnn_stream_t stream);
size_t mccnn_compute_pdf_bwd_points_workspace_bytes(int m, int batch_size);
int mccnn_compute_pdf_bwd_points(const float* sorted_pts, const int* sorted_batch_ids, const int* start_idx, int m,
                                 const int* packed, int e, const float* aabb_min, const float* aabb_max,
                                 int batch_size, float window, float radius, int scale_inv, const float* pdf_grad,
                                 int accumulate, float* dpts_edge, float* dradius, void* ws, size_t ws_bytes,
                                 mccnn_stream_t stream);
int mccnn_edge_grad_reduce(const float* dpts_edge, const int* start_t, const int* perm_t, int n, int e, float* dpts,
                           mccnn_stream_t stream);

/* DEVICE-SIDE POINT COUNTS (hierarchy construction without per-level host read-backs).
 * PointHierarchy (MCConvBuilder.py:101-128) chains sort -> Poisson sampling -> transform_indexs level
 * after level, and the reference reads the number of samples back to the host at every level
 * (poisson_sampling.cu:222) because it sizes the next level's launches. These variants take the
 * number of valid points from DEVICE memory (*n_dev <= n_cap; launches and buffers are sized by the
 * capacity n_cap), so a caller can run all levels back to back -- mccnn_poisson_sampling_count /_fill
 * already work from the cell table and take n_cap as n -- and read every level's size back ONCE at the
 * end. Same results as the host-count forms. sort_step2_dn moves geometry only (feature rows are
 * gathered once the sizes are known). */
int mccnn_sort_step1_dn(const float* pts, const int* batch_ids, const float* aabb_min,
                        const float* aabb_max, int n_cap, const int* n_dev, int batch_size,
                        int num_cells, int* keys, int* new_idx, void* ws, size_t ws_bytes,
                        mccnn_stream_t stream);
int mccnn_sort_step2_dn(const float* pts, const int* batch_ids, const int* keys, const int* new_idx,
                        int n_cap, const int* n_dev, int batch_size, int num_cells, float* out_pts,
                        int* out_batch_ids, int* cell_indexs, void* ws, size_t ws_bytes,
                        mccnn_stream_t stream);
/* One level of a point hierarchy in one call (extension; MCConvBuilder.py:101-128 per level): mccnn_sort_step1_dn +
 * mccnn_sort_step2_dn + mccnn_poisson_sampling_count / _fill + mccnn_transform_indexs_dn with the level's point count in
 * device memory (n_dev) and the sample count left there (s_dev, -1 when a wait of the single-launch Poisson form timed
 * out: the caller repeats the level op by op). Outputs are sized by n_cap. */
size_t mccnn_hierarchy_level_workspace_bytes(int n_cap, int batch_size, int num_cells);
int mccnn_hierarchy_level(const float* pts, const int* batch_ids, const float* aabb_min, const float* aabb_max,
                          int n_cap, const int* n_dev, int batch_size, int num_cells, float radius,
                          int scale_inv, int mode, int* new_idx, float* sorted_pts, int* sorted_batch_ids,
                          int* cell_indexs, float* out_pts, int* out_batch_ids, int* out_indexs,
                          int* transformed_indexs, int* s_dev, void* ws, size_t ws_bytes,
                          mccnn_stream_t stream);
/* SortPointsStep1 + SortPointsStep2 of the POINTS only in one call (extension: what a convolution builder needs of a
 * grid is the sorted points / batch ids, the cell table and index_new_pos -- feature rows are sorted where they are
 * consumed). Same outputs as the two ops; inv_idx (optional): the inverse permutation (sorted position -> input row). */
size_t mccnn_build_grid_workspace_bytes(int n, int batch_size, int num_cells);
int mccnn_build_grid(const float* pts, const int* batch_ids, const float* aabb_min, const float* aabb_max, int n,
                     int batch_size, int num_cells, int* new_idx, float* out_pts, int* out_batch_ids,
                     int* cell_indexs, int* inv_idx, void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_transform_indexs_dn(const int* in_idx, int s_cap, const int* s_dev, const int* new_idx,
                              int n_cap, const int* n_dev, int* out_idx, void* ws, size_t ws_bytes,
                              mccnn_stream_t stream);

/* ROW-PER-LANE LAYOUTS of a neighbour list (extension; no counterpart in the reference, whose kernels walk the list
 * with 8 threads per (edge, block) and float atomics -- spatial_conv.cu:104-176,477-561).
 * A plan stores a CSR list in SELL-64-sigma form. Rows (centres for the forward plan, neighbour points for the
 * transposed plan) longer than 128 edges are cut into VIRTUAL rows of at most 128 edges; virtual rows are sorted by
 * length inside windows of 1024 (taken in the visiting order of the rows) and cut into slices of 64; slice s holds
 * (longest virtual row in s) x 64 slots, slot (it, lane) = edge #it of the lane's virtual row: a 16-byte record
 * (delta0, delta1, delta2, 1 / (pdf K)) and the index of the row at the other end of the edge, zero records as padding.
 * With it a lane owns a ROW: the sum over a centre's edges is a per-lane accumulator instead of a segmented wave scan,
 * and the backward pass finishes the feature-gradient row of a point in the same sweep that feeds the weight-gradient
 * sums (mccnn_spatial_conv_fwd_rows / _bwd_rows). One plan serves every layer over the same neighbour list, PDFs,
 * radius and avg flag.
 * Every size is a function of (rows, e) -- mccnn_rowplan_sizes: num_slices S, slot_capacity (a window's slices hold
 * at most 64 x 128 + its edges slots, so e + 8192 x windows bounds the total), scratch_rows (bound on the number of
 * virtual rows: pieces of cut rows leave their partial sums in one scratch row each) -- so a plan is laid out and
 * filled WITHOUT any host read-back.
 *   layout: plan_vrow[64 S] (row of (slice, lane), -1 = padding lane), plan_vcode[64 S] (virtual row id v of (slice,
 *           lane) when its row is cut, ~v when it is not), slice_off[S + 1] (first slot of every slice; slices beyond
 *           the last virtual row are empty), vpos_row[rows] (first virtual row id of every row). row_start: CSR offsets
 *           of the rows (start_idx with rows = m for the forward plan; start_t of mccnn_transpose_neighbors with
 *           rows = n for the transposed one; entry `rows` is not read, e closes the last row). order: optional
 *           cell-coherent visiting order of the rows (a permutation; only affects locality). Deterministic.
 *   fill:   permutes the per-edge records of mccnn_edge_records into slot order. rec: 16 bytes per slot, other: 4
 *           bytes per slot, both slot_capacity long. */
int mccnn_rowplan_sizes(int rows, int e, int* num_slices, long long* slot_capacity, long long* scratch_rows);
size_t mccnn_rowplan_workspace_bytes(int rows, int e);
int mccnn_rowplan_layout(const int* row_start, int rows, int e, const int* order, int* plan_vrow,
                         int* plan_vcode, int* slice_off, int* vpos_row, void* ws, size_t ws_bytes,
                         mccnn_stream_t stream);
/* Per-edge records (delta0, delta1, delta2, 1 / (pdf K)) in EDGE order, 16 bytes each -- the same bits the forward
 * pass leaves in its state buffer (mccnn_spatial_conv_state_bytes): written once per (list, PDFs, radius, avg) and
 * permuted into both plans by mccnn_rowplan_fill. */
int mccnn_edge_records(const float* sorted_pts, const int* sorted_batch_ids, const float* pdfs,
                       const float* samples, const int* start_idx, const int* packed, const float* aabb_min,
                       const float* aabb_max, int n, int m, int e, int batch_size, float radius,
                       int scale_inv, int avg, void* rec_edges, mccnn_stream_t stream);
int mccnn_rowplan_fill(int transposed, const void* rec_edges, const int* packed, int rows, int e,
                       const int* row_start, const int* perm_t, const int* plan_vrow,
                       const int* plan_vcode, const int* slice_off, const int* vpos_row, void* rec,
                       int* other, mccnn_stream_t stream);

/* The whole plan in ONE call and ONE buffer (what a step of a network pays per neighbour list and direction is host
 * work: five calls and seven allocations cost more than the kernels of a coarse level's list).
 * mccnn_rowplan_buffer: byte offsets of {plan_vrow, plan_vcode, slice_off, vpos_row, plan_other, plan_rec} inside a
 * plan buffer of total_bytes for (rows, e), plus the three sizes of mccnn_rowplan_sizes.
 * mccnn_rowplan_build = [mccnn_transpose_neighbors] + mccnn_rowplan_layout + [mccnn_edge_records] +
 * mccnn_rowplan_fill into that buffer. transposed != 0: rows = the n points; start_t [n + 1] / perm_t [e] are written
 * first unless tlist_ready != 0. rec_edges [e x 16 bytes] is written unless rec_ready != 0 (it serves both plans of a
 * list). order: optional visiting order of the rows (forward plans). */
int mccnn_rowplan_buffer(int rows, int e, long long offsets[6], long long* total_bytes, int* num_slices,
                         long long* slot_capacity, long long* scratch_rows);
size_t mccnn_rowplan_build_workspace_bytes(int rows, int e, int transposed);
/* Sizes of the plan buffer and of the build's workspace that hold for EVERY edge count 0 .. e_cap (for a caller that
 * allocates before the list's true size is known). */
int mccnn_rowplan_bound(int rows, int e_cap, int transposed, long long* buffer_bytes, long long* ws_bytes);
/* 1 when mccnn_rowplan_build evaluates the records of a plan of (rows, e) inside its fill (small lists): rec_edges may then
 * be NULL and is neither read nor written. */
int mccnn_rowplan_inline_records(int rows, int e);
int mccnn_rowplan_build(int transposed, const float* sorted_pts, const int* sorted_batch_ids, const float* pdfs,
                        const float* samples, const int* start_idx, const int* packed, const float* aabb_min,
                        const float* aabb_max, int n, int m, int e, int batch_size, float radius, int scale_inv,
                        int avg, const int* order, void* rec_edges, int rec_ready, int* start_t, int* perm_t,
                        int tlist_ready, void* plan_buffer, void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* SpatialConv / SpatialConvGrad for DEPTH-WISE layers (combin == 0, num_feats % 8 == 0, 16-byte aligned rows) over a
 * row plan -- same results as mccnn_spatial_conv_fwd / _bwd (spatial_conv.cu:178-325,563-792) up to float summation
 * order. fwd_rows takes the FORWARD plan (rows = the m centres); bwd_rows takes the TRANSPOSED plan (rows = the n
 * points, start_t = its row offsets) and evaluates the kernel MLP once per (edge, block) for the feature gradient and
 * the six parameter gradients together (the edge-major form needs a second pass over the transposed list). bf16 != 0:
 * rows (features, outputs, out-gradients, feature gradients) stored as bf16 like mccnn_spatial_conv_*_bf16. scratch:
 * scratch_rows x num_feats floats (mccnn_rowplan_sizes). Every output row is written exactly once; no atomics;
 * bit-reproducible. feat_index (optional, NULL = none): sorted_feats (and feat_grad) hold the rows of the points in
 * another order -- row j of the sorted list is row feat_index[j] there (the grid's inverse permutation: the features of
 * the UNSORTED points are read where they lie and their gradient written back in that order, no sorted copy). */
int mccnn_spatial_conv_fwd_rows(const float* sorted_pts, const void* sorted_feats,
                                const int* sorted_batch_ids, const float* pdfs, const float* samples,
                                const int* start_idx, const int* packed, const float* aabb_min,
                                const float* aabb_max, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, int n, int m, int e,
                                int num_feats, int batch_size, float radius, int scale_inv, int avg,
                                int bf16, const int* plan_vrow, const int* plan_vcode,
                                const int* slice_off, const int* vpos_row, const void* plan_rec,
                                const int* plan_other, void* out, float* scratch, const int* feat_index,
                                mccnn_stream_t stream);
size_t mccnn_spatial_conv_bwd_rows_workspace_bytes(int n, int e, int num_feats);
int mccnn_spatial_conv_bwd_rows(const float* sorted_pts, const void* sorted_feats,
                                const int* sorted_batch_ids, const float* pdfs, const float* samples,
                                const int* start_idx, const int* packed, const float* aabb_min,
                                const float* aabb_max, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* b3, const void* out_grad,
                                int n, int m, int e, int num_feats, int batch_size, float radius,
                                int scale_inv, int avg, int bf16, const int* start_t,
                                const int* plan_vrow, const int* plan_vcode, const int* slice_off,
                                const int* vpos_row, const void* plan_rec, const int* plan_other,
                                void* feat_grad, float* scratch, float* dw1, float* db1, float* dw2,
                                float* db2, float* dw3, float* db3, const int* feat_index, void* ws,
                                size_t ws_bytes, mccnn_stream_t stream);

/* NATIVE STEP EXECUTOR (extension; what ConvolutionBuilder.create_convolution, MCConvBuilder.py:336-427, does around
 * the ops): one call per convolution GEOMETRY and one per layer and direction instead of ~12 op calls, because a step of
 * a network is bound by the host issuing its launches, not by the kernels. Built on the entry points above --
 * identical launches, identical results.
 *
 * mccnn_geometry_t: the grid of the input level at the convolution radius (sort_points_step1/2 of the points), the
 * neighbour list of the output level's points in it (find_neighbors) and its PDFs (compute_pdf) -- one cache entry each
 * of cacheGrids_ / cacheNeighs_ / cachePDFs_ (MCConvBuilder.py:349-391) -- in ONE caller-provided device buffer of
 * mccnn_geometry_bytes(). The host object is created / destroyed by the library (no device memory behind it).
 * build: enqueues everything WITHOUT a host wait. e_capacity: rows of the neighbour list the buffer holds (the caller's
 * guess, e.g. the total of the last batch of this shape); the true total E is stored by the count pass into
 * *total_host, a PINNED host word owned by the caller that has to stay valid until the total has been read
 * (mccnn_geometry_edges, or the first mccnn_conv_* call, which wait for it). E > e_capacity: every mccnn_conv_* call
 * returns MCCNN_E_CAPACITY and the caller builds again with a larger buffer. grid_from: optional geometry over the same
 * points, boxes and cell count whose grid is shared instead of built again (keyGrid hit with another output level);
 * it has to outlive this one. use_pdf == 0: PDFs of 1 (MCConvBuilder.py:388-390). All input pointers are borrowed
 * until the geometry is destroyed or built again. The *_capped entries further down build the same geometry over a
 * capped (or sampled) neighbour list. */
#define MCCNN_E_CAPACITY (-6)   /* neighbour list longer than the e_capacity a geometry was built with */
typedef struct mccnn_geometry mccnn_geometry_t;
mccnn_geometry_t* mccnn_geometry_create(void);
void mccnn_geometry_destroy(mccnn_geometry_t* g);
size_t mccnn_geometry_bytes(int n, int m, int batch_size, int num_cells, int e_capacity, int with_grid);
int mccnn_geometry_build(mccnn_geometry_t* g, const float* pts, const int* batch_ids, int n, const float* centres,
                         const int* centre_batch_ids, int m, const float* aabb_min, const float* aabb_max,
                         int batch_size, int num_cells, float radius, int scale_inv, float window, int use_pdf,
                         int e_capacity, const mccnn_geometry_t* grid_from, void* buffer, size_t buffer_bytes,
                         int* total_host, mccnn_stream_t stream);

/* Several geometries of a network step in ONE call (extension): one launch per kernel KIND over all of them -- head clear,
 * keys + histogram, prefix sums of the cell counters, park, rank + move + cell tables, count pass, prefix sums of the counts,
 * fill pass, KDE: nine launches whatever `count` is (per geometry the chain of mccnn_geometry_build is nine as well; requests
 * with a per-point density add two kinds, the density sweep and the expansion: mccnn_geometry_build_batch_point) -- with
 * results identical to mccnn_geometry_build bit for bit. A request that shares the grid of another request names that
 * request's geometry in grid_from and comes AFTER it. */
typedef struct mccnn_geometry_request {
    mccnn_geometry_t* geometry;
    const float* pts; const int* batch_ids; int n;
    const float* centres; const int* centre_batch_ids; int m;
    const float* aabb_min; const float* aabb_max;
    int batch_size, num_cells;
    float radius; int scale_inv; float window; int use_pdf; int e_capacity;
    const mccnn_geometry_t* grid_from;
    void* buffer; size_t buffer_bytes;
    int* total_host;
} mccnn_geometry_request;
int mccnn_geometry_build_batch(const mccnn_geometry_request* requests, int count, mccnn_stream_t stream);

/* The same geometries over a CAPPED neighbour list (extension; mccnn_find_neighbors_count_capped / _fill_capped /
 * _fill_sampled in the geometry's chain): at most max_neighbors rows per centre, the canonical ranks floor(t k / K) of an
 * over-full row or, with sampled != 0, the stratified sample of `seed`. max_neighbors == 0: no cap (the entries above are
 * these with no cap); sampled != 0 with max_neighbors == 0: MCCNN_E_BADARG. A capped list has at most m * max_neighbors
 * rows: an e_capacity of that size never overflows. The buffer of a capped geometry is sized by
 * mccnn_geometry_bytes_capped (the capped search keeps m more words: mccnn_find_neighbors_capped_workspace_bytes); with
 * max_neighbors == 0 it equals mccnn_geometry_bytes. Lists of <= 4096 centres run count -> fill (the fill pass scans the
 * capped counts itself), larger ones count -> scan -> fill, as without a cap; the bytes are those of the op-level capped
 * calls. A geometry that shares a grid (grid_from) may be capped or not independently of the grid's owner.
 * mccnn_geometry_build_batch_capped: caps[k] belongs to requests[k]; caps == NULL: no request is capped. The count and the
 * fill pass go out once per KIND present in a chunk (uncapped, capped, sampled -- a sampled item's count pass is the
 * capped one); a batch without a capped request issues the launches of mccnn_geometry_build_batch. */
typedef struct mccnn_neighbor_cap { int max_neighbors; int sampled; unsigned seed; } mccnn_neighbor_cap;
size_t mccnn_geometry_bytes_capped(int n, int m, int batch_size, int num_cells, int e_capacity, int with_grid, int max_neighbors);
int mccnn_geometry_build_capped(mccnn_geometry_t* g, const float* pts, const int* batch_ids, int n, const float* centres,
                                const int* centre_batch_ids, int m, const float* aabb_min, const float* aabb_max,
                                int batch_size, int num_cells, float radius, int scale_inv, float window, int use_pdf,
                                int e_capacity, const mccnn_geometry_t* grid_from, void* buffer, size_t buffer_bytes,
                                int* total_host, mccnn_stream_t stream, const mccnn_neighbor_cap* cap);
int mccnn_geometry_build_batch_capped(const mccnn_geometry_request* requests, const mccnn_neighbor_cap* caps, int count,
                                      mccnn_stream_t stream);
/* The PDFs of a geometry from a per-point density (pdfMode='point'): density [n] f32 and counts [n] i32 are the
 * caller's buffers for the grid's points at this window.
 * ready == 0: the build computes them (once, right after the grid) and expands them over the list.
 * ready != 0: they already hold the density of this grid and window, written by work ordered before this call on `stream`,
 *             and the build only expands.
 * The chain of one geometry then is [head clear] grid build [density sweep] [visiting order] count (scan) fill expansion:
 * the sweep is mccnn_compute_pdf_points (the same bytes), the expansion mccnn_expand_pdf reading the edge total from the
 * geometry's device word, in the place of the KDE -- whose workspace stays unused; the geometry buffer is that of
 * mccnn_geometry_bytes, the density lives outside it. point == NULL, points == NULL or an entry with density == NULL: edge
 * mode, the launches and bytes of the entries above. A point request needs use_pdf != 0 and no cap, and both pointers:
 * MCCNN_E_BADARG otherwise (a per-point density over a capped row is far noisier than the per-edge one, see README).
 * mccnn_geometry_build_batch_point: points[k] belongs to requests[k]. Beside the nine launches of a chunk there are two
 * further kinds: ONE density sweep behind the grid phases over the distinct `density` pointers of the chunk that are not
 * ready, and ONE expansion over its point geometries in front of the KDE launch of its edge geometries (which is left out
 * when there is none). Several requests may name the same density: the first one that is not ready computes it, the others
 * come AFTER it in the array and only expand (the rule of grid_from), in whichever chunk or chain they end up. */
typedef struct mccnn_point_pdf { float* density; int* counts; int ready; } mccnn_point_pdf;
int mccnn_geometry_build_point(mccnn_geometry_t* g, const float* pts, const int* batch_ids, int n, const float* centres,
                               const int* centre_batch_ids, int m, const float* aabb_min, const float* aabb_max,
                               int batch_size, int num_cells, float radius, int scale_inv, float window, int use_pdf,
                               int e_capacity, const mccnn_geometry_t* grid_from, void* buffer, size_t buffer_bytes,
                               int* total_host, mccnn_stream_t stream, const mccnn_neighbor_cap* cap,
                               const mccnn_point_pdf* point);
int mccnn_geometry_build_batch_point(const mccnn_geometry_request* requests, const mccnn_neighbor_cap* caps,
                                     const mccnn_point_pdf* points, int count, mccnn_stream_t stream);
/* An edge budget in the geometry's chain (the passes of mccnn_find_neighbors_count_budget / _fill_budget, the same bytes):
 * max_edges = B > 0 lets the search pick, on the device, the largest cap K* <= max_neighbors (0 = no cap of the caller's)
 * whose list has at most B rows (at least 1 per non-empty centre); 0 = no budget: the entries below then ARE the point
 * ones. The chain of one geometry: ... count (unclamped; it clears the budget region) -> selection (1 launch up to 4096
 * centres, 3 above) -> clamped prefix sum -> fill with the cap read from the device word; lists of <= 4096 centres have no
 * scan launch: their fill pass scans min(k, K*) itself (three search launches). cap->sampled is allowed with a cap or a
 * budget. The list holds at most max(B, m) rows: an e_capacity of that size never overflows. The buffer is sized by
 * mccnn_geometry_bytes_budget (the search keeps budget_region bytes behind the capped layout; with max_edges == 0 it equals
 * mccnn_geometry_bytes_capped). max_edges < 0 or a budget together with a per-point density: MCCNN_E_BADARG; more than 2^21
 * centres with a budget: MCCNN_E_TOOLARGE. A budgeted geometry may share the grid of any other geometry and the reverse.
 * mccnn_geometry_build_batch_budget: budgets[k] belongs to requests[k]; budgets == NULL: none. A chunk (<= 16 requests) with
 * budgeted requests adds at most 1 count + 3 + 1 selection + 1 scan + 2 fill launches to those of its other kinds; a batch
 * without one issues the launches of mccnn_geometry_build_batch_point.
 * mccnn_geometry_cap: the device word that holds K* once the build has run (read it in stream order behind the build); NULL
 * for a geometry without a budget, whose cap is the max_neighbors the caller passed. */
typedef struct mccnn_neighbor_budget { int max_edges; } mccnn_neighbor_budget;
size_t mccnn_geometry_bytes_budget(int n, int m, int batch_size, int num_cells, int e_capacity, int with_grid, int max_neighbors,
                                   int max_edges);
int mccnn_geometry_build_budget(mccnn_geometry_t* g, const float* pts, const int* batch_ids, int n, const float* centres,
                                const int* centre_batch_ids, int m, const float* aabb_min, const float* aabb_max,
                                int batch_size, int num_cells, float radius, int scale_inv, float window, int use_pdf,
                                int e_capacity, const mccnn_geometry_t* grid_from, void* buffer, size_t buffer_bytes,
                                int* total_host, mccnn_stream_t stream, const mccnn_neighbor_cap* cap,
                                const mccnn_point_pdf* point, const mccnn_neighbor_budget* budget);
int mccnn_geometry_build_batch_budget(const mccnn_geometry_request* requests, const mccnn_neighbor_cap* caps,
                                      const mccnn_point_pdf* points, const mccnn_neighbor_budget* budgets, int count,
                                      mccnn_stream_t stream);
const int* mccnn_geometry_cap(const mccnn_geometry_t* g);
/* PER-EDGE RECORDS FROM THE KDE (extension, ABI 19). The convolution kernels read one 16-byte record per edge, (delta =
 * (p_j - c_i) / R, 1 / (pdf K)) -- mccnn_edge_records. The KDE of a geometry's build has every input of it at hand (the row's
 * centre is uniform over a wave there, K is the row length, the PDF is produced on the spot), so a build that was ASKED for
 * records leaves them beside the PDFs: the same bytes as mccnn_edge_records over the finished list, for the price of one more
 * pass per row inside the KDE kernel instead of a kernel of gathers and divisions per layer.
 * mccnn_geometry_want_records(g, avg): call on the handle BEFORE its build (single or batch); avg = the `avg` flag of the
 *   layers that will read the records (0 / 1), -1 takes the request back. The records live BEHIND the geometry's own pieces in
 *   the build's buffer: hand the build mccnn_geometry_bytes*(...) + mccnn_geometry_records_bytes(e_capacity) bytes. A buffer
 *   without that room, use_pdf = 0, a per-point density or MCCNN_DEBUG=kde_records=0 leave the request without effect: the
 *   geometry is built as without it and the layers evaluate their records themselves.
 * mccnn_geometry_records: the `avg` the geometry's records hold (0 / 1) and their device address (e_capacity records, E
 *   valid), or -1 and NULL when it has none. Records a row plan's build evaluated into an attached buffer are reported too.
 * mccnn_conv_uses_records: 1 when a layer of this shape and `avg` can read the geometry's records -- a combin layer with one
 *   input feature on the factored kernels, records of that `avg` present. Such a layer passes MCCNN_CONV_READS_RECORDS to
 *   mccnn_conv_prepare / _forward / _backward.
 * mccnn_conv_rows_shape (ABI 31): THE rule that sends a layer to the row-per-lane depth-wise kernels (1) or the edge-streaming
 *   ones (0), for a list of e edges over `rows` rows (the centres; backward != 0: the n_points points) whose feature rows
 *   start at `feats`. mccnn_conv_* decide with it, and a caller that runs the layers op by op asks it instead of restating
 *   it (MCConvModule._rows_shape). A pure host function: only the VALUE of `feats` is looked at (16-byte alignment), nothing
 *   is launched, no GPU is needed. It honours MCCNN_ROW_KERNELS and MCCNN_DEBUG=rows_min_degree / rows_force (read once per
 *   process) and bits 0-1 of mccnn_debug_conv_impl. The thresholds: rows_shape() in csrc/exec.hip; their measurements: DESIGN 5b.
 * mccnn_conv_unsorted_max_points (ABI 31): levels of up to this many points whose layer takes the row kernels in both
 *   directions have their feature rows read where they lie, unsorted (MCCNN_DEBUG=unsorted_max_points, default 32768). */
size_t mccnn_geometry_records_bytes(int e_capacity);
int mccnn_geometry_want_records(mccnn_geometry_t* g, int avg);
int mccnn_geometry_records(const mccnn_geometry_t* g, const void** records);
int mccnn_conv_uses_records(const mccnn_geometry_t* g, int num_in_feats, int num_out_feats, int combin, int avg);
int mccnn_conv_rows_shape(int combin, int num_in_feats, const void* feats, int rows, int n_points, int e, int backward);
int mccnn_conv_unsorted_max_points(void);
/* E, or -1 while the count pass has not retired (wait_us: 0 = look once, < 0 = wait, > 0 = wait at most that long). */
int mccnn_geometry_edges(mccnn_geometry_t* g, int wait_us);
/* out[0..7]: device addresses of sortPts [n,3], sortBatchs [n], cellIndexs [B,nc,nc,nc,2], index_new_pos [n], its
 * inverse [n], startIndexs [m], packedNeighs [e_capacity,2], pdfs [e_capacity]; out[8..13]: n, m, num_cells,
 * e_capacity, E (-1 = not read yet), batch_size; out[14]: device word holding E; out[15]: 1 = owns its grid. */
int mccnn_geometry_info(const mccnn_geometry_t* g, long long out[16]);
/* Further pieces a geometry keeps for the layers over it, each in a caller-provided buffer (256-byte aligned) that lives
 * as long as the geometry: what = MCCNN_PIECE_PLAN_FWD (1) forward row plan, _PLAN_TR (2) transposed row plan, _TLIST (4)
 * transposed neighbour list, _RECORDS (8) per-edge records. mccnn_conv_prepare says which are missing and how large they are. */
#define MCCNN_PIECE_PLAN_FWD 1
#define MCCNN_PIECE_PLAN_TR 2
#define MCCNN_PIECE_TLIST 4
#define MCCNN_PIECE_RECORDS 8
int mccnn_geometry_attach(mccnn_geometry_t* g, int what, void* buffer, size_t bytes);
/* Pieces built ahead of the layers that need them (the transposed list and the transposed row plan of a depth-wise
 * layer's backward pass on a side stream, under the forward passes): piece_bytes waits for E and gives the size of the
 * buffer to attach for ONE piece (what = 1, 2, 4 or 8) and the scratch its build needs; prebuild builds the attached
 * pieces named by the mask `what` (row plans need their records / transposed list attached as mccnn_conv_prepare would
 * ask; avg: the flag of the layers that will use the plans). */
int mccnn_geometry_piece_bytes(mccnn_geometry_t* g, int what, long long* bytes, long long* ws_bytes);
/* The same two sizes WITHOUT a geometry and without waiting: bounds for ONE piece over n points, m centres and any list
 * of at most e_cap edges -- for a caller that allocates the pieces when it queues the geometry's build (another thread
 * attaches and prebuilds them once E has arrived). */
int mccnn_geometry_piece_bound(int n, int m, int e_cap, int what, long long* bytes, long long* ws_bytes);
int mccnn_geometry_prebuild(mccnn_geometry_t* g, int what, int avg, void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* The pieces of several geometries at once (extension): what[k] = mask of the pieces of geoms[k] (their buffers attached with
 * mccnn_geometry_attach). One launch per kernel kind over all of them, in flushes of <= 12 small plans (single-workgroup
 * layout, records evaluated inline) and <= 8 large ones (layout, tile fill / bases + records + scatter), their transpositions
 * as batched chains; what a flush cannot take builds as mccnn_geometry_prebuild does, behind them. Results identical to
 * mccnn_geometry_prebuild per geometry (tests/test_gpu_native.py). Waits for the edge totals. */
size_t mccnn_geometry_prebuild_batch_ws_bytes(mccnn_geometry_t* const* geoms, const int* what, int count);
int mccnn_geometry_prebuild_batch(mccnn_geometry_t* const* geoms, const int* what, int count, int avg, void* ws, size_t ws_bytes,
                                  mccnn_stream_t stream);
/* One layer over a geometry: SpatialConv / SpatialConvGrad INCLUDING sort_features / its gradient
 * (MCConvModuleSrc:35-45,70-81). feats [n, num_in_feats] and feat_grad are rows of the UNSORTED points (f32, or bf16
 * with bf16 != 0: depth-wise layers, num_in_feats % 8 == 0); out [m, combin ? num_out_feats : num_in_feats].
 * flags: MCCNN_CONV_KEEP_STATE (bit 0) = keep the forward state for the backward pass, MCCNN_CONV_DETERMINISTIC (bit 1) =
 * deterministic feature gradient of combin layers with 2..4 input features (gathered through the transposed list instead of
 * float atomics), MCCNN_CONV_READS_RECORDS (bit 2) = the layer reads the geometry's per-edge records (only where
 * mccnn_conv_uses_records says 1, and in all three calls of the layer alike): the
 * forward pass neither evaluates nor stores records, `saved` holds the sorted rows and the per-centre sums alone (16 bytes per
 * edge less), and the backward pass reads the same records (or evaluates them afresh, should a row plan of the other `avg`
 * have replaced them in between).
 * prepare (forward or backward): waits for E, then reports need_mask / need_bytes[k] (pieces to attach first, bit k),
 * the scratch bytes of the call and -- forward -- the bytes of `saved`, which the caller keeps from forward to
 * backward (sorted feature rows + forward state). The kernel family (row-per-lane depth-wise kernels, factored one-feature
 * kernels, edge streaming) is decided once per call, by the rule mccnn_conv_rows_shape answers. */
#define MCCNN_CONV_KEEP_STATE 1
#define MCCNN_CONV_DETERMINISTIC 2
#define MCCNN_CONV_READS_RECORDS 4
int mccnn_conv_prepare(mccnn_geometry_t* g, const void* feats, int num_in_feats, int num_out_feats, int combin, int bf16,
                       int backward, int flags, int* need_mask, long long need_bytes[4], long long* ws_bytes,
                       long long* saved_bytes, int* edges);
int mccnn_conv_forward(mccnn_geometry_t* g, const void* feats, int num_in_feats, int num_out_feats, int combin, int avg,
                       int bf16, int flags, const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* w3, const float* b3, void* out, void* saved, size_t saved_bytes, void* ws,
                       size_t ws_bytes, mccnn_stream_t stream);
int mccnn_conv_backward(mccnn_geometry_t* g, const void* feats, const void* saved, size_t saved_bytes,
                        const void* out_grad, int num_in_feats, int num_out_feats, int combin, int avg, int bf16,
                        int flags, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                        const float* b3, void* feat_grad, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                        float* db3, void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* TRAINING BATCHES BUILT ON THE DEVICE (extension; the reference's loader, utils/DataSet.py:711-842, is host Python).
 * The models live in a STORE on the device: their points concatenated, store_pts [store_rows, 3] f32, and optionally
 * their normals, store_normals [store_rows, 3] f32. A batch is described by one HOST record per slot; the kernel selects
 * the points of every slot by its sampling protocol, rotates them and writes
 *   out_pts [out_rows, 3], out_batch_ids [out_rows], out_src [out_rows] (the store row behind every output row: feature,
 *   label and normal rows follow through it with mccnn_permute_gather), counts [num_slots], status [num_slots].
 * Record: the model is store rows [offset, offset + length) with box [bmin, bmax] (f32 minimum / maximum of its points);
 * the slot owns output rows [out_base, out_base + rows) and writes batch_id into each; rot is the row-major 3 x 3 matrix R
 * of out = p R, evaluated as x * r00 + y * r10 + z * r20 left to right in f32. protocol (DataSet.py:666-671), all in f32:
 *   0 uniform   row t of K = rows reads point lo_t + off_t of the first n = n_sel points: lo_t = floor(t n / K),
 *               off_t = (mix(a + t) (lo_{t+1} - lo_t)) >> 32 -- one point per stratum, K distinct ascending indices;
 *               n < K: point (mix(a + t) n) >> 32 (with replacement). a = mix(seed + 0x9E3779B9), mix as in
 *               mccnn_find_neighbors_fill_sampled. counts = K.
 *   1 split     prob = (x - min) / size > 0.5 ? 1 : 0.25 along the longest box axis (the first of equal ones);
 *   2 gradient  prob = sqrt(clip((x - min - 0.2 size) / (0.6 size), 0.01, 1));
 *   3 lambert   prob = sqrt(clip(view . normal, 0, 1));
 *               pass t = 0, 1, .. visits the model in index order and accepts point i when u < prob,
 *               u = (mix(mix(seed + 0x9E3779B9 (t + 1)) + i) >> 8) 2^-24; accepted points are appended in index order.
 *   4 occlusion the orthographic 128 x 128 z-buffer of the points whose normal faces the view (view . normal < 0): a
 *               facing point is kept when its depth lies within 0.01 of its pixel's minimum; no random numbers.
 * exact != 0: the slot produces exactly `rows` rows -- protocols 1-3 repeat passes until they are collected (the last pass
 * is cut at the row that completes them), at most mccnn_batch_max_passes() of them; protocol 4 cycles over its kept points.
 * exact == 0: one pass, counts[slot] <= length rows are written from out_base on (rows >= length is required), the rest of
 * the slot's rows is left untouched and the caller cuts the result by the counts.
 * status[slot]: MCCNN_BATCH_OK; MCCNN_BATCH_NO_POINT: an exact slot whose first pass accepted nothing (no normal faces the
 * view, an empty model); MCCNN_BATCH_PASS_BOUND: short of its rows after the last pass. A slot that gives up fills the rows
 * it did not produce with its model's row 0 (zeros for an empty model): no output byte of an exact slot is undefined.
 * One workgroup per slot, mccnn_batch_sample_chunk() points per iteration; the records travel by value in the kernel
 * arguments, 32 per launch. No workspace, no memset, no float atomics: the same (store, records) give the same bytes.
 * Every record is checked on the host against store_rows and out_rows before anything is launched (MCCNN_E_BADARG, also
 * for protocols 3 and 4 without normals). */
#define MCCNN_BATCH_OK 0
#define MCCNN_BATCH_NO_POINT 1
#define MCCNN_BATCH_PASS_BOUND 2
typedef struct mccnn_batch_slot {
    int offset, length;      /* the model's rows in the store */
    int protocol;            /* 0 .. 4 */
    int rows;                /* output rows the slot owns (exact: produces) */
    int out_base;            /* its first output row */
    int batch_id;            /* written into out_batch_ids */
    int n_sel;               /* protocol 0: draw from the first n_sel <= length points */
    int exact;
    unsigned seed;
    float view[3];
    float rot[9];
    float bmin[3], bmax[3];
} mccnn_batch_slot;
int mccnn_batch_sample_chunk(void);
int mccnn_batch_max_passes(void);
int mccnn_batch_sample(const float* store_pts, const float* store_normals, int store_rows,
                       const mccnn_batch_slot* slots_host, int num_slots, int out_rows, float* out_pts,
                       int* out_batch_ids, int* out_src, int* counts, int* status, mccnn_stream_t stream);

/* THE DENSE GLUE AS ONE OP (extension, ABI 18; bn_act.hip): y = drop(act(bn(x))) over an [n, c] float32 row-major
 * contiguous tensor, n >= 1, c >= 1 -- what the reference's batch_norm_RELU_drop_out and the batch norms of its MLPs
 * compute (utils/MCNetworkUtils.py:20-144).
 *   training: mean_c = (1/n) sum_i x[i,c], var_c = (1/n) sum_i (x[i,c] - mean_c)^2 (biased, for the normalisation AND the
 *             moving average), rstd_c = 1 / sqrt(var_c + eps); moving = moving * momentum + stat * (1 - momentum), in
 *             place. eval (training == 0): mean, var = the moving statistics, nothing is updated, no dropout.
 *   xhat = (x - mean) * rstd; pre = xhat * gamma + beta; act = relu ? max(pre, 0) : pre; backward gate: pre > 0.
 *   dropout (training): element (i, j) is kept iff (uint64) h < keep_threshold, h = mix(row_hash(seed, i) + (uint32) j)
 *             (csrc/bn_drop.h), keep_threshold = floor(keepProb * 2^32) computed by the caller in double; 2^32 = no
 *             dropout. Kept values are multiplied by keep_scale (1.0f / (float) keepProb). No stored mask: the backward
 *             recomputes it from (seed, i, j).
 *   backward (training form): g = dy * mask * keep_scale * gate, dbeta = sum_i g, dgamma = sum_i g * xhat,
 *             dx = gamma * rstd * (g - dbeta / n - xhat * dgamma / n); dx == NULL: not wanted (same dgamma, dbeta bytes).
 * saved = [mean; rstd], [2, c], written by the training forward and read by the backward. Launches: n <= 256 one forward,
 * one backward; otherwise two and two; eval one. No atomics, no memset, a fixed merge order: the same inputs and seed
 * give the same bytes. ws of mccnn_bn_act_workspace_bytes(n, c) bytes (0 for n <= 256 and for eval; ws may then be NULL).
 * n < 1, c < 1, keep_threshold == 0 or > 2^32, a NULL required pointer: MCCNN_E_BADARG; a missing or short workspace:
 * MCCNN_E_WORKSPACE; both before anything is launched. */
size_t mccnn_bn_act_workspace_bytes(int n, int c);
int mccnn_bn_act_fwd(const float* x, int n, int c, const float* gamma, const float* beta,
                     float* moving_mean, float* moving_var, float momentum, float eps,
                     int training, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                     float* y, float* saved /* [2,c]; may be NULL when !training */,
                     void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_bn_act_bwd(const float* x, const float* dy, int n, int c, const float* gamma, const float* beta,
                     const float* saved, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                     float* dx /* NULL: not wanted */, float* dgamma, float* dbeta,
                     void* ws, size_t ws_bytes, mccnn_stream_t stream);
/* ... ON bf16 ROWS (extension, ABI 20): the same op with x and y each float32 (flag 0) or bfloat16 storage (flag 1),
 * independently -- so the op is also the cast between a layer that keeps f32 rows and one that keeps bf16 rows. dy has
 * y's type and dx has x's. gamma, beta, the moving statistics, saved, dgamma, dbeta, the workspace and every intermediate
 * stay f32: bf16 is widened exactly on load, a bf16 result is rounded to nearest even at the store, everything in between
 * is the arithmetic above, operand for operand; the backward recomputes xhat, the gate and the mask from x, saved and the
 * seed and never reads y. For f32 x the statistics, saved and (before the rounding) y are the bytes of mccnn_bn_act_fwd,
 * whatever y's type; for bf16 x they are the same bytes for both types of y. Same launch counts, the same workspace size.
 * bf16 rows move as 32-bit words: an odd c with a bf16 operand, or a bf16 pointer off a 4-byte boundary, is MCCNN_E_SHAPE;
 * a flag outside {0, 1} MCCNN_E_BADARG; both before anything is launched. 16-byte pieces (8 bf16 columns per access) need
 * c % 8 == 0 and 16-byte aligned row pointers, which the entries look at themselves; other rows move as pairs. With both
 * flags 0 these ARE mccnn_bn_act_fwd / _bwd. */
int mccnn_bn_act_fwd_rows(const void* x, int x_bf16, int n, int c, const float* gamma, const float* beta,
                          float* moving_mean, float* moving_var, float momentum, float eps,
                          int training, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                          void* y, int y_bf16, float* saved /* [2,c]; may be NULL when !training */,
                          void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_bn_act_bwd_rows(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, const float* gamma,
                          const float* beta, const float* saved, int relu, unsigned long long keep_threshold,
                          float keep_scale, unsigned seed, void* dx /* x's type; NULL: not wanted */, float* dgamma,
                          float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream);
/* ... OVER A CONCATENATION (extension, ABI 28; typed segments: ABI 30; bn_act.hip): the same op over the column-wise
 * concatenation of nseg segments, 1 <= nseg <= mccnn_bn_act_cat_max_segments() (8), which is never materialised. x_s is
 * [n, c_s] row-major contiguous, c_s >= 1, C = sum c_s, float32 or -- the _rows entries, xs_bf16[s] == 1 -- bfloat16 storage,
 * every segment on its own; y / dy are [n, C], float32 or bfloat16 storage as in the _rows entries of the contiguous op;
 * everything per column ([C], saved [2, C]) is indexed by the global column, and so is the dropout mask: element (row, global
 * column). The backward writes one contiguous dx_s [n, c_s] of x_s's type per segment that wants one (dxs == NULL: none;
 * dxs[s] == NULL: not that one; dgamma and dbeta keep their bytes either way). xs, xs_bf16 (NULL: all float32), cs and dxs are
 * HOST arrays of nseg entries, read before the call returns: the table travels in the kernel arguments, nothing is uploaded.
 * mccnn_bn_act_cat_fwd / _bwd are the _rows entries with xs_bf16 == NULL.
 * The plan is ALWAYS the contiguous op's at (n, C) with float32 x -- grid, 32-column tile, slabs, merge order and the
 * thread -> global column mapping -- also when every segment is bf16; a thread looks its segment up once and reads
 * x_s + r * c_s + (col - col0_s) in the segment's type: bf16 is widened exactly on load and dx_s rounded to nearest even at
 * the store, everything in between is the float32 arithmetic. 4 columns per thread iff every c_s % 4 == 0, every f32 x_s and
 * wanted f32 dx_s is 16-byte aligned, every bf16 x_s and wanted bf16 dx_s 8-byte aligned and y / dy / ws pass the rule of the
 * _rows entries; otherwise 1 (a bf16 element then moves as one 16-bit access).
 * Let w(x_s) be x_s widened to float32 in a fresh allocation. Whenever the op on (x_s) and mccnn_bn_act_cat_fwd / _bwd on
 * (w(x_s)) take the same number of columns per thread -- some c_s % 4 != 0, or every c_s % 4 == 0 and every pointer aligned as
 * above -- y, saved, both moving statistics, dgamma, dbeta and the dx_s of every f32 segment are byte for byte equal, and the
 * dx_s of a bf16 segment is the round-to-nearest-even of the other's f32 dx_s. And whenever the contiguous op takes the same
 * plan on the concatenated f32 tensor -- C % 4 != 0, or every c_s % 4 == 0 and every pointer aligned -- every output is byte
 * for byte that op's (dx_s: the column slice of its dx); nseg == 1 with an f32 segment is always mccnn_bn_act_fwd_rows /
 * _bwd_rows with f32 x. The same launch counts whatever nseg and the types are, ws of mccnn_bn_act_workspace_bytes(n, C)
 * bytes, no atomics, no memset.
 * nseg outside [1, 8], n < 1, a c_s < 1, a bad threshold, a NULL required pointer or a type flag (of y / dy or of a segment)
 * outside {0, 1}: MCCNN_E_BADARG; C > 2^31 - 1: MCCNN_E_TOOLARGE; bf16 y / dy with an odd C or off a 4-byte boundary, a bf16 x_s
 * or wanted dx_s off a 2-byte boundary: MCCNN_E_SHAPE; a missing or short workspace: MCCNN_E_WORKSPACE; all before anything is
 * launched.
 * Not covered: the cross-rank form over segments, a linear layer reading segments, more than 8 segments. */
int mccnn_bn_act_cat_max_segments(void);
int mccnn_bn_act_cat_fwd(const float* const* xs, const int* cs, int nseg, int n, const float* gamma, const float* beta,
                         float* moving_mean, float* moving_var, float momentum, float eps,
                         int training, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                         void* y, int y_bf16, float* saved /* [2,C]; may be NULL when !training */,
                         void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_bn_act_cat_bwd(const float* const* xs, const int* cs, int nseg, const void* dy, int dy_bf16, int n,
                         const float* gamma, const float* beta, const float* saved, int relu,
                         unsigned long long keep_threshold, float keep_scale, unsigned seed,
                         float* const* dxs /* NULL: none wanted; entries may be NULL */, float* dgamma, float* dbeta,
                         void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_bn_act_cat_fwd_rows(const void* const* xs, const int* xs_bf16 /* NULL: all float32 */, const int* cs, int nseg, int n,
                              const float* gamma, const float* beta, float* moving_mean, float* moving_var, float momentum,
                              float eps, int training, int relu, unsigned long long keep_threshold, float keep_scale,
                              unsigned seed, void* y, int y_bf16, float* saved /* [2,C]; may be NULL when !training */,
                              void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_bn_act_cat_bwd_rows(const void* const* xs, const int* xs_bf16 /* NULL: all float32 */, const int* cs, int nseg,
                              const void* dy, int dy_bf16, int n, const float* gamma, const float* beta, const float* saved,
                              int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                              void* const* dxs /* dx_s has x_s's type; NULL: none wanted; entries may be NULL */,
                              float* dgamma, float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream);
/* ... WITH BATCH STATISTICS ACROSS RANKS (extension, ABI 22; bn_act.hip): the training form of the same op when the rows of
 * a batch are sharded over the `world` ranks of a process group. n, mean and var of the definition above are those of the
 * concatenation of the ranks' rows in rank order (N rows); the op is cut in two where the caller's collective goes, forward
 * and backward. Typed like the _rows entries (x / dx and y / dy each float32 or bfloat16 storage, the same alignment and
 * even-c rules); n is THIS rank's row count, n >= 1 on every rank, and may differ between ranks.
 *   forward:   mccnn_bn_sync_stats  -> [gather parts] -> mccnn_bn_sync_apply
 *   backward:  mccnn_bn_sync_bwd_sums -> [gather parts_b] -> mccnn_bn_sync_bwd_dx
 * parts, parts_b: [world, 3, c] float32 (moved as single floats: 4-byte alignment). A stats / sums stage writes this rank's
 * row -- (count, mean, M2) per column, the slab partials of the plain op merged in its fixed order, resp. (sum g,
 * sum g * xhat, sum xhat) -- and +0.0f into EVERY other row: nothing needs a memset, and an all-reduce(SUM) of the tensor is
 * an exact gather (so is an all-gather of the rows). The stage behind the collective reads all rows.
 *   apply:     every workgroup merges the rows of its columns by Chan's rule in rank order 0 .. world - 1 (once, ahead of
 *              its rows), var = M2 / N; saved = [mean; rstd] and the moving statistics take the global mean and biased
 *              variance; meta = int32[2] = (rowBase, N), rowBase = the rows of the lower ranks. The rest is the plain op's.
 *   dropout:   the mask of local row i is that of GLOBAL row rowBase + i: with one seed on all ranks the shards reproduce
 *              the mask of the unsharded batch.
 *   bwd_sums:  g, xhat, gate and mask recomputed as the plain backward does (mask at global rows; meta and saved are the
 *              forward's). dbeta = this rank's sum g, dgamma = this rank's sum g * xhat: adding them up over the ranks is
 *              the caller's gradient all-reduce.
 *   bwd_dx:    sums the rows of parts_b in rank order: dx = gamma * rstd * (g - Sg / N - (xhat - mh) * (Sgx - mh Sg) / N),
 *              mh = Sh / N the mean of xhat (the saved f32 mean's rounding error; the correction of the plain backward).
 *              dgamma != NULL: rewritten as this rank's sum g * (xhat - mh) -- the plain op's dgamma once the ranks' are
 *              added. dx == NULL: not wanted (dgamma is then required).
 * Launches: stats and bwd_sums two each, one for n <= 256; apply and bwd_dx one each. No atomics, no tickets, fixed merge
 * orders: the same inputs and seed give the same bytes, and from the same gathered parts every rank computes the same
 * bytes of saved and of the moving statistics. world == 1 is allowed (the plain op's y). ws: mccnn_bn_act_workspace_bytes(n, c)
 * for stats and bwd_sums. n, c or world < 1, rank outside [0, world), keep_threshold == 0 or > 2^32, a type flag outside
 * {0, 1}, a NULL required pointer: MCCNN_E_BADARG; n > 2^24 (counts travel as f32): MCCNN_E_TOOLARGE; a missing or short
 * workspace: MCCNN_E_WORKSPACE; the bf16 rules: MCCNN_E_SHAPE; all before anything is launched. N must stay below 2^31.
 * Not covered: a split form of mccnn_linear_bn_act_*, overlapping the collective with other work, ranks without rows,
 * statistics in anything but f32. */
int mccnn_bn_sync_stats(const void* x, int x_bf16, int n, int c, int rank, int world, float* parts /* [world,3,c] */,
                        void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_bn_sync_apply(const void* x, int x_bf16, int n, int c, int rank, int world, const float* parts /* gathered */,
                        const float* gamma, const float* beta, float* moving_mean, float* moving_var, float momentum,
                        float eps, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                        void* y, int y_bf16, float* saved /* [2,c] */, int* meta /* [2] */, mccnn_stream_t stream);
int mccnn_bn_sync_bwd_sums(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, int rank, int world,
                           const float* gamma, const float* beta, const float* saved, const int* meta, int relu,
                           unsigned long long keep_threshold, float keep_scale, unsigned seed,
                           float* parts_b /* [world,3,c] */, float* dgamma, float* dbeta,
                           void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_bn_sync_bwd_dx(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, int rank, int world,
                         const float* gamma, const float* beta, const float* parts_b /* gathered */, const float* saved,
                         const int* meta, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                         void* dx /* x's type; NULL: not wanted */, float* dgamma /* NULL: left as bwd_sums wrote it */,
                         mccnn_stream_t stream);

/* A LINEAR LAYER AND THE DENSE GLUE BEHIND IT AS ONE OP (extension, ABI 21; linear_bn.hip):
 *   z = x w + b,  y = drop(act(bn(z)))
 * x [n, cin], w [cin, cout] (as the store holds *_weights), z [n, cout] float32 row-major contiguous; b, gamma, beta and
 * the moving statistics [cout] float32; n, cin, cout >= 1 with no divisibility rule. bn, act and drop are THE DENSE GLUE AS
 * ONE OP above, applied to z (biased variance, moving statistics updated in place when training, gate pre > 0, the
 * counter-based mask of (seed, i, j)). y is float32 (y_bf16 == 0) or bfloat16 storage (1; an even cout and y on 4 bytes,
 * otherwise MCCNN_E_SHAPE), rounded to nearest even at the store; dy has y's type. z is accumulated in f32 on the f32-input
 * matrix cores -- one fmaf chain over k = 0 .. cin - 1 per element, then + b -- and row i of z does not depend on the other
 * rows of the call. x moves in 16-byte pieces when cin % 4 == 0 and x is on 16 bytes, as single floats otherwise: the
 * same bytes either way.
 *   training: writes z (the backward reads it), saved = [mean; rstd; remainder] [3, cout], the moving statistics and y. Two launches:
 *             the matmul, whose epilogue also leaves the per-slab statistics of z in ws, and the kernel that merges and
 *             applies them; one launch up to 256 rows. Inside, a mean is carried as an exact value of its column plus a
 *             remainder of the size of the std, so xhat keeps f32 precision on columns with |mean| >> std; saved holds
 *             the mean rounded to f32 once, rstd, and what the exact mean has over the rounded one -- forward and
 *             backward both normalise as ((z - mean) - remainder) * rstd, so their gates agree bit for bit.
 *   eval:     the moving statistics, no dropout, nothing updated; z and saved may be NULL, nothing is stored but y. One
 *             launch.
 *   backward: dz = bn_act's backward over z (into ws), dw = x^T dz, db = sum_i dz[i,:] (the cancelling sum it is: batch
 *             norm removes the bias), dx = dz w^T, dx == NULL: not wanted (same bytes for everything else). At most five
 *             launches, four up to 256 rows.
 * No atomics, no memset, fixed merge orders: the same inputs and seed give the same bytes. ws of
 * mccnn_linear_bn_act_workspace_bytes(n, cin, cout) bytes serves both directions (the training forward uses the front of
 * it, none up to 256 rows; eval none: ws may then be NULL). n, cin or cout < 1, keep_threshold == 0 or > 2^32, a type flag
 * outside {0, 1}, a NULL required pointer: MCCNN_E_BADARG; more than 65535 tiles of 64 rows, or cin * cout past 2^31:
 * MCCNN_E_TOOLARGE; a missing or short workspace: MCCNN_E_WORKSPACE; all before anything is launched. */
size_t mccnn_linear_bn_act_workspace_bytes(int n, int cin, int cout);
int mccnn_linear_bn_act_fwd(const float* x, const float* w, const float* b, int n, int cin, int cout, const float* gamma,
                            const float* beta, float* moving_mean, float* moving_var, float momentum, float eps,
                            int training, int relu, unsigned long long keep_threshold, float keep_scale, unsigned seed,
                            float* z /* [n,cout]; may be NULL when !training */, void* y, int y_bf16,
                            float* saved /* [3,cout]; may be NULL when !training */,
                            void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_linear_bn_act_bwd(const float* x, const float* w, const float* z, const void* dy, int dy_bf16, int n, int cin,
                            int cout, const float* gamma, const float* beta, const float* saved, int relu,
                            unsigned long long keep_threshold, float keep_scale, unsigned seed,
                            float* dx /* NULL: not wanted */, float* dw, float* db, float* dgamma, float* dbeta,
                            void* ws, size_t ws_bytes, mccnn_stream_t stream);

/* THE LAST LINEAR LAYER AND THE SOFTMAX CROSS-ENTROPY BEHIND IT AS ONE OP (extension, ABI 23; linear_xent.hip):
 *   z = x w + b,  lse_i = m_i + log(sum_j exp(z_ij - m_i)) with m_i = max_j z_ij,  l_i = lse_i - z[i, labels_i],
 *   loss = (sum over live rows of rw_i l_i) / D,  D = max(number of live rows, 1),
 *   pred_i = the lowest j attaining max_j z_ij (written for every row),  correct = the live rows with pred_i == labels_i.
 * x [n, cin], w [cin, c], b [c] float32 row-major contiguous, labels [n] int32, row_weights [n] float32 (NULL: all 1); n, cin,
 * c >= 1 with no divisibility rule. A row is LIVE iff 0 <= labels_i < c and its weight is != 0: a label outside [0, c)
 * makes the row a weight-0 row, never an error and never an out-of-range read. No live row: loss = +0.0f and all-zero
 * gradients. z is the z of A LINEAR LAYER AND THE DENSE GLUE above, byte for byte (one fmaf chain over k per element, then
 * + b; row i does not depend on the other rows of the call); the maximum is subtracted before every exp.
 *   forward:  writes loss [1], lse [n], meta = {D, correct}, pred [n] unless NULL and the logits z [n, c] unless NULL (the
 *             other outputs have the same bytes either way). One launch up to 256 rows, two above.
 *   backward: with g = loss_grad[0], a DEVICE word read by the kernel,
 *               dz_ij = g rw_i / D (exp(z_ij - lse_i) - [j == labels_i]) on live rows, 0 elsewhere
 *             recomputed from x, w, b, lse and meta (into ws), dx = dz w^T (dx == NULL: not wanted, the same bytes for
 *             the rest), dw = x^T dz, db = sum_i dz[i, :]. At most four launches; three up to 512 rows or without dx, two
 *             with both.
 * No atomics, no memset, fixed merge orders: the same inputs give the same bytes. ws of
 * mccnn_linear_xent_workspace_bytes(n, cin, c) bytes serves both directions (the forward uses the front of it, none up to
 * 256 rows: ws may then be NULL there); the query answers 0 for sizes the op refuses. n, cin or c < 1, a NULL required
 * pointer: MCCNN_E_BADARG; more than 65535 tiles of 64 rows, or cin * c past 2^31: MCCNN_E_TOOLARGE; a missing or short
 * workspace: MCCNN_E_WORKSPACE; all before anything is launched. */
size_t mccnn_linear_xent_workspace_bytes(int n, int cin, int c);
int mccnn_linear_xent_fwd(const float* x, const float* w, const float* b, int n, int cin, int c, const int* labels,
                          const float* row_weights /* NULL: all 1 */, float* loss /* [1] */, float* lse /* [n] */,
                          int* meta /* [2]: D, correct */, int* pred /* [n], NULL: not wanted */,
                          float* logits /* [n,c], NULL: not stored */, void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_linear_xent_bwd(const float* x, const float* w, const float* b, int n, int cin, int c, const int* labels,
                          const float* row_weights, const float* lse, const int* meta, const float* loss_grad /* [1], device */,
                          float* dx /* NULL: not wanted */, float* dw, float* db, void* ws, size_t ws_bytes,
                          mccnn_stream_t stream);

/* THE COSINE-DISTANCE LOSS OF NORMAL ESTIMATION AS ONE OP (extension, ABI 24; cosine_loss.hip): per row i, all in float32,
 * every sum over j ascending as one fmaf chain, eps = 1e-12f (tf.nn.l2_normalize's),
 *   sp = sum_j p_j^2,  rp = 1 / sqrt(max(sp, eps)),  u_j = p_j rp;     st, rt, v_j = t_j rt likewise from the target,
 *   cos_i = sum_j u_j v_j,  l_i = 1 - cos_i,
 *   a_i = 2 atan2f(sqrt(sum_j (u_j - v_j)^2), sqrt(sum_j (u_j + v_j)^2))   (pi / 2 when both sums are 0),
 *   loss = (sum over live rows of rw_i l_i) / D,  cosSum = sum over live rows of cos_i,  angleSum = sum over live rows of a_i,
 *   D = max(number of live rows, 1).
 * pred, target [n, c] float32 row-major contiguous, row_weights [n] float32 (NULL: all 1); n, c >= 1, n * c < 2^31, no
 * divisibility rule and no alignment rule beyond 4 bytes (rows of three floats are never 16-byte aligned). Inputs are finite and
 * their squares do not overflow. A row is LIVE iff its weight is != 0 (without weights: every row); a zero target is live and
 * has cos = 0. loss is tf.losses.cosine_distance with SUM_BY_NONZERO_WEIGHTS (without weights: the mean); the two sums are
 * unweighted metrics. The angle is NOT acos(cos_i): that form loses half the digits near +-1, this one is exact at u = +-v.
 * No live row: loss = +0.0f, zero sums, all-zero dpred.
 *   forward:  writes loss [1], sums = {cosSum, angleSum}, meta = {D}. One launch up to 256 rows, two above.
 *   backward: with g = loss_grad[0], a DEVICE word read by the kernel, and s = g rw_i / D,
 *               dpred_ij = -s rp (v_j - cos_i u_j)   on live rows with sp >= eps
 *               dpred_ij = -s 1e6f v_j               on live rows with sp <  eps (the clamp makes u linear in p)
 *               dpred_ij = 0                         on the other rows
 *             recomputed from pred, target and meta; nothing per row is kept. One launch. No gradient with respect to target
 *             or the weights.
 * No atomics, no memset, fixed merge orders: the same inputs give the same bytes. The forward's ws holds
 * mccnn_cosine_loss_workspace_bytes(n, c) bytes: 0 up to 256 rows (ws may then be NULL) and for sizes the op refuses. n or
 * c < 1, a NULL required pointer: MCCNN_E_BADARG; n * c >= 2^31: MCCNN_E_TOOLARGE; a missing or short workspace:
 * MCCNN_E_WORKSPACE; all before anything is launched. */
size_t mccnn_cosine_loss_workspace_bytes(int n, int c);
int mccnn_cosine_loss_fwd(const float* pred, const float* target, int n, int c, const float* row_weights /* NULL: all 1 */,
                          float* loss /* [1] */, float* sums /* [2]: cosSum, angleSum */, int* meta /* [1]: D */,
                          void* ws, size_t ws_bytes, mccnn_stream_t stream);
int mccnn_cosine_loss_bwd(const float* pred, const float* target, int n, int c, const float* row_weights, const int* meta,
                          const float* loss_grad /* [1], device */, float* dpred, mccnn_stream_t stream);

/* SEGMENTATION SCORES ON THE DEVICE: PER-CLOUD, PER-CLASS COUNTS (extension, ABI 25; seg_counts.hip). With B = num_clouds,
 * C = num_classes, l = labels[i], p = pred[i] and b = batch_ids[i] (0 when batch_ids is NULL), row i is LIVE iff
 *   0 <= l < C,  l != ignore_label,  its weight is not 0 (-0.0f is 0; a NaN is "not 0": the live rule of
 *   mccnn_linear_xent_fwd),  0 <= b < B.
 * A dead row changes nothing. A bad batch id makes the row dead: it is never clamped into another cloud's counts and nothing
 * is read or written out of range. For a live row
 *   counts[b, l, 2] += 1                                                    (ground truth G)
 *   p == l:  counts[b, l, 0] += 1 (intersection I),  counts[b, l, 1] += 1    (union U)
 *   p != l:  counts[b, l, 1] += 1,  and counts[b, p, 1] += 1 when 0 <= p < C
 * so a prediction outside [0, C) on a live row is a miss of l and touches nothing else. With ignore_label = 0 and B = 1 these
 * are the per-class sums of the reference's ScanNet.py:307-315, per cloud the intersection / union of ShapeNet.py:294-302.
 * counts [B, C, 3] int64 is ADDED to: the caller zeroes it once and accumulates over as many calls as it likes. pred, labels,
 * batch_ids [n] int32, row_weights [n] float32 (NULL: all 1), 4-byte aligned; where all of them are 16-byte aligned the rows
 * are read 16 bytes at a time. One launch, no workspace, no memset; integer atomics only, so the same inputs give the same
 * bytes in every run. Where B C 3 32-bit words fit mccnn_seg_counts_lds_bytes' budget (32 KB) every workgroup counts into a
 * table in LDS and adds its non-zero words to counts at its end; above it live rows add straight to counts.
 * mccnn_seg_counts_lds_bytes(B, C): the bytes of that table, 0: the route without one (and for B or C < 1).
 * n == 0 launches nothing and returns 0. B or C < 1, n < 0, a NULL pred / labels / counts: MCCNN_E_BADARG; B C 3 >= 2^31:
 * MCCNN_E_TOOLARGE; all before anything is launched. */
size_t mccnn_seg_counts_lds_bytes(int num_clouds, int num_classes);
int mccnn_seg_counts_add(const int* pred, const int* labels, const float* row_weights /* NULL: all 1 */,
                         const int* batch_ids /* NULL: every row is cloud 0 */, int n, int num_clouds, int num_classes,
                         int ignore_label /* < 0: none */, long long* counts /* [num_clouds, num_classes, 3], += */,
                         mccnn_stream_t stream);

/* VOXEL ACCURACY ON THE DEVICE: PER-VOXEL MAJORITY VOTES (extension, ABI 26; voxel_acc.hip, voxel_key.h). ScanNet's own
 * metric (ScanNet.py:321-339): the points of a cloud are binned into the voxels of a grid of `resolution` over the cloud's box
 * minimum, every occupied voxel votes for its most frequent label and its most frequent prediction, and the valid voxels are
 * counted per label, all and those whose two votes agree. With B = num_clouds, C = num_classes, l = labels[i], p = pred[i] and
 * b = batch_ids[i] (0 when batch_ids is NULL):
 *   coordinates  v_a = ceilf((pts[i, a] - aabb_min[b, a]) / resolution) per axis a, the subtraction and the division correctly
 *                rounded float32. Row i is DROPPED iff some v_a is not finite, below 0 or above 65535.
 *   dead rows    l outside [0, C), b outside [0, B) (never clamped into another cloud, nothing is read out of range), or
 *                dropped. Every other row is LIVE -- one whose label is ignore_label too: it votes and counts in the share.
 *   voxel        of a live row: the integer tuple (b, v_x, v_y, v_z), kept as it is. (The reference flattens the triple in
 *                float32 with strides nVoxels, which aliases (0, y, z) with (nVoxels_x, y - 1, z) and is inexact above 2^24;
 *                the tuple does neither.)
 *   per voxel    L[c] = its live rows with label c, P[c] = its live rows with p == c (a prediction outside [0, C) votes for
 *                nothing), s = sum L, ul = the lowest c attaining max L, up = the lowest c attaining max P (0 when P is all
 *                zero), g = L[ignore_label] (0 without one). VALID iff (double) g / (double) s < max_ignore_share in IEEE
 *                double -- the reference's expression, with 0.3 -- and ul != ignore_label.
 *   output       every valid voxel: counts[b, ul, 1] += 1 (G) and, where ul == up, counts[b, ul, 0] += 1 (V).
 * counts [B, C, 2] int64 is ADDED to: the caller zeroes it once and accumulates over as many calls as it likes. dropped:
 * optional int32 [1] device word, incremented by the number of rows with a label and a batch id in range that were dropped
 * for their coordinates; the library never reads it. pts [n, 3] float32, pred, labels, batch_ids [n] int32, aabb_min [B, 3]
 * float32: 4-byte aligned, nothing more. Integer atomics only and no float in any decision but the per-row ceilf and the
 * per-voxel quotient: the same inputs give the same bytes in every run and in any arrival order.
 * A hash table in the workspace: cap slots, a power of two, of one uint64 key (1 << 63 | b << 48 | v_x << 32 | v_y << 16 | v_z;
 * 0: empty -- an all-zero workspace is the empty table) and a uint32 [2, C] histogram each; home slot a murmur-style mix of
 * the key masked by cap - 1, linear probing. mccnn_voxel_acc_workspace_bytes(n, C) = cap_rec (8 + 8 C), cap_rec the smallest
 * power of two >= max(2 n, 64) (0 for n < 0, n >= 2^30 or C < 1). Any 16-byte aligned workspace that holds cap_min slots, the
 * smallest power of two > n, is accepted (an empty slot always exists); the largest power of two that fits, up to cap_rec, is
 * used. ws_clean = 0: the used part of the workspace is cleared first (one launch more); ws_clean = 1: the caller vouches
 * that it is all zero. Either way the call leaves what it used all zero again, so a workspace that only this entry writes
 * is cleared once. Launches: 3 with ws_clean = 0, 2 with ws_clean = 1 (vote, score), 0 for n == 0, which returns 0.
 * A NULL pts / pred / labels / aabb_min / counts / ws, n < 0, B or C < 1, a resolution that is not a finite positive number,
 * a workspace off a 16-byte boundary: MCCNN_E_BADARG; B > 32768, n >= 2^30 or B C 2 >= 2^31: MCCNN_E_TOOLARGE; a workspace
 * below cap_min (8 + 8 C) bytes: MCCNN_E_WORKSPACE; all before anything is launched. */
size_t mccnn_voxel_acc_workspace_bytes(int n, int num_classes);
int mccnn_voxel_acc_add(const float* pts, const int* pred, const int* labels, const int* batch_ids /* NULL: cloud 0 */,
                        const float* aabb_min /* [num_clouds, 3] */, int n, int num_clouds, int num_classes,
                        int ignore_label /* < 0: none */, float resolution, double max_ignore_share,
                        long long* counts /* [num_clouds, num_classes, 2], += */, int* dropped /* NULL: not counted */,
                        void* ws, size_t ws_bytes, int ws_clean, mccnn_stream_t stream);

/* THE OPTIMISER STEP AS ONE OP: ADAM WITH L2 DECAY OVER MANY TENSORS (extension, ABI 27; adam.hip). Per element, in float32,
 * with the record's step_size, bc2_sqrt, weight_decay and the call's beta1, beta2, eps, grad_scale, every operation rounded
 * once and in this order (1 - beta is the float32 difference):
 *   g   = grad_scale * grad                      (skipped when grad_scale == 1.0f)
 *   g   = weight_decay * p + g                   (skipped when weight_decay == 0.0f; L2 in the gradient, not AdamW)
 *   m'  = m + (1 - beta1) * (g - m)
 *   v'  = beta2 * v + ((1 - beta2) * g) * g
 *   den = sqrt(v') / bc2_sqrt + eps
 *   p'  = p - step_size * (m' / den)
 * p, m and v [n] float32 are updated in place, g [n] is only read. The caller computes the per-tensor scalars from the
 * tensor's own step count t >= 1, in double from the float32 betas the call passes, rounded once to float:
 *   torch.optim.Adam's arithmetic:      step_size = lr / (1 - beta1^t),                      bc2_sqrt = sqrt(1 - beta2^t)
 *   tf.train.AdamOptimizer's (epsilon outside the bias correction):
 *                                       step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t),    bc2_sqrt = 1
 * `tensors` is a HOST array of `count` records, read before the call returns; the records of up to mccnn_adam_max_tensors()
 * tensors travel by value in the arguments of one launch, so nothing is uploaded and nothing has to stay valid afterwards. A
 * record with n == 0 is skipped: its pointers and scalars are not looked at. A call issues ceil(live / max) launches, live =
 * the records with n > 0, and none for count == 0 or live == 0 (MCCNN_OK). Pointers need 4-byte alignment only; a tensor whose
 * four pointers are all 16-byte aligned is read and written 16 bytes at a time, every other one float by float, and nothing
 * outside [0, n) of any array is touched either way. No atomics, no workspace, no memset, nothing read back: the same inputs
 * give the same bytes. The library cannot check that the arrays of a call do not overlap one another (p, m, v of one tensor,
 * or any array of two tensors): the result is then unspecified.
 * count < 0, a NULL array with count > 0, a record with n < 0, a record with n > 0 and a NULL or not 4-byte aligned pointer, a
 * non-finite step_size / weight_decay / bc2_sqrt or bc2_sqrt <= 0, beta1 or beta2 outside [0, 1), eps < 0, a non-finite beta1 /
 * beta2 / eps / grad_scale: MCCNN_E_BADARG; more than 2^31 - 1 workgroups in one launch: MCCNN_E_TOOLARGE (out of reach while
 * a workgroup takes 4096 elements of a tensor of at most 2^31 - 1); all before anything is launched. */
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    int n;
    float step_size;
    float bc2_sqrt;
    float weight_decay;
} mccnn_adam_tensor;
int mccnn_adam_max_tensors(void); /* tensors one launch takes */
int mccnn_adam_step(const mccnn_adam_tensor* tensors /* HOST array */, int count, float beta1, float beta2, float eps,
                    float grad_scale, mccnn_stream_t stream);

/* ... CLIPPED BY THE GLOBAL GRADIENT NORM, AND SKIPPED WHEN THAT NORM IS NOT FINITE (extension, ABI 29; adam.hip, grad_clip.h).
 * With gs = grad_scale and the live tensors = the records with n > 0, in record order, e = 2^-23:
 *   S       = sum over live tensors and elements of (gs * grad)^2
 *   norm    = float32(sqrt(S))
 *   coef    = 1                                          if max_norm == 0, or norm is not finite
 *           = min(1.0f, max_norm / (norm + 1e-6f))       otherwise, in float32: one add, one divide, one min
 *                                                        (torch.nn.utils.clip_grad_norm_'s formula)
 *   skipped = 1 if skip_nonfinite and norm is not finite, else 0
 *   skips  += skipped
 * mccnn_grad_norm writes {norm, coef, skipped, skips} into `record`, 16 bytes of DEVICE memory on a 16-byte boundary that
 * the caller zeroes once when allocating it (skips is cumulative over the calls; a call reads nothing else of it). Nothing is
 * read back. Of a tensor record it looks at g and n only -- p, m, v and the scalars can hold anything -- so it serves as
 * the norm of any list of float32 arrays. Products and squares are float32; the sums inside a chunk of 4096 elements are
 * float32 and tree-shaped, the chunks' partials float64 and summed in index order: norm is within 7.25 e of the exact value
 * (derivation in adam.hip). A square or a chunk sum beyond FLT_MAX (|gs * grad| above about 1.8e19) is inf, and the step then
 * reads as non-finite: nothing is rescaled. `ws` is DEVICE memory on an 8-byte boundary of at least mccnn_grad_norm_ws(tensors,
 * count) bytes (8 per chunk of every live tensor; 0 for none, or for a table the call would refuse); every partial in it is
 * written before it is read, so it needs no clearing. No atomics, no memset: the same inputs give the same bytes, record
 * included. Launches: ceil(live / mccnn_adam_max_tensors()) + 1, none with no live tensor (MCCNN_OK; the record stays).
 * count < 0, a NULL table with count > 0, n < 0, a NULL or not 4-byte aligned g with n > 0, a non-finite grad_scale, a
 * negative or non-finite max_norm, a NULL record or one off a 16-byte boundary, a ws off an 8-byte boundary: MCCNN_E_BADARG;
 * a ws that is NULL or too small with live tensors: MCCNN_E_WORKSPACE; 2^31 chunks or more: MCCNN_E_TOOLARGE; all before
 * anything is launched.
 * mccnn_adam_step_clipped is mccnn_adam_step (its checks, its launches) with a record: every workgroup reads the 16 bytes
 * once; with skipped == 1 the whole grid returns before its first access to p, m, v; otherwise the element definition runs with
 * grad_scale' = float32(grad_scale * coef), rounded once, in place of grad_scale (coef == 1.0f changes no bit). A NULL record
 * or one off a 16-byte boundary: MCCNN_E_BADARG. The step counts behind step_size and bc2_sqrt are the caller's: a caller
 * that reads nothing back counts a skipped step too. */
typedef struct { float norm; float coef; int skipped; int skips; } mccnn_grad_record;   /* 16 bytes, DEVICE memory */
size_t mccnn_grad_norm_ws(const mccnn_adam_tensor* tensors /* HOST array */, int count);   /* bytes of partials */
int mccnn_grad_norm(const mccnn_adam_tensor* tensors /* HOST array */, int count, float grad_scale,
                    float max_norm /* 0: no clipping */, int skip_nonfinite, mccnn_grad_record* record, void* ws, size_t ws_bytes,
                    mccnn_stream_t stream);
int mccnn_adam_step_clipped(const mccnn_adam_tensor* tensors /* HOST array */, int count, float beta1, float beta2, float eps,
                            float grad_scale, const mccnn_grad_record* record, mccnn_stream_t stream);

/* TEST HOOK, not part of the operator surface: selects the convolution implementation for A/B
 * parity tests (bit 0: VALU fallback kernels, bit 1: general MFMA kernels for one-input-feature
 * layers; bit 2: one-input-feature backward passes never take the cooperative edge kernel, bit 3:
 * they take it whenever the block count is even, whatever the list length; 0 = product default).
 * With bit 4 set the call writes bits 0-1 only and leaves bits 2-3 as they are. Returns the previous mask. Initial value: MCCNN_DEBUG keys force_valu / no_f1 / f1_coop_off /
 * f1_coop_force in the environment, read once. */
int mccnn_debug_conv_impl(int mask);

/* Diagnostics: number of kernel launches the library has issued in this process (all streams). bench.py prints the
 * difference over one step: below ~50k points a step is bound by launches, not by the kernels. */
long long mccnn_debug_launch_count(void);
/* Diagnostics: nanoseconds the host has spent so far inside the library WAITING for an edge total (mccnn_geometry_edges /
 * the first mccnn_conv_* call over a geometry). bench.py subtracts it from a step's host time: what is left is the
 * host's own work per step. */
long long mccnn_debug_wait_ns(void);
/* ... of the CALLING thread only when it says so: a helper thread that waits in the caller's place switches its own
 * accounting off (returns the previous setting; thread-local, default on). */
int mccnn_debug_wait_accounting(int on);
/* The calling THREAD's launches are background work from now on (on != 0) / no longer (on == 0): they run on a queue of
 * their own beside kernels a step waits for (ConvolutionBuilder.prefetch_geometry: the geometry of the next batch under
 * the convolutions of the current one). Kernels that would fill every wave slot hold back in that mode; results do not
 * change. Returns the previous setting. */
int mccnn_background_launches(int on);
/* TEST HOOK: combin layers with one input feature run their forward edge pass with four consecutive edges per lane
 * (one segmented scan per 256 edges) on lists of at least `edges` edges (default 2 000 000; shorter lists keep 64-edge
 * chunks: more waves to spread over the chip). 0 = always, INT_MAX = never. Same results up to float summation order.
 * Returns the previous threshold. */
int mccnn_debug_f1_x4_min_edges(int edges);
/* TEST HOOK: small problems (coarse hierarchy levels: a few thousand points / edges) run single-workgroup forms of
 * the grid build, the list transposition ... that replace 4 - 8 launches by one; on = 0 sends them through the
 * multi-launch kernels of the large problems instead (same results). Returns the previous setting. Initial value: on,
 * unless MCCNN_SMALL_OFF is set in the environment. */
int mccnn_debug_small_kernels(int on);

#ifdef __cplusplus
}
#endif
#endif /* MCCNN_H_ */
