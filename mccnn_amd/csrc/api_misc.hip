// Version / diagnostics entry points of libmccnn_hip.
#include "common.h"
#include <cstdlib>

namespace mccnn {
std::atomic<long long> g_launches{0};
thread_local int g_background = 0;
std::atomic<int> g_small_off{debug_int("small_off", 0) ? 1 : 0};
std::atomic<int> g_f1_x4_min_edges{debug_int("f1_x4_min_e", 2000000)};

// The head of a call chain whose first kernel itself needs zeros (histogram counters of a grid build, ...): ONE launch
// for everything the chain wants cleared up front; every later need is met by a kernel of the chain (clear_span_dev).
__global__ __launch_bounds__(256) void clear_spans(ClearSpan a, ClearSpan b, ClearSpan c) {
    clear_span_dev(a);
    clear_span_dev(b);
    clear_span_dev(c);
}
// caller-owned buffers of any 4-byte-aligned size (a zero-filled scatter target, a one-word counter): 4-byte granular
__global__ __launch_bounds__(256) void zero_words(unsigned* __restrict__ p, unsigned long long words) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < words; k += stride) p[k] = 0u;
}
__global__ __launch_bounds__(256) void fill_words(unsigned* __restrict__ p, unsigned long long words, unsigned v) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < words; k += stride) p[k] = v;
}
int launch_fill_words(void* p, size_t words, unsigned v, hipStream_t s) {
    if (words == 0) return 0;
    long long blocks = (long long)((words + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    fill_words<<<(int)blocks, 256, 0, s>>>(reinterpret_cast<unsigned*>(p), (unsigned long long)words, v);
    MCCNN_LAUNCHED();
    return 0;
}
int launch_zero_words(void* p, size_t words, hipStream_t s) {
    if (words == 0) return 0;
    if ((((uintptr_t)p) & 15) == 0 && (words & 3) == 0) return launch_clear_spans(clear_span(p, words * 4), no_span(), no_span(), s);
    long long blocks = (long long)((words + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    zero_words<<<(int)blocks, 256, 0, s>>>(reinterpret_cast<unsigned*>(p), (unsigned long long)words);
    MCCNN_LAUNCHED();
    return 0;
}
// ... of a whole batch of geometries (mccnn_geometry_build_batch): every span in one launch
__global__ __launch_bounds__(256) void clear_spans_batch(SpanBatch sb) {
    for (int k = 0; k < sb.count; ++k) clear_span_dev(sb.sp[k]);
}
int launch_clear_batch(const SpanBatch& sb, hipStream_t s) {
    unsigned long long most = 0;
    for (int k = 0; k < sb.count; ++k) most = sb.sp[k].n16 > most ? sb.sp[k].n16 : most;
    if (most == 0) return 0;
    long long blocks = (long long)((most + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    clear_spans_batch<<<(int)blocks, 256, 0, s>>>(sb);
    MCCNN_LAUNCHED();
    return 0;
}
int launch_clear_spans(ClearSpan a, ClearSpan b, ClearSpan c, hipStream_t s) {
    const unsigned long long most = a.n16 > b.n16 ? (a.n16 > c.n16 ? a.n16 : c.n16) : (b.n16 > c.n16 ? b.n16 : c.n16);
    if (most == 0) return 0;
    long long blocks = (long long)((most + 255) / 256);
    if (blocks > 4096) blocks = 4096;   // 16 B per thread and trip: 16 MB per sweep of the grid
    clear_spans<<<(int)blocks, 256, 0, s>>>(a, b, c);
    MCCNN_LAUNCHED();
    return 0;
}
}

extern "C" {

int mccnn_block_size(void) { return MCCNN_MLP; }
int mccnn_abi_version(void) { return 31; }  // 2: optional forward state of spatial_conv; 3: bf16 rows, device-side counts; 4: compute_pdf_dn; 5: row plans, aabb_extent; 6: rowplan_build, build_grid; 7: feat_index of the row kernels, hierarchy_level, find_neighbors_count2; 8: background_launches, debug_f1_x4_min_edges; 9: native step executor (mccnn_geometry_*, mccnn_conv_*); 10: mccnn_geometry_build_batch, mccnn_geometry_prebuild_batch; 11: gradients with respect to positions (mccnn_spatial_conv_bwd_points, mccnn_compute_pdf_bwd_points, mccnn_edge_grad_reduce); 12: per-point KDE (mccnn_compute_pdf_points, mccnn_expand_pdf); 13: per-point densities in the native step executor (mccnn_geometry_build_point, mccnn_geometry_build_batch_point); 14: position gradients of the per-point KDE (mccnn_compute_pdf_points_bwd, mccnn_expand_pdf_bwd); 15: training batches built on the device (mccnn_batch_sample); 16: an edge budget for the neighbour search (mccnn_find_neighbors_count_budget / _fill_budget); 17: the edge budget in the native step executor (mccnn_geometry_build_budget, mccnn_geometry_build_batch_budget, mccnn_geometry_cap); 18: the dense glue as one op (mccnn_bn_act_fwd, mccnn_bn_act_bwd, mccnn_bn_act_workspace_bytes); 19: per-edge records from the KDE of a geometry (mccnn_geometry_want_records, mccnn_geometry_records_bytes, mccnn_geometry_records, mccnn_conv_uses_records; flags bit 2 of mccnn_conv_*); 20: the dense glue on bf16 rows (mccnn_bn_act_fwd_rows, mccnn_bn_act_bwd_rows); 21: a linear layer and the dense glue behind it as one op (mccnn_linear_bn_act_fwd, mccnn_linear_bn_act_bwd, mccnn_linear_bn_act_workspace_bytes); 22: the dense glue with batch statistics across ranks (mccnn_bn_sync_stats, mccnn_bn_sync_apply, mccnn_bn_sync_bwd_sums, mccnn_bn_sync_bwd_dx); 23: the last linear layer + softmax cross-entropy as one op (mccnn_linear_xent_fwd, mccnn_linear_xent_bwd, mccnn_linear_xent_workspace_bytes); 24: the cosine-distance loss of normal estimation as one op (mccnn_cosine_loss_fwd, mccnn_cosine_loss_bwd, mccnn_cosine_loss_workspace_bytes); 25: per-cloud, per-class segmentation counts on the device (mccnn_seg_counts_add, mccnn_seg_counts_lds_bytes); 26: voxel accuracy on the device, per-voxel majority votes in a hash table (mccnn_voxel_acc_add, mccnn_voxel_acc_workspace_bytes); 27: the optimiser step as one op, Adam with L2 decay over many tensors (mccnn_adam_step, mccnn_adam_max_tensors); 28: the dense glue over a column-wise concatenation of up to 8 f32 segments (mccnn_bn_act_cat_fwd, mccnn_bn_act_cat_bwd, mccnn_bn_act_cat_max_segments); 29: the optimiser step clipped by the global gradient norm and skipped when it is not finite (mccnn_grad_norm, mccnn_grad_norm_ws, mccnn_adam_step_clipped); 30: the dense glue over a concatenation with a type per segment, f32 or bf16 (mccnn_bn_act_cat_fwd_rows, mccnn_bn_act_cat_bwd_rows); 31: the rows / streaming rule as a query (mccnn_conv_rows_shape, mccnn_conv_unsorted_max_points), names for the flag and piece bits of mccnn_conv_* / mccnn_geometry_attach
const char* mccnn_arch(void) { return "gfx950"; }
int mccnn_background_launches(int on) { const int prev = mccnn::g_background; mccnn::g_background = on ? 1 : 0; return prev; }
int mccnn_debug_f1_x4_min_edges(int edges) { return mccnn::g_f1_x4_min_edges.exchange(edges < 0 ? 0 : edges); }
int mccnn_debug_small_kernels(int on) { return mccnn::g_small_off.exchange(on ? 0 : 1) == 0 ? 1 : 0; }
long long mccnn_debug_launch_count(void) { return mccnn::g_launches.load(std::memory_order_relaxed); }

const char* mccnn_error_string(int code) {
    switch (code) {
        case MCCNN_OK: return "ok";
        case MCCNN_E_BADARG: return "invalid argument (null pointer or non-positive size/attribute)";
        case MCCNN_E_BATCHID: return "batch id outside [0, batch_size)";
        case MCCNN_E_TOOLARGE: return "problem does not fit 32-bit indexing (B*nc^3, E or LDS tile)";
        case MCCNN_E_WORKSPACE: return "workspace missing or smaller than the *_workspace_bytes query";
        case MCCNN_E_SHAPE: return "kernel-MLP shape rule violated (spatial_conv.cc:258-300)";
        case MCCNN_E_CAPACITY: return "neighbour list longer than the capacity the geometry was built with";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown mccnn error";
}

}  // extern "C"
