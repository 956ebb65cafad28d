// Run-time switches of the library and of the torch extension.
//
// FOUR environment variables select a code path and are part of the interface (README, "Switches"):
//     MCCNN_NATIVE=0        layers go op by op through the Python op surface instead of the native step executor
//     MCCNN_TORCH_EXT=0     the ctypes binding of the C-ABI instead of lib/_mccnn_torch.so
//     MCCNN_ROW_KERNELS=0   depth-wise layers on the edge-streaming kernels instead of the row-per-lane ones
//     MCCNN_GEO_PREFETCH=0  no learned prefetch of the next layers' geometry
// Everything else -- A/B switches of single kernels, tracing, fault injection for the soak tests -- is ONE list:
//     MCCNN_DEBUG="key=value,key,..."      (a bare key means key=1; read once per process)
// THE table of keys is kDebugKeys below (library keys first, then the Python side's: mccnn_amd/_env.py carries the same
// table and tests/test_capi_cpu.py checks that the two are equal, that every key any source file queries is in it and
// that every key in it is queried). A key of MCCNN_DEBUG that is in neither is reported ONCE on stderr -- a misspelt
// switch must not silently time the default on both sides of an A/B. Library keys (default):
//     small_off (0)                  1 = tiny grids / lists take the kernels of the large inputs (mccnn_debug_small_kernels)
//     plan_small (4096)              capacity of the single-workgroup plan layout, clamped to [1024, MCCNN_PLAN_SMALL]
//     plan_small_max_l (16)          longest piece of a plan in the single-workgroup layout
//     plan_mid_l (16)                shortest piece of a plan of a mid-size list (< 16384 rows)
//     plan_min_l (4)                 shortest piece of a plan of a small list
//     rows_force (0)                 1 = depth-wise layers take the row kernels wherever they apply
//     rows_min_degree (16)           mean row length from which the backward pass of a large list takes the row kernels
//     unsorted_max_points (32768)    levels up to this size: the row kernels read the unsorted feature rows in place
//     force_valu (0)                 1 = spatial_conv on the VALU kernels (seeds mccnn_debug_conv_impl)
//     no_f1 (0)                      1 = one-input-feature combin layers on the general kernels (seeds mccnn_debug_conv_impl)
//     f1_x4_min_e (2000000)          edges from which a one-input-feature forward pass takes four edges per lane
//     f1_x4_waves_per_cu (0)         waves per CU of that pass (0 = as many as fit)
//     nw_lean (-1)                   1 / 0 = the lean / bounds-checked search loop (-1: lean except for background launches)
//     nw_lds_pad (-1)                LDS bytes a neighbour search asks for (-1 = 24000 for background launches, else 0)
//     scan_bg_tiles (8)              tiles from which a background scan takes the two-launch form (0 = never)
//     issue_thread (1)               0 = the torch extension issues side-stream builds on the calling thread
//     job_delay_us (0)               fault injection: a random pause of up to this many us before every helper-thread job
//     hier_trace (0)                 1 = a stderr line per prefetched hierarchy job
//     geo_own_pool (1)               0 = prefetched geometries take their memory from the caller's stream
//     trace_terminate (0)            1 = a backtrace on std::terminate
//     aabb_one_max (8192)            compute_aabb in one launch up to this many points
//     plan_batch_sync (0)            1 = a synchronisation and a stderr line per launch of the plan batch
//     caller_join_off (0)            fault injection: a geometry nobody joined does not order the caller's stream
//     bwd_min_chunks (2)             64-edge chunks per wave of the edge-streaming backward passes at least
//     f1_coop_min_chunks (3)         chunks per workgroup (whole chip in use) from which a one-input-feature backward pass takes the cooperative edge kernel
//     f1_coop_off (0)                1 = never the cooperative edge kernel (seeds mccnn_debug_conv_impl, bit 2)
//     f1_coop_force (0)              1 = the cooperative edge kernel whenever the block count is even (seeds mccnn_debug_conv_impl, bit 3)
//     kde_records (1)                0 = the KDE of a geometry writes no per-edge records (the layers evaluate their own); shared with the Python side
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace mccnn {

#define MCCNN_DEBUG_KEYS                                                                                                   \
    "small_off", "plan_small", "plan_small_max_l", "plan_mid_l", "plan_min_l", "rows_force",                              \
    "rows_min_degree", "unsorted_max_points", "force_valu", "no_f1", "f1_x4_min_e", "f1_x4_waves_per_cu", "nw_lean",      \
    "nw_lds_pad", "scan_bg_tiles", "issue_thread", "job_delay_us",                                                       \
    "hier_trace", "geo_own_pool", "trace_terminate", "aabb_one_max", "plan_batch_sync", "caller_join_off", "bwd_min_chunks", \
    "f1_coop_min_chunks", "f1_coop_off", "f1_coop_force", "kde_records",                                                 \
    /* Python side (mccnn_amd/_env.py) */                                                                                \
    "fuse_sort", "native_prefetch", "plan_prefetch", "plan_prefetch_max_e", "geo_prefetch_min",                          \
    "ecap_scale", "hier_pmode", "geo_trace"
static const char* const kDebugKeys[] = {MCCNN_DEBUG_KEYS};

// Parses MCCNN_DEBUG once; items whose key is not in kDebugKeys are reported on stderr (once per process and library).
inline const std::string& debug_list() {
    static const std::string list = [] {
        const char* e = getenv("MCCNN_DEBUG");
        std::string l(e ? e : "");
        size_t p = 0;
        while (p < l.size()) {
            size_t q = l.find(',', p);
            if (q == std::string::npos) q = l.size();
            size_t a = p, b = q;
            while (a < b && l[a] == ' ') ++a;
            while (b > a && l[b - 1] == ' ') --b;
            size_t eq = l.find('=', a);
            if (eq == std::string::npos || eq > b) eq = b;
            size_t kb = eq;
            while (kb > a && l[kb - 1] == ' ') --kb;
            const std::string key = l.substr(a, kb - a);
            if (!key.empty()) {
                bool known = false;
                for (const char* k : kDebugKeys) known = known || key == k;
                if (!known) fprintf(stderr, "mccnn: MCCNN_DEBUG key '%s' is not known (csrc/debug_opts.h kDebugKeys): ignored\n", key.c_str());
            }
            p = q + 1;
        }
        return l;
    }();
    return list;
}

// value of `key` in MCCNN_DEBUG ("" for a bare key), or nullptr
inline const char* debug_opt(const char* key) {
    const std::string& list = debug_list();
    static thread_local std::string val;
    const size_t kl = strlen(key);
    size_t p = 0;
    while (p < list.size()) {
        size_t q = list.find(',', p);
        if (q == std::string::npos) q = list.size();
        const size_t next = q + 1;
        while (p < q && list[p] == ' ') ++p;                 // (blanks around an item are ignored, as on the Python side)
        while (q > p && list[q - 1] == ' ') --q;
        if (q - p >= kl && list.compare(p, kl, key) == 0 && (q - p == kl || list[p + kl] == '=')) {
            val = (q - p == kl) ? std::string("1") : list.substr(p + kl + 1, q - p - kl - 1);
            return val.c_str();
        }
        p = next;
    }
    return nullptr;
}
inline int debug_int(const char* key, int dflt) { const char* v = debug_opt(key); return v ? atoi(v) : dflt; }
inline double debug_float(const char* key, double dflt) { const char* v = debug_opt(key); return v ? atof(v) : dflt; }

}  // namespace mccnn
