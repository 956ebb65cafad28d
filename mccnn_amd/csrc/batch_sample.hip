// The device batcher's kernel (mccnn_batch_sample): one training batch out of a store of models, one workgroup per slot.
// A slot's record (mccnn_batch_slot, include/mccnn.h) names its model, its sampling protocol, the view direction, the
// rotation and a seed; the workgroup walks the model in chunks of its own size, compacts the accepted points with a
// ballot / mbcnt rank per wave and a 16-entry table per workgroup, and writes rotated points, batch ids and source rows
// straight to out_base + have. `have` is carried from chunk to chunk and from pass to pass. Every protocol is evaluated in
// f32 in a fixed operand order (no FMA contraction, correctly rounded divide and sqrt: common.h), so that a NumPy float32
// restatement makes the same decisions (tests/device_batcher_ref.py). A translation unit of its own: the other kernels keep
// their code. No atomics on floats, no generator state: the same (store, slots) give the same bytes.
#include "common.h"
#include "batch_sample.h"

namespace mccnn {

constexpr int kBatchThreads = MCCNN_BATCH_CHUNK;
constexpr int kBatchWaves = kBatchThreads / 64;
constexpr int kSlotsPerLaunch = 32;        // 32 x 108 bytes by value: inside the 4 KB of kernel arguments
constexpr int kScreen = 128;               // the z-buffer of the occlusion protocol: 128 x 128 words = 64 KiB of LDS

struct BatchSlots { mccnn_batch_slot s[kSlotsPerLaunch]; };

// rank of a flagged thread among the flagged threads of the workgroup (thread order), and their number
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
    const unsigned long long bm = __ballot(flag);
    const int wave = threadIdx.x >> 6;
    const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0));
    if (lane_id() == 0) wsum[wave] = __popcll(bm);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kBatchWaves; ++k) {
        const int c = wsum[k];
        base += k < wave ? c : 0;
        tot += c;
    }
    __syncthreads();   // wsum is written again by the next chunk
    total = tot;
    return base + r;
}

// row `row` of the batch = point i of the slot's model, rotated: x * r00 + y * r10 + z * r20, left to right
__device__ __forceinline__ void emit_row(const mccnn_batch_slot& s, const float* __restrict__ pts, int i, long long row,
                                         float* __restrict__ op, int* __restrict__ ob, int* __restrict__ os) {
    const float* p = pts + ((size_t)s.offset + (size_t)i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    float* o = op + (size_t)row * 3;
    o[0] = x * s.rot[0] + y * s.rot[3] + z * s.rot[6];
    o[1] = x * s.rot[1] + y * s.rot[4] + z * s.rot[7];
    o[2] = x * s.rot[2] + y * s.rot[5] + z * s.rot[8];
    ob[row] = s.batch_id;
    os[row] = s.offset + i;
}

// order-preserving map of an f32 onto uint32 (any sign), for the integer minimum of the z-buffer
__device__ __forceinline__ unsigned depth_key(float z) {
    const unsigned b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_depth(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the orthographic camera of sample_occlusion, in f32
struct OccCamera {
    float xx, xy, xz, yx, yy, yz, vx, vy, vz, sx, sy, sz, pixel, depth;
};
__device__ __forceinline__ OccCamera occ_camera(const mccnn_batch_slot& s) {
    OccCamera c;
    c.vx = s.view[0]; c.vy = s.view[1]; c.vz = s.view[2];
    // x = view x (0, 1, 0), normalised; y = x x view, normalised
    const float ax = -c.vz, az = c.vx;
    const float xl = sqrtf(ax * ax + az * az);
    c.xx = ax / xl; c.xy = 0.f; c.xz = az / xl;
    const float bx = -(c.xz * c.vy), by = c.xz * c.vx - c.xx * c.vz, bz = c.xx * c.vy;
    const float yl = sqrtf(bx * bx + by * by + bz * bz);
    c.yx = bx / yl; c.yy = by / yl; c.yz = bz / yl;
    const float dx = s.bmax[0] - s.bmin[0], dy = s.bmax[1] - s.bmin[1], dz = s.bmax[2] - s.bmin[2];
    const float diag = sqrtf(dx * dx + dy * dy + dz * dz) * 0.5f;
    const float cx = (s.bmax[0] + s.bmin[0]) * 0.5f, cy = (s.bmax[1] + s.bmin[1]) * 0.5f, cz = (s.bmax[2] + s.bmin[2]) * 0.5f;
    c.pixel = diag / (float)(kScreen / 2);
    c.depth = diag * 2.0f;
    c.sx = cx - c.vx * diag - c.xx * diag - c.yx * diag;
    c.sy = cy - c.vy * diag - c.xy * diag - c.yy * diag;
    c.sz = cz - c.vz * diag - c.xz * diag - c.yz * diag;
    return c;
}
__device__ __forceinline__ int occ_pixel_coord(float t, float pixel) {
    float q = floorf(t / pixel);
    q = q >= -1073741824.0f ? q : -1073741824.0f;   // (NaN goes to the lower bound)
    q = q <= 1073741824.0f ? q : 1073741824.0f;
    return (int)q & (kScreen - 1);                  // the host's wrap of pixel indices
}
// -> facing; pix, z of point i of the slot's model
__device__ __forceinline__ bool occ_project(const OccCamera& c, const mccnn_batch_slot& s, const float* __restrict__ pts,
                                            const float* __restrict__ normals, int i, int& pix, float& z) {
    const size_t r = ((size_t)s.offset + (size_t)i) * 3;
    const float nx = normals[r], ny = normals[r + 1], nz = normals[r + 2];
    const float t0 = pts[r] - c.sx, t1 = pts[r + 1] - c.sy, t2 = pts[r + 2] - c.sz;
    const float tx = t0 * c.xx + t1 * c.xy + t2 * c.xz;
    const float ty = t0 * c.yx + t1 * c.yy + t2 * c.yz;
    z = (t0 * c.vx + t1 * c.vy + t2 * c.vz) / c.depth;
    pix = occ_pixel_coord(tx, c.pixel) * kScreen + occ_pixel_coord(ty, c.pixel);
    return (nx * c.vx + ny * c.vy + nz * c.vz) < 0.f;
}

__global__ __launch_bounds__(kBatchThreads) void batch_sample_k(BatchSlots a, int first, const float* __restrict__ pts,
                                                                const float* __restrict__ normals, int store_rows,
                                                                float* __restrict__ op, int* __restrict__ ob,
                                                                int* __restrict__ os, int* __restrict__ counts,
                                                                int* __restrict__ status) {
    __shared__ unsigned zbuf[kScreen * kScreen];
    __shared__ int wsum[kBatchWaves];
    const mccnn_batch_slot& s = a.s[blockIdx.x];
    const int tid = threadIdx.x;
    const int n = s.length, R = s.rows;
    const long long base = s.out_base;
    int have = 0;

    if (s.protocol == 0) {
        // uniform: a stratified draw of R rows over the first n_sel points (with replacement when there are fewer)
        const int ns = s.n_sel;
        if (ns > 0) {
            const uint32_t h = batch_pass_hash(s.seed, 0);
            for (int t = tid; t < R; t += kBatchThreads)
                emit_row(s, pts, (int)batch_uniform_index((uint32_t)t, (uint32_t)ns, (uint32_t)R, h), base + t, op, ob, os);
            have = R;
        }
    } else if (s.protocol == 4) {
        // occlusion: per-pixel minimum depth of the facing points, then every facing point within 0.01 of it, cycled
        const OccCamera c = occ_camera(s);
        for (int k = tid; k < kScreen * kScreen; k += kBatchThreads) zbuf[k] = 0xFFFFFFFFu;
        __syncthreads();
        for (int b0 = 0; b0 < n; b0 += kBatchThreads) {
            const int i = b0 + tid;
            if (i < n) {
                int pix;
                float z;
                if (occ_project(c, s, pts, normals, i, pix, z)) atomicMin(&zbuf[pix], depth_key(z));
            }
        }
        __syncthreads();
        for (int b0 = 0; b0 < n; b0 += kBatchThreads) {
            const int i = b0 + tid;
            bool keep = false;
            if (i < n) {
                int pix;
                float z;
                const bool facing = occ_project(c, s, pts, normals, i, pix, z);
                keep = facing && (z - key_depth(zbuf[pix])) < 0.01f;
            }
            int total;
            const int rank = block_rank(keep, wsum, total);
            if (keep && have + rank < R) emit_row(s, pts, i, base + have + rank, op, ob, os);
            have = min(R, have + total);
            if (have >= R) break;
        }
        if (s.exact && have > 0 && have < R) {
            // the host's _cycle: row r repeats row r mod (kept points); the rows written above are this workgroup's own
            __syncthreads();
            const int kept = have;
            for (int r = kept + tid; r < R; r += kBatchThreads) {
                const size_t q = (size_t)(base + r % kept), d = (size_t)(base + r);
                op[d * 3] = op[q * 3];
                op[d * 3 + 1] = op[q * 3 + 1];
                op[d * 3 + 2] = op[q * 3 + 2];
                ob[d] = s.batch_id;
                os[d] = os[q];
            }
            have = R;
        }
    } else {
        // split, gradient, lambert: accept point i of pass t when its draw is below its probability
        const float s0 = s.bmax[0] - s.bmin[0], s1 = s.bmax[1] - s.bmin[1], s2 = s.bmax[2] - s.bmin[2];
        int ax = 0;
        float size = s0;
        if (s1 > size) { ax = 1; size = s1; }
        if (s2 > size) { ax = 2; size = s2; }
        const float lo = s.bmin[ax];
        const float gsub = size * 0.2f, gdiv = size * 0.6f;
        const float vx = s.view[0], vy = s.view[1], vz = s.view[2];
        const int passes = s.exact ? MCCNN_BATCH_MAX_PASSES : 1;
        for (int pass = 0; pass < passes; ++pass) {
            const uint32_t h = batch_pass_hash(s.seed, pass);
            for (int b0 = 0; b0 < n; b0 += kBatchThreads) {
                const int i = b0 + tid;
                bool acc = false;
                if (i < n) {
                    const size_t r = ((size_t)s.offset + (size_t)i) * 3;
                    float prob;
                    if (s.protocol == 1) {
                        const float pos = (pts[r + ax] - lo) / size;
                        prob = pos > 0.5f ? 1.0f : 0.25f;
                    } else if (s.protocol == 2) {
                        const float p = (pts[r + ax] - lo - gsub) / gdiv;
                        float cl = p > 0.01f ? p : 0.01f;
                        cl = cl < 1.0f ? cl : 1.0f;
                        prob = sqrtf(cl);
                    } else {
                        const float d = normals[r] * vx + normals[r + 1] * vy + normals[r + 2] * vz;
                        float cl = d > 0.0f ? d : 0.0f;
                        cl = cl < 1.0f ? cl : 1.0f;
                        prob = sqrtf(cl);
                    }
                    const float u = (float)batch_draw24(h, (uint32_t)i) * 5.9604644775390625e-8f;   // 2^-24
                    acc = u < prob;
                }
                int total;
                const int rank = block_rank(acc, wsum, total);
                if (acc && have + rank < R) emit_row(s, pts, i, base + have + rank, op, ob, os);
                have = min(R, have + total);
                if (have >= R) break;
            }
            if (have >= R || have == 0) break;   // done, or a first pass that accepted nothing
        }
    }

    int st = MCCNN_BATCH_OK;
    if (s.exact && have < R) {
        // gave up: no output byte stays undefined
        st = have == 0 ? MCCNN_BATCH_NO_POINT : MCCNN_BATCH_PASS_BOUND;
        for (int r = have + tid; r < R; r += kBatchThreads) {
            if (n > 0) {
                emit_row(s, pts, 0, base + r, op, ob, os);
            } else {
                const size_t d = (size_t)(base + r);
                op[d * 3] = op[d * 3 + 1] = op[d * 3 + 2] = 0.f;
                ob[d] = s.batch_id;
                os[d] = min(s.offset, store_rows - 1);
            }
        }
    }
    if (tid == 0) {
        counts[first + blockIdx.x] = have;
        status[first + blockIdx.x] = st;
    }
}

}  // namespace mccnn

using namespace mccnn;

extern "C" {

int mccnn_batch_sample_chunk(void) { return MCCNN_BATCH_CHUNK; }
int mccnn_batch_max_passes(void) { return MCCNN_BATCH_MAX_PASSES; }

int mccnn_batch_sample(const float* store_pts, const float* store_normals, int store_rows, const mccnn_batch_slot* slots_host,
                       int num_slots, int out_rows, float* out_pts, int* out_batch_ids, int* out_src, int* counts,
                       int* status, mccnn_stream_t stream) {
    if (num_slots < 0 || out_rows < 0 || store_rows <= 0) return MCCNN_E_BADARG;
    if (num_slots == 0) return 0;
    if (!store_pts || !slots_host || !counts || !status) return MCCNN_E_BADARG;
    if (out_rows > 0 && (!out_pts || !out_batch_ids || !out_src)) return MCCNN_E_BADARG;
    // every row a workgroup can write lies in [out_base, out_base + rows): checked here, once, on the host
    for (int k = 0; k < num_slots; ++k) {
        const mccnn_batch_slot& s = slots_host[k];
        if (s.offset < 0 || s.length < 0 || (long long)s.offset + s.length > store_rows) return MCCNN_E_BADARG;
        if (s.protocol < 0 || s.protocol > 4 || s.rows < 0 || s.out_base < 0) return MCCNN_E_BADARG;
        if ((long long)s.out_base + s.rows > out_rows) return MCCNN_E_BADARG;
        if (s.n_sel < 0 || s.n_sel > s.length) return MCCNN_E_BADARG;
        if (s.protocol >= 3 && !store_normals) return MCCNN_E_BADARG;
        // one pass of a variable-count slot accepts at most `length` points
        if (!s.exact && s.protocol != 0 && s.rows < s.length) return MCCNN_E_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int first = 0; first < num_slots; first += kSlotsPerLaunch) {
        const int cnt = num_slots - first < kSlotsPerLaunch ? num_slots - first : kSlotsPerLaunch;
        BatchSlots a;
        for (int k = 0; k < kSlotsPerLaunch; ++k) a.s[k] = slots_host[first + (k < cnt ? k : 0)];
        batch_sample_k<<<cnt, kBatchThreads, 0, st>>>(a, first, store_pts, store_normals, store_rows, out_pts, out_batch_ids,
                                                      out_src, counts, status);
        MCCNN_LAUNCHED();
    }
    return 0;
}

}  // extern "C"
