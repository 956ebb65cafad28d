// Voxel accuracy on the device (mccnn_voxel_acc_add): the scalar half -- the voxel coordinate of a point with its drop rule,
// the 64-bit key of a voxel, the hash that picks its home slot and the two table capacities. Plain C++ with no other header of
// the library behind it, so that the host compiles the very routines the kernels run (tools/voxel_key_check.cpp).
//
//   coordinate  v = ceilf((p - min) / res) per axis: one float32 subtraction and one float32 division, each correctly rounded
//               (the library is built without FMA contraction and with correctly rounded f32 division). The row is DROPPED
//               iff v is not finite, below 0 or above 65535; -0.0f (a point a fraction of a voxel below the minimum) is 0.
//   key         1 << 63 | b << 48 | v_x << 32 | v_y << 16 | v_z with b < 2^15: never 0, so 0 marks an empty slot and an all-zero
//               workspace is the empty table. The tuple (b, v_x, v_y, v_z) is kept as it is: no flattening, no aliasing.
//   hash        the 64-bit finaliser of MurmurHash3 (public domain); the home slot is hash & (cap - 1).
//   capacities  cap_rec = the smallest power of two >= max(2 n, 64) (load <= 0.5), cap_min = the smallest power of two > n
//               (an empty slot always exists: every probe chain ends).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MCCNN_VOXEL_FN __host__ __device__ __forceinline__
#else
#define MCCNN_VOXEL_FN inline
#endif

namespace mccnn {

#define MCCNN_VOXEL_MAX_COORD 65535     // 16 bits per axis
#define MCCNN_VOXEL_MAX_CLOUDS 32768    // 15 bits of cloud under the occupied bit

// -> false: the row is dropped; true: v holds the coordinate
MCCNN_VOXEL_FN bool voxel_coord(float p, float mn, float res, uint32_t& v) {
    const float q = ceilf((p - mn) / res);
    if (!(q >= 0.0f && q <= (float)MCCNN_VOXEL_MAX_COORD)) return false;   // (a NaN fails both comparisons)
    v = (uint32_t)q;                                                       // (-0.0f -> 0)
    return true;
}

MCCNN_VOXEL_FN uint64_t voxel_key(uint32_t b, uint32_t vx, uint32_t vy, uint32_t vz) {
    return (1ull << 63) | ((uint64_t)b << 48) | ((uint64_t)vx << 32) | ((uint64_t)vy << 16) | (uint64_t)vz;
}
MCCNN_VOXEL_FN uint32_t voxel_key_cloud(uint64_t key) { return (uint32_t)(key >> 48) & 0x7fffu; }

MCCNN_VOXEL_FN uint64_t voxel_hash(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// n < 2^30: both are at most 2^31
MCCNN_VOXEL_FN uint64_t voxel_cap_rec(uint64_t n) {
    uint64_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}
MCCNN_VOXEL_FN uint64_t voxel_cap_min(uint64_t n) {
    uint64_t cap = 1;
    while (cap <= n) cap <<= 1;
    return cap;
}
// bytes of one slot: the key and a uint32 [2, C] histogram (labels, predictions)
MCCNN_VOXEL_FN uint64_t voxel_slot_bytes(uint64_t C) { return 8 + 8 * C; }

// per occupied voxel, from its two histograms: the lowest class attaining the maximum (0 for an all-zero row), the rows s and
// the rows g of the ignore label -> valid iff (double) g / (double) s < share in IEEE double and ul != ignore
MCCNN_VOXEL_FN bool voxel_valid(uint32_t g, uint32_t s, int ul, int ignore, double share) {
    return s > 0 && (double)g / (double)s < share && ul != ignore;
}

}  // namespace mccnn
