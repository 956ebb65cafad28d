// The dropout mask of the fused dense glue (mccnn_bn_act_fwd / _bwd, bn_act.hip): which elements of an [n, c] tensor a
// call with a given seed keeps. Plain integer C++ over neigh_sample.h's hash, so that the host compiles the very
// predicate the kernels run (tools/bn_drop_check.cpp).
//
// Element (i, j) is kept iff (uint64) h < T,  h = mix(row_hash(seed, i) + (uint32) j),  T = floor(keepProb * 2^32).
// T = 2^32 keeps everything ("no dropout"); T = 0 would keep nothing and is rejected by the C-ABI. No generator state, no
// stored mask: the backward pass recomputes the bit from (seed, i, j).
#pragma once
#include <cstdint>
#include "neigh_sample.h"

namespace mccnn {

constexpr uint64_t kBnDropAll = 0x100000000ull;   // T of "keep every element"

// the per-row half of the hash, shared by the elements of row i
MCCNN_SAMPLE_FN uint32_t bn_drop_row(uint32_t seed, int i) { return sample_row_hash(seed, i); }

// row = bn_drop_row(seed, i)
MCCNN_SAMPLE_FN bool bn_drop_keep(uint32_t row, uint32_t j, uint64_t T) { return (uint64_t)sample_mix(row + j) < T; }

// T of a keep probability in (0, 1]: floor(keepProb * 2^32), in double (exact: a double times a power of two)
inline uint64_t bn_drop_threshold(double keepProb) { return (uint64_t)(keepProb * 4294967296.0); }

}  // namespace mccnn
