// What linear_bn.hip shares with bn_act.hip: the slab rule of the batch statistics and the backward with a two-part mean.
#pragma once
#include "common.h"

namespace mccnn {

// rows of a slab of the batch statistics of an n-row tensor (n itself up to 256 rows); slabs = ceil(n / rows)
int bn_slab_rows(int n);

// mccnn_bn_act_bwd_rows with one more argument. shift: NULL, or [c] -- what the exact mean of a column has over saved's
// f32 one; xhat is then ((x - mean) - shift) * rstd.
int bn_act_bwd_impl(const void* x, int x_bf16, const void* dy, int dy_bf16, int n, int c, const float* gamma, const float* beta,
                    const float* saved, const float* shift, int relu, unsigned long long keep_threshold, float keep_scale,
                    unsigned seed, void* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, mccnn_stream_t stream);

}  // namespace mccnn
