// Clipping by the global gradient norm (mccnn_grad_norm): the scalar half that turns the norm into the record's coefficient
// and skip flag. Plain C++ with no other header of the library behind it, so that the host compiles the very routine the
// finish kernel runs (tools/grad_clip_check.cpp).
//
//     coef    = 1                                     if max_norm == 0 (no clipping), or norm is not finite
//             = min(1.0f, max_norm / (norm + 1e-6f))  otherwise: one float32 add, one divide, one min
//                                                     (torch.nn.utils.clip_grad_norm_'s formula)
//     skipped = 1 if skip_nonfinite and norm is not finite, else 0
//
// A norm below max_norm - 1e-6 gives a quotient above 1 and so exactly 1.0f: multiplying by it changes no bit. "Finite" is
// read from the exponent bits, the same test under any compiler flags. The library and the check program are both compiled
// without contraction and with a correctly rounded divide, so the two sides agree to the bit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MCCNN_CLIP_FN __host__ __device__ __forceinline__
#else
#define MCCNN_CLIP_FN inline
#endif

namespace mccnn {

MCCNN_CLIP_FN bool clip_finite(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

MCCNN_CLIP_FN float clip_coef(float norm, float max_norm) {
    if (max_norm == 0.0f || !clip_finite(norm)) return 1.0f;
    const float q = max_norm / (norm + 1e-6f);
    return q < 1.0f ? q : 1.0f;
}

MCCNN_CLIP_FN int clip_skipped(float norm, int skip_nonfinite) { return (skip_nonfinite != 0 && !clip_finite(norm)) ? 1 : 0; }

}  // namespace mccnn
