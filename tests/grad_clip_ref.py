"""A float64 NumPy model of the norm pass in front of the optimiser step (mccnn_grad_norm, FusedAdam(maxGradNorm, skipNonFinite)),
written from the definition in include/mccnn.h, with the bar of the tests.

    S       = sum over live tensors and elements of (gs * grad)^2,   gs = float32(grad_scale)
    norm    = float32(sqrt(S))
    coef    = 1 if max_norm == 0 or norm is not finite, else min(1.0f, max_norm / (norm + 1e-6f))      (float32)
    skipped = 1 if skip_nonfinite and norm is not finite, else 0

The bar on the norm, e = 2^-23: |norm - ref| <= 16 e ref against the float64 norm. The op's own worst case is 7.25 e (27
float32 roundings of non-negative terms on any path through a 4096-element chunk, halved by the square root, and the
rounding of the result; csrc/adam.hip derives it), so a kernel that misses the bar is wrong.
"""
import math

import numpy as np

E = 2.0 ** -23
BAR = 16 * E
RECORD = np.dtype([("norm", "<f4"), ("coef", "<f4"), ("skipped", "<i4"), ("skips", "<i4")])   # mccnn_grad_record
assert RECORD.itemsize == 16


def f32(x):
    return float(np.float32(x))


def norm64(grads, grad_scale=1.0):
    """The float64 norm of float32(grad_scale) * grads, grads any list of arrays."""
    gs = float(np.float32(grad_scale))
    with np.errstate(over="ignore", invalid="ignore"):
        return math.sqrt(sum(float(np.sum((gs * np.asarray(g, dtype=np.float64).reshape(-1)) ** 2)) for g in grads))


def coef32(norm, max_norm):
    """The coefficient of a float32 norm, in float32 operations -> np.float32."""
    norm, max_norm = np.float32(norm), np.float32(max_norm)
    if max_norm == 0 or not np.isfinite(norm):
        return np.float32(1.0)
    with np.errstate(over="ignore"):
        q = np.float32(max_norm / np.float32(norm + np.float32(1e-6)))
    return q if q < 1 else np.float32(1.0)


def share(norm, ref):
    """The share of the bar that a float32 norm uses against the float64 one; <= 1 passes. ref == 0 takes an exact 0."""
    if ref == 0:
        return 0.0 if float(norm) == 0.0 else math.inf
    return abs(float(norm) - ref) / (BAR * ref)
