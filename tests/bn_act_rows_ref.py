"""Cases and bars of the fused dense glue on bf16 rows (mccnn_bn_act_fwd_rows / _bwd_rows), over tests/bn_act_ref.py:
bfloat16 in NumPy (round to nearest even, exact widening), make_case(n, c) with x and dy rounded to bf16 for the bf16
operands, and the float64 reference evaluated on those rounded values.
"""
import numpy as np

import bn_act_ref as ref

# why each is here: one row, one wide unit / one pair / pair form, c % 8 != 0 / wide form / first slab form, a full
# 64-column tile / pair form, several tiles, the last partly filled / many tiles, few rows / odd row count, pair form /
# more than 64 slabs of 128 rows: the slabs grow / large n
SHAPES = [(1, 8), (2, 2), (63, 6), (65, 16), (257, 64), (1000, 130), (3, 1024), (4099, 34), (8321, 8), (20000, 16)]
EXACT_SHAPES = [(65, 16), (63, 6), (257, 64), (1000, 130), (8321, 8)]
COMBOS = [(False, False), (False, True), (True, False), (True, True)]     # (x is bf16, y / dy is bf16)
COMBO_IDS = ["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"]


def to_bf16_bits(a):
    """float32 -> the uint16 bit patterns of bfloat16, round to nearest even (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def from_bf16_bits(b):
    """uint16 bit patterns of bfloat16 -> float32, exact."""
    return (np.asarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_bf16(a):
    """float32 values rounded to the nearest bfloat16 (ties to even), as float32."""
    return from_bf16_bits(to_bf16_bits(a))


_CASES = {}


def case(n, c, x_bf16, y_bf16):
    """ref.make_case(n, c) with x rounded to bf16 when x is a bf16 operand and dy when y / dy is; shared, read-only."""
    key = (n, c, bool(x_bf16), bool(y_bf16))
    if key not in _CASES:
        d = dict(ref.case(n, c))
        if x_bf16:
            d["x"] = round_bf16(d["x"])
        if y_bf16:
            d["dy"] = round_bf16(d["dy"])
        for v in d.values():
            v.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


_FWD = {}


def reference(shape, x_bf16, relu, keepProb, seed):
    """float64 training forward of a case -> (dict of ref.forward, mask, scale); computed once, shared, read-only. (The
    forward does not depend on dy, so neither does the key.)"""
    key = (shape, bool(x_bf16), relu, keepProb, seed)
    if key not in _FWD:
        n, c = shape
        d = case(n, c, x_bf16, False)
        mask = None if keepProb is None else ref.keep_mask(seed, n, c, ref.threshold(keepProb))
        scale = 1.0 if keepProb is None else 1.0 / keepProb
        _FWD[key] = (ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, relu, mask, scale), mask, scale)
    return _FWD[key]


def assert_bf16_close(v, r, what="bf16 output"):
    """A bf16 result v (widened) against its float64 reference r: |v - r| <= 2^-8 |r| + 1e-4 max|r| -- the unit roundoff of
    an 8-bit significand, and what is rounded is within the f32 bar of r."""
    v, r = np.asarray(v, np.float64), np.asarray(r, np.float64)
    assert v.shape == r.shape, (what, v.shape, r.shape)
    assert np.isfinite(v).all(), what
    excess = np.abs(v - r) - (2.0 ** -8 * np.abs(r) + 1e-4 * np.abs(r).max())
    assert excess.max() <= 0.0, "%s: %.3e over the bf16 bar at %s" % (what, excess.max(), np.unravel_index(excess.argmax(), r.shape))
