"""Cases of the dense glue over a concatenation of typed segments (mccnn_bn_act_cat_fwd_rows / _bwd_rows,
dense_glue.bn_relu_dropout_cat on float32 and bfloat16 segments).

A case is a column split of bn_act_ref.case(n, C) with a type per segment; the columns of the bf16 segments are rounded to
bf16 first, so the float64 reference of the whole [n, C] array sees the values the op sees. The yardstick of the bytes is the
existing float32 entry on the widened segments: the rule under which the two take the same number of columns per thread is
restated here (same_plan), next to the library's own columns-per-thread rule (rows_vec), which tools/bn_cat_rows_check.cpp
holds against csrc/bn_cat.h."""
import collections

import numpy as np

import bn_act_ref as ref
import bn_act_rows_ref as rows
import bn_cat_ref as cat

F, B = 0, 1     # a segment's type flag: float32, bfloat16

#: n, the widths, the type flags, and (segment index, ELEMENTS its view starts behind an aligned allocation) pairs
Case = collections.namedtuple("Case", "n widths types off")

CASES = [
    Case(2, (1,), (B,), ()),                                  # S = 1, 16-bit accesses
    Case(63, (1, 1, 1), (B, F, B), ()),                       # one launch, every column its own type
    Case(65, (8, 8), (B, F), ()),                             # one launch, 4 per thread, type boundary inside a tile and a wave
    Case(257, (4, 8, 4), (F, B, F), ()),                      # two launches
    Case(257, (4,) * 8, (B, F) * 4, ()),                      # the maximum S, alternating
    Case(300, (32, 4, 28), (B, B, B), ()),                    # all bf16, two tiles; outDtype=None gives a bf16 y
    Case(1000, (3, 5, 122), (B, F, B), ()),                   # 1 per thread, bf16 rows off a 4-byte boundary
    Case(4099, (16, 16, 1), (B, B, F), ()),                   # C % 4 != 0, slabs
    Case(20000, (8, 8), (F, B), ()),                          # grown slabs
    Case(257, (8, 8), (B, B), ((1, 2),)),                     # 1 per thread by the 8-byte rule: 4 bytes into its buffer
]


def case_id(c):
    return "%d-%s%s" % (c.n, "+".join("%d%s" % (w, "fb"[t]) for w, t in zip(c.widths, c.types)), "-off" if c.off else "")


IDS = [case_id(c) for c in CASES]


def width(c):
    return sum(c.widths)


def offset(c, k):
    """The elements segment k of case c starts behind an aligned allocation."""
    return dict(c.off).get(k, 0)


def pointer_ok(flag, byte_offset):
    """A segment's rows (x_s, or a wanted dx_s) allow 4 columns per thread: f32 on 16 bytes, bf16 on 8."""
    return byte_offset % (8 if flag else 16) == 0


def rows_vec(widths, types, byte_offsets, dx_byte_offsets=None):
    """Columns per thread of the typed op as far as the segments decide: 4 iff every width is a multiple of 4 and every x_s
    and wanted dx_s (dx_byte_offsets: None, or per segment its offset, None where not wanted) passes pointer_ok; else 1."""
    if any(w % 4 for w in widths):
        return 1
    if not all(pointer_ok(t, o) for t, o in zip(types, byte_offsets)):
        return 1
    if dx_byte_offsets is not None and not all(o is None or pointer_ok(t, o) for t, o in zip(types, dx_byte_offsets)):
        return 1
    return 4


def byte_offsets(c):
    """Per segment, what its pointer has over a 16-byte boundary in the tests: off[k] elements of its type."""
    return [offset(c, k) * (2 if t else 4) for k, t in enumerate(c.types)]


def same_plan(c):
    """The typed op on the case's segments and the float32 entry on their widened copies (fresh, aligned allocations) take
    the same number of columns per thread: some c_s % 4 != 0, or every c_s % 4 == 0 and every pointer aligned."""
    return rows_vec(c.widths, c.types, byte_offsets(c)) == cat.cat_vec(c.widths, True)


def out_dtype_is_bf16(types, out=None):
    """outDtype=None: bf16 iff every segment is bf16 (torch.cat's result type); out: 0 / 1 where it is given."""
    return bool(all(types)) if out is None else bool(out)


_DATA = {}


def data(c, dy_bf16=False):
    """bn_act_ref.case(n, C) with the columns of the bf16 segments (and dy when it is a bf16 operand) rounded to bf16; shared,
    read-only."""
    key = (c.n, c.widths, c.types, bool(dy_bf16))
    if key not in _DATA:
        d = dict(ref.case(c.n, width(c)))
        x = np.array(d["x"])
        at = 0
        for w, t in zip(c.widths, c.types):
            if t:
                x[:, at:at + w] = rows.round_bf16(x[:, at:at + w])
            at += w
        d["x"] = x
        if dy_bf16:
            d["dy"] = rows.round_bf16(d["dy"])
        for v in d.values():
            v.setflags(write=False)
        _DATA[key] = d
    return _DATA[key]
