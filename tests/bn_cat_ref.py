"""Cases of the dense glue over a concatenation (mccnn_bn_act_cat_fwd / _bwd, dense_glue.bn_relu_dropout_cat).

A case is a column split of bn_act_ref.make_case(n, C): batch norm is per column, so the float64 reference of the op over
the segments is bn_act_ref.forward / backward on the whole [n, C] array, and dx_s is the column slice of dx. Each case
says whether the library takes the SAME plan for the segments as for the contiguous op on torch.cat(xs, 1) -- then every
output is byte for byte that op's -- by the rule restated here (plans_coincide)."""
import collections

import numpy as np

import bn_act_ref as ref

MAX_SEGMENTS = 8

#: n, the widths, and the segments (by index) that sit 4 bytes off a 16-byte boundary
Case = collections.namedtuple("Case", "n widths off")

CASES = [
    Case(2, (1,), ()),                              # S = 1, vec = 1
    Case(63, (1, 1, 1), ()),                        # one-launch form, every column its own segment
    Case(65, (8, 8), ()),                           # one-launch form, vec = 4, boundary inside a tile
    Case(257, (4, 8, 4), ()),                       # two-launch form, three segments in one tile
    Case(257, (4, 4, 4, 4, 4, 4, 4, 4), ()),        # the maximum S
    Case(300, (32, 4, 28), ()),                     # one boundary on a tile edge, one inside (C = 64, two tiles at vec = 4)
    Case(1000, (3, 5, 122), ()),                    # vec = 1, odd widths, several tiles
    Case(4099, (16, 16, 1), ()),                    # C % 4 != 0 with aligned multiple-of-4 segments, slabs
    Case(20000, (8, 8), ()),                        # grown slabs (n > 64 * 128)
    Case(257, (6, 10), ()),                         # C % 4 == 0 but segments not: plans differ, float bar only
    Case(257, (8, 8), (1,)),                        # vec = 1 by alignment
]


def case_id(c):
    return "%d-%s%s" % (c.n, "+".join(str(w) for w in c.widths), "-off" if c.off else "")


IDS = [case_id(c) for c in CASES]


def width(c):
    return sum(c.widths)


def cat_vec(widths, aligned=True):
    """Columns per thread of the op over segments: 4 iff every width is a multiple of 4 and every pointer is aligned."""
    return 4 if aligned and all(w % 4 == 0 for w in widths) else 1


def plain_vec(c, aligned=True):
    """... of the contiguous op at width c (the rule bn_act_ref.row_lanes restates for aligned rows)."""
    return 4 if aligned and c % 4 == 0 else 1


def row_lanes(vec, c):
    """Row lanes of a workgroup at `vec` columns per thread and width c: 256 / (threads across a tile)."""
    units, most, tw = c // vec, ref.TILE_COLS // vec, 1
    while tw < most and tw < units:
        tw *= 2
    return ref.THREADS // tw


def plans_coincide(c):
    """The segments of case c take the plan of the contiguous op on their (aligned) concatenation."""
    return cat_vec(c.widths, not c.off) == plain_vec(width(c))


def split(a, widths):
    """The column blocks of a [n, C] array, each C-contiguous."""
    out, at = [], 0
    for w in widths:
        out.append(np.ascontiguousarray(a[:, at:at + w]))
        at += w
    return out


def data(c):
    """bn_act_ref.case(n, C): shared, read-only."""
    return ref.case(c.n, width(c))
