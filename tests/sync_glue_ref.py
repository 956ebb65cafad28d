"""NumPy model of the dense glue with batch statistics across ranks (mccnn_bn_sync_*, MCConvModule.bn_relu_dropout_sync):
the op cut in two where the collective goes, in the kernels' f32 arithmetic.

Per rank: the (count, mean, M2) partial of its rows as the kernels compute it (bn_act_ref's restatement: shifted sums per
row lane, Chan's merge in the LDS tree, slab partials). Behind the gather: Chan's merge of the ranks' partials in rank
order, var = M2 / N, the plain op's apply with the dropout mask at GLOBAL rows. Backward: per-rank f32 sums
(sum g, sum g * xhat, sum xhat), added in rank order, dx with the plain backward's shift correction. The float64
whole-batch reference, the cases and the mask are bn_act_ref's.
"""
import numpy as np

import bn_act_ref as ref
from bn_act_ref import backward, case, forward, keep_mask, threshold  # noqa: F401  (the float64 reference, re-exported)

# shape -> rows per rank: ragged, one-row ranks, ranks on both sides of the 256-row threshold between the kernel forms
SPLITS = {(1000, 130): [1, 255, 257, 487], (257, 64): [256, 1], (4099, 33): [3000, 1099], (63, 3): [1, 62]}
SHAPES = list(SPLITS)
f32 = np.float32


def bounds(shape):
    """[(row0, row1)] of the ranks of a shape's split."""
    out, r0 = [], 0
    for k in SPLITS[shape]:
        out.append((r0, r0 + k))
        r0 += k
    assert r0 == shape[0]
    return out


def rank_partial(x):
    """(count, mean, M2) of the columns of a rank's rows, f32, as mccnn_bn_sync_stats leaves them in the rank's row."""
    x = np.asarray(x, f32)
    n, c = x.shape
    R, sr = ref.row_lanes(c), ref.slab_rows(n)
    zero = np.zeros(c, f32)
    slabs = []
    for row0 in range(0, n, sr):
        row1 = min(n, row0 + sr)
        K = x[row0]
        lanes = []
        for ry in range(R):
            rows = x[row0 + ry:row1:R]
            d = rows - K
            s1, s2 = zero.copy(), zero.copy()
            for v in d:
                s1 = s1 + v
                s2 = s2 + v * v
            cnt = f32(len(rows))
            q = s1 / cnt if len(rows) else zero
            lanes.append((cnt, K + q if len(rows) else K.copy(), np.maximum(s2 - s1 * q, f32(0))))
        slabs.append(ref._tree(lanes))
    if len(slabs) == 1:
        return slabs[0]
    lanes = []
    for ry in range(R):
        acc = (f32(0), zero.copy(), zero.copy())
        for s in range(ry, len(slabs), R):
            acc = ref._chan(*acc, *slabs[s])
        lanes.append(acc)
    return ref._tree(lanes)


def merge_ranks(parts):
    """Chan's merge of the ranks' partials in rank order -> (N as int, mean, var = M2 / N), f32."""
    acc = (f32(0), None, None)
    total = 0
    for cnt, mean, m2 in parts:
        total += int(cnt)
        acc = (cnt, mean, m2) if acc[0] == 0 else ref._chan(*acc, cnt, mean, m2)
    return total, acc[1], acc[2] / f32(total)


def model_forward(shape, relu, keepProb, seed, eps=1e-3, momentum=0.99):
    """The split forward of a case in f32 -> dict(y [concatenated], mean, rstd, mov_mean, mov_var, gates, bases, N)."""
    d = case(*shape)
    n, c = shape
    bs = bounds(shape)
    total, mean, var = merge_ranks([rank_partial(d["x"][a:b]) for a, b in bs])
    rstd = f32(1) / np.sqrt(var + f32(eps))
    keep = f32(1) - f32(momentum)
    mm = d["mov_mean"] * f32(momentum) + mean * keep
    mv = d["mov_var"] * f32(momentum) + var * keep
    T = threshold(keepProb)
    scale = f32(1) if keepProb is None else f32(1) / f32(keepProb)
    ys, gates, bases = [], [], []
    for a, b in bs:
        pre = (d["x"][a:b] - mean) * rstd * d["gamma"] + d["beta"]
        act = np.where(pre > 0, pre, f32(0)) if relu else pre
        if keepProb is not None:
            rows = np.arange(a, b)[:, None]                     # the mask of GLOBAL row rowBase + i
            act = np.where(ref.keep_bits(seed, rows, np.arange(c)[None, :], T), act * scale, f32(0))
        ys.append(act.astype(f32))
        gates.append(pre > 0)
        bases.append(a)
    return dict(y=np.concatenate(ys), mean=mean, rstd=rstd, mov_mean=mm, mov_var=mv, gates=np.concatenate(gates), bases=bases,
                N=total)


def model_backward(shape, fwd, relu, keepProb, seed):
    """The split backward in f32 from model_forward's result -> (dx [concatenated], [dgamma per rank], [dbeta per rank])."""
    d = case(*shape)
    n, c = shape
    bs = bounds(shape)
    mean, rstd = fwd["mean"], fwd["rstd"]
    T = threshold(keepProb)
    scale = f32(1) if keepProb is None else f32(1) / f32(keepProb)
    per = []
    for a, b in bs:
        xh = (d["x"][a:b] - mean) * rstd
        g = d["dy"][a:b].astype(f32)
        if keepProb is not None:
            g = np.where(ref.keep_bits(seed, np.arange(a, b)[:, None], np.arange(c)[None, :], T), g * scale, f32(0))
        if relu:
            g = np.where(fwd["gates"][a:b], g, f32(0))
        per.append((g, xh, g.sum(0, dtype=f32), (g * xh).sum(0, dtype=f32), xh.sum(0, dtype=f32)))
    zero = np.zeros(c, f32)
    sg, sx, sh = zero.copy(), zero.copy(), zero.copy()
    for _, _, a_, b_, c_ in per:                                # the gathered partials, in rank order
        sg, sx, sh = sg + a_, sx + b_, sh + c_
    fn = f32(fwd["N"])
    mh = sh / fn
    dg = sx - mh * sg
    dxs, dgs, dbs = [], [], []
    for g, xh, og, ox, _ in per:
        dxs.append((d["gamma"] * rstd) * (g - sg / fn - (xh - mh) * (dg / fn)))
        dgs.append(ox - mh * og)
        dbs.append(og)
    return np.concatenate(dxs).astype(f32), dgs, dbs
