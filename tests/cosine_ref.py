"""A float64 NumPy model of the cosine-distance loss of normal estimation (include/mccnn.h, "THE COSINE-DISTANCE LOSS OF NORMAL
ESTIMATION AS ONE OP"), and the cases its tests share. It takes the float32 inputs, does all arithmetic in float64 and applies
the eps clamps and the live rule as the definition states them:

    sp = sum_j p_j^2   rp = 1 / sqrt(max(sp, eps))   u = p rp        st, rt, v likewise from the target      eps = 1e-12
    cos_i = sum_j u_j v_j     l_i = 1 - cos_i     a_i = 2 atan2(|u - v|, |u + v|)   (pi / 2 when both lengths are 0)
    live: weight != 0 (no weights: every row)     D = max(live rows, 1)
    loss = sum_live rw_i l_i / D     cosSum = sum_live cos_i     angleSum = sum_live a_i
    dpred_j = -s rp (v_j - cos_i u_j)  (sp >= eps),   -s 1e6 v_j  (sp < eps),   0 on dead rows,      s = g rw_i / D
"""
import numpy as np

EPS = np.float64(np.float32(1e-12))   # the op's constant is the float32 nearest to 1e-12
CLAMP_SLOPE = np.float64(np.float32(1e6))

#: (n, c) of the GPU tests: one row; the wave boundary; one launch against two; many slabs and a ragged tail; widths around
#: the register forms (1 .. 4) and two read in place (5, 17)
SHAPES = [(1, 3), (63, 3), (64, 3), (65, 3), (256, 3), (257, 3), (4099, 3), (300, 1), (300, 2), (300, 4), (300, 5), (300, 17)]


def _unit_rows(rng, n, c):
    v = rng.standard_normal((n, c))
    v[np.abs(v).sum(1) == 0] = 1.0
    return v / np.sqrt((v * v).sum(1, keepdims=True))


def case(n, c, seed=0):
    """-> dict(pred, target, rw (float32), clamped (bool [n]: the rows with sp < eps)). Rows by index mod 8: 0, 4, 5 generic
    (random directions, norms spread over 1e-3 .. 1e3), 1 exactly parallel (p = 2 t), 2 exactly opposite (p = -2 t), 3
    orthogonal (c >= 2; generic when c = 1), 6 a zero target / a zero prediction / a prediction of norm 1e-8 in turn, 7
    generic with weight 0. No row has sp or st within a factor 100 of eps: norms are 0, 1e-8 or >= 1e-4 (1e-3 for the
    generic rows), so the float32 and float64 evaluations take the same side of the clamp. Weights: zeros on rows 7 mod 8,
    non-unit values elsewhere."""
    rng = np.random.default_rng(1000 * n + 10 * c + seed)
    norm = lambda: 10.0 ** rng.uniform(-3, 3, (n, 1))   # noqa: E731
    p = _unit_rows(rng, n, c) * norm()
    t = _unit_rows(rng, n, c) * norm()
    k = np.arange(n)
    par, opp, orth, odd = k % 8 == 1, k % 8 == 2, k % 8 == 3, k % 8 == 6
    p, t = p.astype(np.float32), t.astype(np.float32)
    p[par] = np.float32(2) * t[par]
    p[opp] = np.float32(-2) * t[opp]
    if c >= 2:   # orthogonal: (a, b, 0 ...) against (-b, a, 0 ...), exactly
        rows = np.nonzero(orth)[0]
        a, b = t[rows, 0].copy(), t[rows, 1].copy()
        t[rows] = 0
        p[rows] = 0
        t[rows, 0], t[rows, 1] = a, b
        p[rows, 0], p[rows, 1] = -b * np.float32(2), a * np.float32(2)
    rows = np.nonzero(odd)[0]
    for m, r in enumerate(rows):
        if m % 3 == 0:
            t[r] = 0
        elif m % 3 == 1:
            p[r] = 0
        else:
            p[r] = (_unit_rows(rng, 1, c)[0] * 1e-8).astype(np.float32)
    rw = rng.uniform(0.25, 4.0, n).astype(np.float32)
    rw[k % 8 == 7] = 0
    sp = (p.astype(np.float64) ** 2).sum(1)
    st = (t.astype(np.float64) ** 2).sum(1)
    for s in (sp, st):   # nothing within a factor 100 of the clamp
        assert not ((s > EPS / 100) & (s < EPS * 100)).any()
    return dict(pred=p, target=t, rw=rw, clamped=sp < EPS)


def parallel_case(n, c, seed=0):
    """Exactly parallel rows only: pred = 2 target, norms 1e-3 .. 1e3."""
    rng = np.random.default_rng(77 + n + seed)
    t = (_unit_rows(rng, n, c) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    return dict(pred=np.float32(2) * t, target=t)


def _rows(pred, target):
    p, t = np.asarray(pred, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    sp, st = (p * p).sum(1), (t * t).sum(1)
    rp, rt = 1.0 / np.sqrt(np.maximum(sp, EPS)), 1.0 / np.sqrt(np.maximum(st, EPS))
    u, v = p * rp[:, None], t * rt[:, None]
    return sp, rp, u, v, (u * v).sum(1)


def live_rows(n, rw=None):
    return np.ones(n, bool) if rw is None else np.asarray(rw, np.float32) != 0


def forward(pred, target, rw=None):
    """-> dict(loss, cosSum, angleSum, D, live, cos [n], angle [n], and the sums of the absolute terms of the three sums:
    lossAbs (already divided by D), cosAbs, angleAbs)."""
    sp, rp, u, v, cos = _rows(pred, target)
    n = len(cos)
    live = live_rows(n, rw)
    w = np.ones(n) if rw is None else np.asarray(rw, np.float32).astype(np.float64)
    far, near = np.sqrt(((u - v) ** 2).sum(1)), np.sqrt(((u + v) ** 2).sum(1))
    ang = np.where((far == 0) & (near == 0), np.pi / 2, 2.0 * np.arctan2(far, near))
    D = max(int(live.sum()), 1)
    terms = np.where(live, w * (1.0 - cos), 0.0)
    return dict(loss=terms.sum() / D, cosSum=np.where(live, cos, 0.0).sum(), angleSum=np.where(live, ang, 0.0).sum(), D=D,
                live=live, cos=cos, angle=ang, lossAbs=np.abs(terms).sum() / D, cosAbs=np.abs(np.where(live, cos, 0.0)).sum(),
                angleAbs=np.where(live, ang, 0.0).sum())


def backward(pred, target, rw=None, g=1.0):
    """dpred [n, c] (float64) for the upstream gradient g of loss."""
    sp, rp, u, v, cos = _rows(pred, target)
    n = len(cos)
    live = live_rows(n, rw)
    w = np.ones(n) if rw is None else np.asarray(rw, np.float32).astype(np.float64)
    D = max(int(live.sum()), 1)
    s = (g * w / D)[:, None]
    d = np.where((sp >= EPS)[:, None], -s * rp[:, None] * (v - cos[:, None] * u), -s * CLAMP_SLOPE * v)
    return np.where(live[:, None], d, 0.0)


def backward_terms(pred, target, rw=None, g=1.0):
    """The sum of the absolute values of the two terms every element of dpred is the difference of, |s| rp (|v_j| + |cos_i u_j|)
    (clamped rows: the one term |s| 1e6 |v_j|), 0 on dead rows. With c = 1 an unclamped row has u = +-1 and v - cos u = 0
    identically: its exact gradient is 0 and this is the only scale a float32 result can be held to."""
    sp, rp, u, v, cos = _rows(pred, target)
    n = len(cos)
    live = live_rows(n, rw)
    w = np.ones(n) if rw is None else np.asarray(rw, np.float32).astype(np.float64)
    s = np.abs(g * w / max(int(live.sum()), 1))[:, None]
    d = np.where((sp >= EPS)[:, None], s * rp[:, None] * (np.abs(v) + np.abs(cos[:, None] * u)), s * CLAMP_SLOPE * np.abs(v))
    return np.where(live[:, None], d, 0.0)


def grad_scale(want, terms, rows, c):
    """The scale the gradient of a set of rows is held to: the largest |entry| of the reference over the set -- and with c = 1,
    where the exact gradient of every unclamped row is 0, the largest sum of absolute terms (backward_terms) instead."""
    return float(np.abs(terms[rows]).max()) if c == 1 else float(np.abs(want[rows]).max())
