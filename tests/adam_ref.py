"""A float64 NumPy model of the optimiser step (mccnn_adam_step, FusedAdam), written from the definition in include/mccnn.h,
with the per-element tolerances of the tests and their inputs.

    g   = grad_scale * grad
    g   = weight_decay * p + g
    m'  = m + (1 - beta1) * (g - m)
    v'  = beta2 * v + ((1 - beta2) * g) * g
    den = sqrt(v') / bc2_sqrt + eps
    p'  = p - step_size * (m' / den)

Tolerances, from the reference's own quantities, e = 2^-23:

    G     = |grad_scale * grad| + weight_decay * |p|
    tol_m = 4 e (|m| + G)
    tol_v = 8 e v'
    tol_p = 4 e (|p'| + |u|) + step_size * tol_m / den,     u = step_size * m' / den

A float32 evaluation of the definition, with or without fused multiply-adds, uses at most 0.24 of tol_p, 0.13 of tol_m and
0.34 of tol_v on the inputs below (five steps of 300 000 elements, both forms, weight_decay in {0, 1e-2}, grad_scale in
{1, 0.25}), so a kernel that misses a bar is wrong.

Inputs: p standard normal, every 13th element scaled by 1e-4; |grad| log-uniform in [1e-6, 1e2] with a random sign, every 97th
exactly 0. On tensors WITH decay the gradient takes the sign of p: otherwise weight_decay * p + grad can cancel to nothing, and
v' = ... g^2 then has no relative accuracy in ANY float32 implementation. That is the conditioning of the sum, not a property
of the kernel, and tol_v is relative to v'.
"""
import math

import numpy as np

E = 2.0 ** -23
FORMS = ("torch", "tf")


def f32(x):
    return float(np.float32(x))


def scalars(form, lr, beta1, beta2, t, round32=True):
    """(step_size, bc2_sqrt) of step t >= 1 in double; round32: rounded once to float32 (what the kernel is handed)."""
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    if form == "torch":
        ss, bs = lr / bc1, math.sqrt(bc2)
    else:
        assert form == "tf"
        ss, bs = lr * math.sqrt(bc2) / bc1, 1.0
    return (f32(ss), f32(bs)) if round32 else (ss, bs)


def step(p, grad, m, v, step_size, bc2_sqrt, weight_decay, beta1, beta2, eps, grad_scale, omb=None):
    """One step in float64 -> dict(p, m, v, tol_p, tol_m, tol_v), arrays like p. Scalars are taken as they come (hand it the
    float32 values the kernel gets). omb: (1 - beta1, 1 - beta2) where they are not the float64 differences -- the kernel
    forms them in float32, which is exact for the betas >= 0.5 of every test."""
    p, grad, m, v = (np.asarray(a, dtype=np.float64) for a in (p, grad, m, v))
    omb1, omb2 = omb if omb is not None else (1.0 - beta1, 1.0 - beta2)
    g = grad_scale * grad
    g = weight_decay * p + g
    m1 = m + omb1 * (g - m)
    v1 = beta2 * v + (omb2 * g) * g
    den = np.sqrt(v1) / bc2_sqrt + eps
    u = step_size * (m1 / den)
    p1 = p - u
    G = np.abs(grad_scale * grad) + weight_decay * np.abs(p)
    tol_m = 4 * E * (np.abs(m) + G)
    tol_v = 8 * E * v1
    tol_p = 4 * E * (np.abs(p1) + np.abs(u)) + step_size * tol_m / den
    return dict(p=p1, m=m1, v=v1, tol_p=tol_p, tol_m=tol_m, tol_v=tol_v)


def inputs(n, seed, decay):
    """(p, grad) float32 [n] as described in the module's docstring."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n)
    p[::13] *= 1e-4
    p = p.astype(np.float32)
    mag = 10.0 ** rng.uniform(-6.0, 2.0, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if decay:
        sign = np.where(p < 0, -1.0, 1.0)
    g = (mag * sign)
    g[::97] = 0.0
    return p, g.astype(np.float32)


def case(n, seed, form, weight_decay, grad_scale, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The inputs and the reference of ONE kernel step at step count t: for t > 1 the moments (and p) are what one reference
    step at t - 1 over another gradient left, rounded to float32; for t == 1 they are zero. -> dict with p, g, m, v (float32
    inputs), the float32 scalars, and `want` = step(...) over them."""
    b1, b2, ep, gs, wd = f32(beta1), f32(beta2), f32(eps), f32(grad_scale), f32(weight_decay)
    p, g = inputs(n, seed, weight_decay != 0)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    if t > 1:
        _, g0 = inputs(n, seed + 7919, weight_decay != 0)
        ss0, bs0 = scalars(form, lr, b1, b2, t - 1)
        prev = step(p, g0, m, v, ss0, bs0, wd, b1, b2, ep, gs)
        p, m, v = (prev[k].astype(np.float32) for k in ("p", "m", "v"))
        if weight_decay != 0:   # (the gradient keeps the sign of the p it meets)
            g = (np.abs(g) * np.where(p < 0, -1.0, 1.0)).astype(np.float32)
    ss, bs = scalars(form, lr, b1, b2, t)
    want = step(p, g, m, v, ss, bs, wd, b1, b2, ep, gs)
    return dict(p=p, g=g, m=m, v=v, step_size=ss, bc2_sqrt=bs, weight_decay=wd, beta1=b1, beta2=b2, eps=ep, grad_scale=gs, want=want)


def worst(got_p, got_m, got_v, want):
    """The largest share of each bar that the result uses -> (p, m, v); <= 1 passes. A tolerance of 0 takes an exact match."""
    out = []
    for got, key in ((got_p, "p"), (got_m, "m"), (got_v, "v")):
        err = np.abs(np.asarray(got, dtype=np.float64) - want[key])
        tol = want["tol_" + key]
        share = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
        out.append(float(share.max(initial=0.0)))
    return tuple(out)
