"""Reference of the linear layer + dense glue as one op (mccnn_linear_bn_act_fwd / _bwd,
MCConvModule.linear_bn_relu_dropout): z = x @ W + b, y = drop(act(bn(z))).

float64 NumPy forward and backward on top of tests/bn_act_ref.py (the glue and the mask), the shared cases, and the naive
f32 statistics a sloppy matmul epilogue would compute.
"""
import numpy as np

import bn_act_ref as bn

# (n, cin, cout): n on both sides of 256 and of a slab boundary, more than one slab per lane and more than 64 x 128 rows
# (20000); cin and cout no multiple of 4 or 16; cin longer than a k chunk (33, 64, 130, 520); cout wider than a column tile
# (70, 128); cout = 1
SHAPES = [(1, 1, 1), (2, 3, 1), (63, 5, 3), (65, 16, 16), (256, 8, 40), (257, 33, 17), (300, 64, 128), (1000, 130, 70),
          (37, 520, 8), (4099, 24, 40), (20000, 16, 32)]
IDS = ["%dx%dx%d" % s for s in SHAPES]


def make_case(n, cin, cout):
    """Seeded per shape: columns of z with |mean| >> std (a bias of up to 100 over a product of O(1)), a constant column
    and an all-off column."""
    rng = np.random.default_rng(2000 + n + 31 * cin + 977 * cout)
    x = rng.uniform(-2.0, 2.0, cin) + 10.0 ** rng.uniform(-1.0, 0.5, cin) * rng.standard_normal((n, cin))
    w = 10.0 ** rng.uniform(-1.5, 0.0, cout) * rng.standard_normal((cin, cout)) / np.sqrt(cin)
    b = rng.uniform(-100.0, 100.0, cout)
    gamma = rng.uniform(0.5, 1.5, cout)
    gamma[rng.uniform(0.0, 1.0, cout) < 0.25] *= -1.0
    beta = rng.uniform(-0.5, 0.5, cout)
    if cout >= 3:
        w[:, 1] = 0.0
        b[1] = 3.25
        beta[1] = 0.25
        beta[2] = -8.0
    dy = rng.standard_normal((n, cout))
    mov_mean = rng.uniform(-1.0, 1.0, cout)
    mov_var = rng.uniform(0.5, 2.0, cout)
    d = dict(x=x, w=w, b=b, gamma=gamma, beta=beta, dy=dy, mov_mean=mov_mean, mov_var=mov_var)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}


_CASES = {}


def case(n, cin, cout):
    """The case of a shape, made once and shared (read-only)."""
    key = (n, cin, cout)
    if key not in _CASES:
        d = make_case(*key)
        for v in d.values():
            v.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


def linear(x, w, b):
    """z = x @ W + b in float64."""
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64) + np.asarray(b, np.float64)


def forward(d, training=True, relu=True, mask=None, scale=1.0, z=None):
    """bn_act_ref.forward over z (default: the float64 z of the case) -> its dict plus z."""
    z = linear(d["x"], d["w"], d["b"]) if z is None else np.asarray(z, np.float64)
    out = bn.forward(z, d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], training, relu, mask, scale)
    out["z"] = z
    return out


def backward(d, z, mean, rstd, relu=True, mask=None, scale=1.0, gate=None):
    """-> dict(dz, dx, dw, db, dgamma, dbeta), float64, from the z, statistics and gates handed in."""
    dz, dgamma, dbeta = bn.backward(z, d["dy"], d["gamma"], d["beta"], mean, rstd, relu, mask, scale, gate)
    x, w = np.asarray(d["x"], np.float64), np.asarray(d["w"], np.float64)
    return dict(dz=dz, dx=dz @ w.T, dw=x.T @ dz, db=dz.sum(0), dgamma=dgamma, dbeta=dbeta)
