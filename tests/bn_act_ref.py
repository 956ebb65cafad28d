"""Reference of the fused dense glue (mccnn_bn_act_fwd / _bwd, MCConvModule.bn_relu_dropout): y = drop(act(bn(x))).

float64 NumPy forward and backward, the counter-based dropout mask in uint32 NumPy (csrc/bn_drop.h), the shared test
cases, and an f32 restatement of the kernels' statistics (per-lane shifted sums, Chan's merge in the kernels' tree, slab
partials) that shows the GPU test's bar attainable without a GPU.
"""
import numpy as np

SHAPES = [(1, 8), (2, 1), (63, 3), (65, 16), (257, 64), (1000, 130), (3, 1024), (4099, 33), (20000, 16)]
DROP_ALL = 1 << 32
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------- the mask
def mix(x):
    """murmur3 finaliser on uint32 (any shape)."""
    x = np.asarray(x, np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    x ^= x >> np.uint64(16)
    return x


def row_hash(seed, i):
    i = np.asarray(i, np.uint64)
    return mix((np.uint64(seed) + np.uint64(0x9E3779B9) * ((i + np.uint64(1)) & _M32)) & _M32)


def threshold(keepProb):
    """T = floor(keepProb * 2^32) in double; None -> 2^32 (keep everything)."""
    return DROP_ALL if keepProb is None else int(float(keepProb) * 4294967296.0)


def keep_bits(seed, i, j, T):
    """element-wise keep bit of (row i, column j)."""
    h = mix((row_hash(seed, i) + (np.asarray(j, np.uint64) & _M32)) & _M32)
    return h < np.uint64(T) if T < DROP_ALL else np.ones(h.shape, bool)


def keep_mask(seed, n, c, T):
    return keep_bits(seed, np.arange(n)[:, None], np.arange(c)[None, :], T)


# ------------------------------------------------------------------------------------------------- float64 op
def forward(x, gamma, beta, mov_mean, mov_var, training, relu=True, mask=None, scale=1.0, momentum=0.99, eps=1e-3):
    """-> dict(y, pre, xhat, mean, var, rstd, mov_mean, mov_var), all float64. mask: boolean [n, c] or None."""
    x, gamma, beta = (np.asarray(t, np.float64) for t in (x, gamma, beta))
    mm, mv = np.asarray(mov_mean, np.float64).copy(), np.asarray(mov_var, np.float64).copy()
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        mm = mm * momentum + mean * (1.0 - momentum)
        mv = mv * momentum + var * (1.0 - momentum)
    else:
        mean, var = mm, mv
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    pre = xhat * gamma + beta
    y = np.maximum(pre, 0.0) if relu else pre.copy()
    if training and mask is not None:
        y = np.where(mask, y * scale, 0.0)
    return dict(y=y, pre=pre, xhat=xhat, mean=mean, var=var, rstd=rstd, mov_mean=mm, mov_var=mv)


def backward(x, dy, gamma, beta, mean, rstd, relu=True, mask=None, scale=1.0, gate=None):
    """Training-mode gradients -> (dx, dgamma, dbeta), float64. gate: the ReLU gate, default pre > 0."""
    x, dy, gamma, beta = (np.asarray(t, np.float64) for t in (x, dy, gamma, beta))
    n = x.shape[0]
    xhat = (x - mean) * rstd
    if gate is None:
        gate = (xhat * gamma + beta) > 0.0
    g = dy.copy()
    if mask is not None:
        g = np.where(mask, g * scale, 0.0)
    if relu:
        g = np.where(gate, g, 0.0)
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dx = gamma * rstd * (g - dbeta / n - xhat * dgamma / n)
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------- cases
def make_case(n, c):
    """Seeded per shape (1000 + n + c): x with |mean| >> std in many columns, a constant column, an all-off column."""
    rng = np.random.default_rng(1000 + n + c)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, c)
    offset = rng.uniform(-30.0, 30.0, c)
    x = (offset + scale * rng.standard_normal((n, c))).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, c)
    gamma[rng.random(c) < 0.25] *= -1.0
    gamma = gamma.astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, c).astype(np.float32)
    if c >= 3:
        x[:, 1] = 3.25
        beta[1] = 0.25
        beta[2] = -8.0
    dy = rng.standard_normal((n, c)).astype(np.float32)
    mov_mean = rng.uniform(-1.0, 1.0, c).astype(np.float32)   # non-trivial starting values
    mov_var = rng.uniform(0.5, 2.0, c).astype(np.float32)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, mov_mean=mov_mean, mov_var=mov_var)


_CASES = {}


def case(n, c):
    """The case of a shape, made once and shared (treat as read-only)."""
    if (n, c) not in _CASES:
        d = make_case(n, c)
        for v in d.values():
            v.setflags(write=False)
        _CASES[(n, c)] = d
    return _CASES[(n, c)]


def band_share(pre, rel=1e-5):
    """Share of elements with |pre| <= rel * max|pre|: where an f32 gate may differ from the float64 one."""
    return float((np.abs(pre) <= rel * np.abs(pre).max()).mean())


def naive_f32_rstd(x, eps=1e-3):
    """What a plain f32 sum x^2 / n - mean^2 gives (the form the statistics tests must reject)."""
    x = np.asarray(x, np.float32)
    n = np.float32(x.shape[0])
    s1 = np.zeros(x.shape[1], np.float32)
    s2 = np.zeros(x.shape[1], np.float32)
    for r in range(x.shape[0]):
        s1 = s1 + x[r]
        s2 = s2 + x[r] * x[r]
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, np.float32(0))
    return (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float64)


# ------------------------------------------------------------------------------------------------- the kernels' f32 statistics
SMALL_ROWS, SLAB_ROWS, MAX_SLABS, TILE_COLS, THREADS = 256, 128, 64, 32, 256


def slab_rows(n):
    if n <= SMALL_ROWS:
        return n
    if -(-n // SLAB_ROWS) <= MAX_SLABS:
        return SLAB_ROWS
    return -(-(-(-n // MAX_SLABS)) // 32) * 32


def row_lanes(c):
    """Row lanes of a workgroup: 256 / (threads across a tile)."""
    vec = 4 if c % 4 == 0 else 1
    units, most, tw = c // vec, TILE_COLS // vec, 1
    while tw < most and tw < units:
        tw *= 2
    return THREADS // tw


def _chan(nA, mA, qA, nB, mB, qB):
    """Chan's merge in f32; counts are scalars (nB == 0: A unchanged, nA == 0: B)."""
    f32 = np.float32
    if nB == 0:
        return nA, mA, qA
    if nA == 0:
        return nB, mB, qB
    n = f32(nA + nB)
    f = f32(nB / n)
    w = f32(nA * f)
    d = mB - mA
    return n, mA + d * f, qA + qB + d * d * w


def _tree(parts):
    """parts[ry] = (cnt, mean, m2): lanes merged as the kernels' LDS tree does (ry with ry + s, s = R/2 .. 1)."""
    parts = list(parts)
    s = len(parts) // 2
    while s >= 1:
        for ry in range(s):
            parts[ry] = _chan(*parts[ry], *parts[ry + s])
        s //= 2
    return parts[0]


def kernel_stats_f32(x):
    """(mean, var) of the columns of x as the kernels compute them, in f32 NumPy: per row lane sums shifted by the slab's
    first row, Chan's merge over the lanes (tree), slab partials merged lane-strided and by the same tree."""
    f32 = np.float32
    x = np.asarray(x, f32)
    n, c = x.shape
    R, sr = row_lanes(c), slab_rows(n)
    zero = np.zeros(c, f32)
    slabs = []
    for row0 in range(0, n, sr):
        row1 = min(n, row0 + sr)
        K = x[row0]
        lanes = []
        for ry in range(R):
            rows = x[row0 + ry:row1:R]
            s1, s2 = zero.copy(), zero.copy()
            for v in rows:
                d = v - K
                s1 = s1 + d
                s2 = s2 + d * d
            cnt = f32(len(rows))
            q = s1 / cnt if len(rows) else zero
            lanes.append((cnt, K + q if len(rows) else K.copy(), np.maximum(s2 - s1 * q, f32(0))))
        slabs.append(_tree(lanes))
    if len(slabs) == 1:
        cnt, mean, m2 = slabs[0]
    else:
        lanes = []
        for ry in range(R):
            acc = (f32(0), zero.copy(), zero.copy())
            for s in range(ry, len(slabs), R):
                acc = _chan(*acc, *slabs[s])
            lanes.append(acc)
        cnt, mean, m2 = _tree(lanes)
    return mean, m2 / f32(n)


def kernel_forward_f32(x, gamma, beta, relu=True, eps=1e-3):
    """y, mean, rstd of the training forward without dropout, in the kernels' f32 arithmetic."""
    f32 = np.float32
    mean, var = kernel_stats_f32(x)
    rstd = f32(1) / np.sqrt(var + f32(eps))
    pre = (np.asarray(x, f32) - mean) * rstd * np.asarray(gamma, f32) + np.asarray(beta, f32)
    return (np.where(pre > 0, pre, f32(0)) if relu else pre), mean, rstd
