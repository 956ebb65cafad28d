"""Reference of the last linear layer + softmax cross-entropy as one op (mccnn_linear_xent_fwd / _bwd,
MCConvModule.linear_softmax_xent, VariableStore(fusedLoss=True)): float64 NumPy forward and backward of the definition in
include/mccnn.h, and the shared cases.

  z = x W + b,  lse_i = m_i + log(sum_j exp(z_ij - m_i)),  l_i = lse_i - z[i, y_i]
  live_i = 0 <= y_i < C and rw_i != 0,  D = max(number of live rows, 1),  loss = sum_live rw_i l_i / D
  pred_i = the lowest arg-max of row i,  correct = the live rows with pred_i == y_i
  dz_ij = g rw_i / D (exp(z_ij - lse_i) - [j == y_i]) on live rows, 0 elsewhere;  dx = dz W^T, dW = x^T dz, db = sum_i dz
"""
import numpy as np

# (n, cin, C): n on both sides of a 64-row tile, of the one-launch limit (256) and of a dW slab (512); C of 1, below, at,
# just above and several times a column tile (64); cin longer than a k chunk (32); 20000 rows: the long column sum of db
SHAPES = [(1, 1, 1), (2, 3, 2), (63, 5, 3), (64, 16, 21), (65, 64, 40), (256, 8, 40), (257, 33, 50), (300, 64, 64),
          (300, 40, 130), (129, 8, 257), (1000, 130, 65), (37, 520, 8), (4099, 24, 40), (20000, 16, 50)]
IDS = ["%dx%dx%d" % s for s in SHAPES]


def make_case(n, cin, C, hot=False):
    """Seeded per shape. hot (C >= 3): the logits of column 0 sit 95 above and those of column C - 1 95 below the others -- a
    naive exp overflows float32, the row losses reach 190. A fifth of the weights are 0; from 8 rows on, two labels are out
    of range (-1 and C)."""
    rng = np.random.default_rng(3000 + n + 31 * cin + 977 * C + (7 if hot else 0))
    x = rng.uniform(-2, 2, cin) + 10 ** rng.uniform(-1, 0.5, cin) * rng.standard_normal((n, cin))
    w = 10 ** rng.uniform(-1, 0, C) * rng.standard_normal((cin, C)) / np.sqrt(cin)
    b = rng.uniform(-3, 3, C)
    if hot and C >= 3:
        b[0] += 95
        b[C - 1] -= 95
    labels = rng.integers(0, C, n)
    rw = rng.uniform(0.25, 4, n)
    rw[rng.uniform(0, 1, n) < 0.2] = 0
    if n >= 8:
        labels[3] = -1
        labels[5] = C
    d = dict(x=x, w=w, b=b, rw=rw)
    d = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}
    d["labels"] = np.ascontiguousarray(labels, dtype=np.int32)
    return d


_CASES = {}


def case(n, cin, C, hot=False):
    """The case of a shape, made once and shared (read-only)."""
    key = (n, cin, C, bool(hot))
    if key not in _CASES:
        d = make_case(*key)
        for v in d.values():
            v.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


def linear(x, w, b):
    """z = x @ W + b in float64."""
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64) + np.asarray(b, np.float64)


def live_rows(labels, C, rw=None):
    labels = np.asarray(labels).reshape(-1)
    live = (labels >= 0) & (labels < C)
    if rw is not None:
        live &= np.asarray(rw).reshape(-1) != 0
    return live


def forward(z, labels, rw=None):
    """-> dict(lse [n], rows [n] (l_i, 0 on rows that are not live), loss, pred [n], D, correct, live [n]) from the logits
    handed in, float64."""
    z = np.asarray(z, np.float64)
    n, C = z.shape
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    live = live_rows(labels, C, rw)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    zy = z[np.arange(n), np.clip(labels, 0, C - 1)]
    wgt = np.ones(n) if rw is None else np.asarray(rw, np.float64).reshape(-1)
    rows = np.where(live, lse - zy, 0.0)
    D = max(int(live.sum()), 1)
    loss = float((np.where(live, wgt, 0.0) * rows).sum() / D)
    pred = np.argmax(z, 1).astype(np.int32)   # (the first of equal maxima)
    correct = int((live & (pred == labels)).sum())
    return dict(lse=lse, rows=rows, loss=loss, pred=pred, D=D, correct=correct, live=live)


def backward(x, w, z, labels, rw=None, g=1.0, lse=None, D=None):
    """-> dict(dz, dx, dw, db), float64, from the logits (and, when given, the lse and D) handed in."""
    z = np.asarray(z, np.float64)
    n, C = z.shape
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    out = forward(z, labels, rw)
    lse = out["lse"] if lse is None else np.asarray(lse, np.float64)
    D = out["D"] if D is None else int(D)
    wgt = np.ones(n) if rw is None else np.asarray(rw, np.float64).reshape(-1)
    p = np.exp(z - lse[:, None])
    p[np.arange(n), np.clip(labels, 0, C - 1)] -= 1.0
    dz = np.where(out["live"], float(g) * wgt / D, 0.0)[:, None] * p
    dz[~out["live"]] = 0.0
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    return dict(dz=dz, dx=dz @ w.T, dw=x.T @ dz, db=dz.sum(0))
