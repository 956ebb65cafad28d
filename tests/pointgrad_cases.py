"""Seeded geometries of the position-gradient edge tests (tests/test_point_grads_edges_cpu.py builds them with the CPU
oracle and asserts what each one reaches; tests/test_gpu_point_grads_edges.py checks that the GPU ops give the same
integers and runs the gradient kernels over them), the layer shapes they run with, and the comparison rules (the project's
bar, hybrid sums over ambiguous edges)."""
import numpy as np

from tests import pointgrad_ref as ref
from tests.helpers import make_cloud, make_mlp, make_room, run_chain
from mccnn_amd.workloads import conv_nb

WINDOW = 0.2
RTOL = 1e-4
AMBIGUITY_CAP = 0.02                                     # ambiguous edges / E, a condition of every case
CLUMPS = (255, 256, 257, 1023, 1024, 1025, 2049, 3073)   # A: the exact length of each clump's row
FAR_CENTRES = 4                                          # A: centres that reach no point
EMPTY_CLOUDS = (3, 7)                                    # B, D: batches without points

SHAPES = [  # combin, fin, fout, bf16
    (True, 1, 64, False),
    (True, 3, 8, False),
    (True, 8, 3, False),      # combin with Fin > 4
    (True, 1, 13, False),     # padded neurons (13 of 16)
    (True, 2, 5, False),      # padded neurons (10 of 16)
    (True, 4, 130, False),    # nb = 65
    (False, 16, 16, False),
    (False, 520, 520, False),  # nb = 65
    (False, 24, 24, True),    # bf16 rows of 24
]


def shape_id(s):
    return "%s%d-%d%s" % ("T" if s[0] else "F", s[1], s[2], "-bf16" if s[3] else "")


def mlp_for(shape):
    combin, fin, fout, _ = shape
    return make_mlp(conv_nb(fin, fout, combin), 1000 + 7 * fin + fout)


# ---------------------------------------------------------------------------------------------- geometries
def _geom_A(scaleInv):
    """Tight clumps of exactly k points within 0.3 R of a centre, 0.5 apart on x (R = 0.1), one centre on each, plus
    FAR_CENTRES centres between the clumps that reach nothing. scaleInv: the relative radius that gives R = 0.1."""
    rng = np.random.default_rng(0)
    R = 0.1
    pts, cen = [], []
    for i, k in enumerate(CLUMPS):
        c = np.array([0.5 * i, 0.0, 0.0])
        v = rng.normal(size=(k, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        pts.append(c + v * (0.3 * R * rng.random(k) ** (1 / 3))[:, None])
        cen.append(c)
    cen += [np.array([0.5 * i + 0.25, 0.0, 0.0]) for i in range(FAR_CENTRES)]
    P = np.concatenate(pts).astype(np.float32)
    C = np.array(cen, np.float32)
    radius = R
    if scaleInv:
        radius = R / float((P.max(0) - P.min(0)).max())
    return dict(pts=P, bids=np.zeros((len(P), 1), np.int32), centres=C, cbids=np.zeros((len(C), 1), np.int32), B=1,
                radius=radius, scaleInv=scaleInv)


def _geom_B(shift=0.0):
    """B = 12 clustered ragged clouds (relative radius 0.1), clouds 3 and 7 emptied. Per cloud: 3 lonely points far off
    the cloud's corner (nobody reaches them), pooling centres = every 4th point jittered, 2 of them pushed outside the
    box, and 2 centres far outside that reach nothing."""
    B = 12
    rng = np.random.default_rng(41)
    p0, b0 = make_cloud(300, B, 40, "clustered", ragged=True)
    pts, bids, cen, cb, lonely = [], [], [], [], []
    n = 0
    for b in range(B):
        if b in EMPTY_CLOUDS:
            continue
        p = p0[b0[:, 0] == b].astype(np.float64)
        base = 0.25 * b
        far = base + np.array([[1.6, 1.6, 1.6], [1.6, 1.45, 1.6], [1.45, 1.6, 1.6]])
        c = p[::4] + 0.02 * rng.normal(size=(len(p[::4]), 3))
        c[:2] = base + np.array([[-0.05, 0.5, 0.5], [0.5, 1.08, 0.5]])          # just outside the box
        c = np.concatenate([c, base + np.array([[-0.9, -0.9, -0.9], [0.5, -1.0, 2.5]])])  # far outside: empty rows
        pts += [p, far]
        lonely += list(range(n + len(p), n + len(p) + len(far)))
        n += len(p) + len(far)
        bids.append(np.full(len(p) + len(far), b))
        cen.append(c)
        cb.append(np.full(len(c), b))
    P = (np.concatenate(pts) + shift).astype(np.float32)
    C = (np.concatenate(cen) + shift).astype(np.float32)
    return dict(pts=P, bids=np.concatenate(bids).astype(np.int32).reshape(-1, 1), centres=C,
                cbids=np.concatenate(cb).astype(np.int32).reshape(-1, 1), B=B, radius=0.1, scaleInv=True,
                lonely=np.array(lonely))


def _geom_C():
    """Coordinates on a 1/64 lattice (many points on every box face); cloud 1 has x and y extents exactly equal (40/64)
    and z shorter. Relative radius, centres = the points (level 0 of a PointHierarchy)."""
    rng = np.random.default_rng(51)
    B = 3
    pts, bids = [], []
    for b in range(B):
        n = 500
        if b == 1:
            q = np.concatenate([rng.integers(0, 41, (n, 2)), rng.integers(0, 25, (n, 1))], 1)
            q[:2, :2] = [[0, 0], [40, 40]]
        else:
            q = rng.integers(0, 33 + 8 * b, (n, 3))
        pts.append(q / 64.0 + 0.25 * b)
        bids.append(np.full(n, b))
    P = np.concatenate(pts).astype(np.float32)
    return dict(pts=P, bids=np.concatenate(bids).astype(np.int32).reshape(-1, 1), centres=None, cbids=None, B=B,
                radius=0.12, scaleInv=True, equal_xy=1)


def _geom_E():
    """Two 20000-point rooms, absolute radius 0.1, centres = the points."""
    p = [make_room(20000, s) for s in (61, 62)]
    P = np.concatenate(p).astype(np.float32)
    bids = np.concatenate([np.full(len(q), b) for b, q in enumerate(p)]).astype(np.int32).reshape(-1, 1)
    return dict(pts=P, bids=bids, centres=None, cbids=None, B=2, radius=0.1, scaleInv=False)


GEOMS = ("A_abs", "A_rel", "B", "C", "D", "E")


def geometry(name):
    if name in ("A_abs", "A_rel"):
        return _geom_A(name == "A_rel")
    if name == "B":
        return _geom_B()
    if name == "D":
        return _geom_B(500.0)
    if name == "C":
        return _geom_C()
    if name == "E":
        return _geom_E()
    raise ValueError(name)


def build(g, ops, wrap, unwrap):
    """The op chain (compute_aabb, sort, find_neighbors, compute_pdf) of geometry g on an op surface -> run_chain's dict."""
    f0 = np.zeros((len(g["pts"]), 1), np.float32)
    return run_chain(ops, wrap, unwrap, g["pts"], g["bids"], f0, g["B"], g["radius"], g["scaleInv"], window=WINDOW, fout=1,
                     centres=g["centres"], centre_bids=g["cbids"])


def centres_of(g):
    return g["pts"] if g["centres"] is None else g["centres"]


def row_lengths(r):
    st = np.asarray(r["startIndexs"]).reshape(-1).astype(np.int64)
    return np.diff(np.append(st, len(r["packedNeighs"])))


def in_degree(r):
    return np.bincount(np.asarray(r["packedNeighs"])[:, 0], minlength=len(r["sortPts"]))


def ambiguity(g, r, shape):
    """conv_ambiguity of a layer shape over geometry g's chain r."""
    return ref.conv_ambiguity(r["sortPts"], centres_of(g), r["sortBatchs"], r["packedNeighs"], r["aabbMin"], r["aabbMax"],
                              mlp_for(shape), g["radius"], g["scaleInv"])


# ---------------------------------------------------------------------------------------------- bars
def close_figures(got, want):
    """(norm-wise, element-wise) error of the project's bar: ||got - want|| / ||want|| and max |got - want| / max |want|."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-30)
    nrm = float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))
    elem = float(np.abs(got - want).max() / scale) if want.size else 0.0
    return nrm, elem


def check_close(got, want, what):
    """The project's bar: norm-wise relative error <= 1e-4, and every element within 1e-4 x the tensor's largest magnitude.
    Prints the two figures before it asserts."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    nrm, elem = close_figures(got, want)
    print("  %-28s norm-wise %.3e  element-wise %.3e" % (what, nrm, elem))
    assert nrm <= RTOL and elem <= RTOL, "%s: norm-wise %.3e, element-wise %.3e" % (what, nrm, elem)


def batch_sums_f32(per_row, row_batch, B):
    """A plain float32 summation of per-row values, in row order, per batch."""
    out = np.zeros(B, np.float32)
    for b in range(B):
        v = np.asarray(per_row)[row_batch == b].astype(np.float32)
        out[b] = np.cumsum(v, dtype=np.float32)[-1] if v.size else np.float32(0)
    return out


def row_batch(r, g):
    """The batch of each centre row (the batch of its first neighbour; rows without edges count for no batch)."""
    st = np.asarray(r["startIndexs"]).reshape(-1)
    deg = row_lengths(r)
    rb = np.full(len(st), -1, np.int64)
    has = deg > 0
    rb[has] = np.asarray(r["sortBatchs"]).reshape(-1)[np.asarray(r["packedNeighs"])[st[has], 0]]
    return rb


def per_row(values, r):
    """Sum of per-edge values over each centre row, in float64."""
    return np.bincount(np.asarray(r["packedNeighs"])[:, 1], weights=np.asarray(values, np.float64),
                       minlength=len(row_lengths(r)))
