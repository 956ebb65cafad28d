"""TEST INFRASTRUCTURE for pdfMode='point': the expected output of compute_pdf_points / expand_pdf in NumPy float64 over the
ORACLE's neighbour rows, and the oracle-backed op surface with the two ops added (a whole graph through `ops=`).

Definition (per sorted point j of cloud b, R_b = radius * maxExtent_b with scaleInv, else radius, in f32):
    N(j)       = the row of find_neighbors called with the sorted points as their own centres
    counts[j]  = |N(j)|
    density[j] = sum over l in N(j) of prod_a (1/h) 0.39894228 exp(-0.5 ((p_l,a - p_j,a) / (R_b h))^2),  h = window
    pdfs[e]    = float32(density[j]) / float32(len_i)   for the edge e = (j, i) of an uncapped list over that grid
Never imported by the product package."""
import numpy as np

from tests.oracle_ops import OracleOps, _n, _t


def point_rows(oracle, sortPts, sortBatchs, cellIndexs, aabbMin, aabbMax, radius, batchSize, scaleInv):
    """(startIndexs [N,1], packedNeighs [E,2]) of the oracle's search with the sorted points as their own centres."""
    return oracle.find_neighbors(sortPts, sortBatchs, sortPts, cellIndexs, aabbMin, aabbMax, radius, batchSize, scaleInv)


def cloud_radius(sortBatchs, aabbMin, aabbMax, radius, batchSize, scaleInv):
    """R_b of every point's cloud in the f32 arithmetic of the kernels -> float32 [N]."""
    mn, mx = np.asarray(aabbMin, np.float32), np.asarray(aabbMax, np.float32)
    with np.errstate(over="ignore"):      # (a batch id without points has the kernels' empty box: FLT_MAX, -FLT_MAX)
        ext = (mx - mn).max(axis=1).astype(np.float32)
    b = np.clip(np.asarray(sortBatchs).reshape(-1), 0, batchSize - 1)
    R = (np.float32(radius) * ext).astype(np.float32) if scaleInv else np.full(len(ext), np.float32(radius), np.float32)
    return R[b]


def density_ref(oracle, sortPts, sortBatchs, cellIndexs, aabbMin, aabbMax, window, radius, batchSize, scaleInv):
    """-> (density float64 [N,1], counts int32 [N,1]) from the oracle's rows, the Gaussians in float64."""
    sortPts = np.asarray(sortPts, np.float32)
    n = len(sortPts)
    start, packed = point_rows(oracle, sortPts, sortBatchs, cellIndexs, aabbMin, aabbMax, radius, batchSize, scaleInv)
    packed = np.asarray(packed).reshape(-1, 2)
    assert len(np.asarray(start).reshape(-1)) == n
    l, j = packed[:, 0].astype(np.int64), packed[:, 1].astype(np.int64)
    counts = np.bincount(j, minlength=n).astype(np.int32)
    R = cloud_radius(sortBatchs, aabbMin, aabbMax, radius, batchSize, scaleInv).astype(np.float64)
    h = float(np.float32(window))
    P = sortPts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (P[l] - P[j]) / (R[j] * h)[:, None]
        g = np.prod((1.0 / h) * 0.39894228 * np.exp(-0.5 * d * d), axis=1)
    density = np.bincount(j, weights=g, minlength=n) if len(j) else np.zeros(n)
    return density.reshape(-1, 1), counts.reshape(-1, 1)


def row_lengths(startIndexs, e):
    st = np.asarray(startIndexs).reshape(-1).astype(np.int64)
    return np.diff(np.append(st, int(e)))


def expand_ref(density, startIndexs, packedNeighs):
    """pdfs float32 [E,1]: np.float32(density[j]) / np.float32(len_i), one correctly rounded f32 divide."""
    packed = np.asarray(packedNeighs).reshape(-1, 2)
    k = row_lengths(startIndexs, len(packed))
    d32 = np.asarray(density).reshape(-1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = d32[packed[:, 0]] / k[packed[:, 1]].astype(np.float32)
    return out.astype(np.float32).reshape(-1, 1)


class PointPdfOracleOps(OracleOps):
    """OracleOps with compute_pdf_points / expand_pdf (the float64 reference above, rounded to f32), on CPU torch tensors."""

    def compute_pdf_points(self, p, b, cells, mn, mx, window, radius, B, si):
        d, c = density_ref(self.o, _n(p), _n(b), _n(cells), _n(mn), _n(mx), window, radius, B, si)
        return _t(d.astype(np.float32)), _t(c)

    def expand_pdf(self, density, st, pk):
        return _t(expand_ref(_n(density), _n(st), _n(pk)))


# ------------------------------------------------------------------------------------------------- inputs
def small_clouds():
    """Three clouds of 37, 1 and 90 points in cubes of side 0.05 at offsets 0.3 b: every cloud lies inside every one of its
    balls at absolute radius 0.1 (rows 37 / 1 / 90); at relative radius 2.0 too, except the one-point cloud, whose R is 0."""
    rng = np.random.default_rng(311)
    sizes = (37, 1, 90)
    pts = [np.float32(0.05) * rng.random((n, 3), dtype=np.float32) + np.float32(0.3 * b) for b, n in enumerate(sizes)]
    bids = [np.full((n, 1), b, np.int32) for b, n in enumerate(sizes)]
    return np.concatenate(pts).astype(np.float32), np.concatenate(bids), len(sizes), sizes


def sorted_grid(ops, pts, bids, B, radius, scaleInv, wrap=lambda a: a):
    """compute_aabb -> sort of (pts, bids) on an op surface -> (mn, mx, sortPts, sortBatchs, cellIndexs, indexs) handles."""
    P, Bi = wrap(pts), wrap(bids)
    F = wrap(np.zeros((len(pts), 1), np.float32))
    mn, mx = ops.compute_aabb(P, Bi, B, scaleInv)
    keys, idx = ops.sort_points_step1(P, Bi, mn, mx, B, radius, scaleInv)
    sP, sB, _, cells = ops.sort_points_step2(P, Bi, F, keys, idx, mn, mx, B, radius, scaleInv)
    return mn, mx, sP, sB, cells, idx
