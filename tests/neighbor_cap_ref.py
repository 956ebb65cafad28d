"""The expected output of find_neighbors(maxNeighbors=K): the uncapped list (the oracle's), thinned row by row in NumPy, and
the seeded geometries the capped search is tested on.

Rule (K > 0): a row of k <= K hits is unchanged; a row of k > K hits keeps exactly the K hits at the canonical ranks
r_t = floor(t * k / K), t = 0 .. K-1, in that order (64-bit integers). startIndexs is the exclusive prefix sum of min(k, K).
Per-hit form of the same rule (a compaction pass): t = (r * K + k - 1) // k; rank r is kept iff t < K and (t * k) // K == r,
and its output slot is t."""
import numpy as np


def cap_ranks(k, K):
    """Canonical ranks a row of k hits keeps under cap K (K > 0), ascending: int64 [min(k, K)]."""
    k, K = int(k), int(K)
    if k <= K:
        return np.arange(k, dtype=np.int64)
    return (np.arange(K, dtype=np.int64) * k) // K


def cap_slot(r, k, K):
    """Output slot of the hit at canonical rank r of a row of k hits under cap K, or -1 when the cap drops it (Python
    integers: no overflow)."""
    r, k, K = int(r), int(k), int(K)
    if k <= K:
        return r
    t = (r * K + k - 1) // k
    return t if (t < K and (t * k) // K == r) else -1


def row_lengths(start, e):
    st = np.asarray(start).reshape(-1).astype(np.int64)
    return np.diff(np.append(st, int(e)))


def cap_list(start, packed, K):
    """(startIndexs [M,1] i32, packedNeighs [E,2] i32) of an uncapped CSR list -> the same pair under cap K (0 = no cap)."""
    start = np.asarray(start)
    packed = np.asarray(packed).reshape(-1, 2)
    if int(K) <= 0:
        return start.copy(), packed.copy()
    K = int(K)
    st = start.reshape(-1).astype(np.int64)
    k = row_lengths(st, len(packed))
    kept = np.minimum(k, K)
    new_start = np.concatenate([[0], np.cumsum(kept)[:-1]]).astype(np.int64) if len(k) else np.zeros(0, np.int64)
    row = np.repeat(np.arange(len(k), dtype=np.int64), kept)          # row of every output slot
    t = np.arange(int(kept.sum()), dtype=np.int64) - new_start[row]    # its slot inside the row
    rank = np.where(k[row] > K, (t * k[row]) // K, t)
    return new_start.astype(np.int32).reshape(-1, 1), np.ascontiguousarray(packed[st[row] + rank]).astype(np.int32)


# ------------------------------------------------------------------------------------------------- geometries
# Each: dict(pts, bids, centres, cbids, B, radius, scaleInv). Centres are always an array of their own (never the point
# array itself), so a search over them gets no visiting-order hint.

def _two_clouds(rng, sizes):
    pts = [rng.random((n, 3), dtype=np.float32) + np.float32(0.25 * b) for b, n in enumerate(sizes)]
    bids = [np.full((n, 1), b, np.int32) for b, n in enumerate(sizes)]
    return np.concatenate(pts).astype(np.float32), np.concatenate(bids)


def geom_mixed():
    """Two uniform clouds of 700 and 300 points, relative radius 0.25; centres = the points and 20 centres that lie
    outside every cloud's reach (10 per cloud)."""
    rng = np.random.default_rng(101)
    pts, bids = _two_clouds(rng, (700, 300))
    far = (np.float32(5.0) + rng.random((20, 3), dtype=np.float32)).astype(np.float32)
    fb = (np.arange(20, dtype=np.int32) % 2).reshape(-1, 1)
    return dict(pts=pts, bids=bids, centres=np.concatenate([pts, far]), cbids=np.concatenate([bids, fb]), B=2, radius=0.25,
                scaleInv=True)


def geom_mid_windows():
    """One cloud of 1500 points, 1300 uniform and a loose blob of 200 around the middle; relative radius 0.2 (5 cells per
    axis): the windows of the inner cells hold 257..512 points."""
    rng = np.random.default_rng(102)
    blob = (0.5 + 0.05 * rng.normal(size=(200, 3))).astype(np.float32)
    pts = np.concatenate([rng.random((1300, 3), dtype=np.float32), blob]).astype(np.float32)
    rng.shuffle(pts)
    bids = np.zeros((len(pts), 1), np.int32)
    return dict(pts=pts, bids=bids, centres=pts.copy(), cbids=bids, B=1, radius=0.2, scaleInv=True)


def geom_big_windows():
    """3000 points, 2000 uniform and a dense blob of 1000; relative radius 0.1: windows of more than 512 points and rows of
    more than 600 hits around the blob."""
    rng = np.random.default_rng(103)
    blob = (0.5 + 0.02 * rng.normal(size=(1000, 3))).astype(np.float32)
    pts = np.concatenate([rng.random((2000, 3), dtype=np.float32), blob]).astype(np.float32)
    rng.shuffle(pts)
    bids = np.zeros((len(pts), 1), np.int32)
    return dict(pts=pts, bids=bids, centres=pts.copy(), cbids=bids, B=1, radius=0.1, scaleInv=True)


def geom_many_centres():
    """Two uniform clouds of 3000 points each, absolute radius 0.12; centres = a shuffled subset of 5000 points (more than
    the 4096 of the small-list regime)."""
    rng = np.random.default_rng(104)
    pts, bids = _two_clouds(rng, (3000, 3000))
    sel = rng.permutation(len(pts))[:5000]
    return dict(pts=pts, bids=bids, centres=np.ascontiguousarray(pts[sel]), cbids=np.ascontiguousarray(bids[sel]), B=2,
                radius=0.12, scaleInv=False)


GEOMETRIES = dict(mixed=geom_mixed, mid_windows=geom_mid_windows, big_windows=geom_big_windows,
                  many_centres=geom_many_centres)


def uncapped(ops, g, wrap=lambda a: a, unwrap=lambda a: a):
    """compute_aabb -> sort -> find_neighbors of geometry g on an op surface -> dict of arrays (and the surface's handles)."""
    P, Bi = wrap(g["pts"]), wrap(g["bids"])
    F = wrap(np.zeros((len(g["pts"]), 1), np.float32))
    B, radius, si = g["B"], g["radius"], g["scaleInv"]
    mn, mx = ops.compute_aabb(P, Bi, B, si)
    keys, idx = ops.sort_points_step1(P, Bi, mn, mx, B, radius, si)
    sP, sB, _, cells = ops.sort_points_step2(P, Bi, F, keys, idx, mn, mx, B, radius, si)
    C, Cb = wrap(g["centres"]), wrap(g["cbids"])
    start, packed = ops.find_neighbors(C, Cb, sP, cells, mn, mx, radius, B, si)
    h = dict(mn=mn, mx=mx, sP=sP, sB=sB, cells=cells, C=C, Cb=Cb, idx=idx)
    r = dict(aabbMin=unwrap(mn), aabbMax=unwrap(mx), sortPts=unwrap(sP), sortBatchs=unwrap(sB), cellIndexs=unwrap(cells),
             indexs=unwrap(idx), startIndexs=unwrap(start), packedNeighs=unwrap(packed))
    r["_handles"] = h
    return r


def window_sizes(g, r):
    """Points in the 27-cell window of every centre (what the search kernel stages for it): int64 [M]."""
    cells = np.asarray(r["cellIndexs"]).astype(np.int64)
    nc = cells.shape[1]
    mn, mx = np.asarray(r["aabbMin"], np.float32), np.asarray(r["aabbMax"], np.float32)
    cb = np.clip(np.asarray(g["cbids"]).reshape(-1), 0, g["B"] - 1)
    ext = (mx - mn).max(axis=1).astype(np.float32)
    cs = (ext / np.float32(nc)).astype(np.float32)
    xyz = np.floor((np.asarray(g["centres"], np.float32) - mn[cb]) / cs[cb, None]).astype(np.int64)
    xyz = np.clip(xyz, 0, nc - 1)
    length = np.zeros((g["B"], nc + 2, nc + 2, nc + 2), np.int64)      # padded: cells outside the grid hold nothing
    length[:, 1:-1, 1:-1, 1:-1] = cells[..., 1] - cells[..., 0]
    out = np.zeros(len(cb), np.int64)
    for dx in (0, 1, 2):
        for dy in (0, 1, 2):
            for dz in (0, 1, 2):
                out += length[cb, xyz[:, 0] + dx, xyz[:, 1] + dy, xyz[:, 2] + dz]
    return out
