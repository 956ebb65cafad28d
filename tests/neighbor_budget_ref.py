"""The cap find_neighbors(maxEdges=B) must choose, in Python integers, and a geometry with rows far above 65 536 hits. The
list itself is then tests/neighbor_cap_ref.py's cap_list (or tests/neighbor_sample_ref.py's sample_list) at that cap.

Rule: with k_i the uncapped row lengths, kmax = max(max_i k_i, 1), Ku = maxNeighbors (0 = none) and S(K) = sum_i min(k_i, K),
    K* = max{ K : 1 <= K <= min(Ku, kmax), S(K) <= B }   if S(1) <= B,      K* = 1 otherwise (every non-empty row keeps a hit)."""
import numpy as np

from tests.neighbor_cap_ref import GEOMETRIES, cap_list, row_lengths, uncapped  # noqa: F401 (re-exported)


def edges_under(k, K):
    """S(K) = sum_i min(k_i, K) as a Python integer."""
    return sum(min(int(x), int(K)) for x in np.asarray(k).reshape(-1).tolist())


def budget_cap(k, B, Ku=0):
    """K* of row lengths k under the budget B > 0 and the user's cap Ku (0 = none): bisection over [1, min(Ku, kmax)]."""
    k = [int(x) for x in np.asarray(k).reshape(-1).tolist()]
    B, Ku = int(B), int(Ku)
    assert B > 0 and Ku >= 0
    top = max(max(k, default=0), 1)
    if Ku > 0:
        top = min(top, Ku)
    S = lambda K: sum(min(x, K) for x in k)
    if S(1) > B:
        return 1
    lo, hi = 1, top          # S(lo) <= B always
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if S(mid) <= B:
            lo = mid
        else:
            hi = mid - 1
    return lo


def geom_tall_rows():
    """70 000 points in a ball of radius 0.03 about the middle of the unit cube and the cube's 8 corners, relative radius 0.1;
    6 centres: three that reach the whole ball, one that reaches most of it, a corner (1 hit) and one that reaches nothing."""
    rng = np.random.default_rng(105)
    v = rng.normal(size=(70000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ball = (v * (0.03 * rng.random((70000, 1)) ** (1.0 / 3.0)) + 0.5).astype(np.float32)
    corners = np.asarray([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    pts = np.concatenate([ball, corners]).astype(np.float32)
    bids = np.zeros((len(pts), 1), np.int32)
    centres = np.asarray([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.52, 0.5, 0.5], [0.58, 0.5, 0.5], [0, 0, 0], [0.25, 0.25, 0.25]],
                         np.float32)
    return dict(pts=pts, bids=bids, centres=centres, cbids=np.zeros((6, 1), np.int32), B=1, radius=0.1, scaleInv=True)


BUDGET_GEOMETRIES = dict(GEOMETRIES, tall_rows=geom_tall_rows)

#: geometry -> (m, uncapped E, kmax, ((B, K*, E(K*)), ...)): computed on the CPU from the oracle's lists
#: (tests/test_neighbor_budget_cpu.py asserts every figure)
TABLE = dict(
    mixed=(1020, 28868, 59, ((500, 1, 1000), (1020, 1, 1000), (2040, 2, 2000), (7217, 7, 6971), (14434, 15, 14330),
                             (28867, 58, 28867), (28868, 59, 28868), (28869, 59, 28868))),
    mid_windows=(1500, 99172, 240, ((24793, 16, 23862), (49586, 38, 49291), (99171, 239, 99171))),
    big_windows=(3000, 1032324, 1015, ((6000, 2, 5995), (258081, 237, 257718), (516162, 492, 515571),
                                       (1032323, 1014, 1032318))),
    many_centres=(5000, 97982, 40, ((5000, 1, 5000), (24495, 4, 20000), (48991, 9, 44740), (97981, 39, 97981))),
    tall_rows=(6, 273288, 70000, ((6, 1, 5), (200000, 49999, 199997), (262149, 66287, 262149), (270000, 68904, 270000),
                                  (273287, 69999, 273285))),
)
TALL_ROW_LENGTHS = (70000, 70000, 70000, 63287, 1, 0)
