"""find_neighbors(maxEdges=B) on the 100k room: ms per call of the budgeted search (count + selection + scan + fill, HIP events,
the op with its edge-count read-back), the cap K* it chose and the resulting E, for B = E/2 and E/4 of the uncapped list (or
the budgets on the command line) -- and, from the same process, ms per call of find_neighbors(maxNeighbors=K*), the yardstick:
the same count and fill kernels around a plain scan. Their difference is what the selection (and the clamp in the scan's
load) costs; the launches per call of both are printed beside it (mccnn_debug_launch_count)."""
import sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd import MCConvModule as M, _lib
from mccnn_amd.workloads import make_room
lib = _lib.load()
P = torch.from_numpy(make_room(100000, 20180601)).cuda()
Bi = torch.zeros((P.shape[0], 1), dtype=torch.int32, device=P.device)
mn, mx = M.compute_aabb(P, Bi, 1, False)
sP, sB, cells, idx, inv = M.build_grid(P, Bi, mn, mx, 1, 0.1, False)


def timed(**kw):
    """-> (best ms per call, worst of five runs, launches per call, the last result)"""
    for _ in range(10):
        res = M.find_neighbors(P, Bi, sP, cells, mn, mx, 0.1, 1, False, **kw)
    torch.cuda.synchronize()
    best = worst = None
    for rep in range(5):   # best of five runs of 50 calls
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        n0 = lib.mccnn_debug_launch_count()
        e0.record()
        for _ in range(50):
            res = M.find_neighbors(P, Bi, sP, cells, mn, mx, 0.1, 1, False, **kw)
        e1.record(); torch.cuda.synchronize()
        launches = (lib.mccnn_debug_launch_count() - n0) / 50.0
        t = e0.elapsed_time(e1) / 50
        best = t if best is None else min(best, t)
        worst = t if worst is None else max(worst, t)
    return best, worst, launches, res


t0, w0, l0, (st, pk) = timed()
E = pk.shape[0]
print("no cap                       find_neighbors ms %.4f (worst of 5: %.4f)  launches %.1f  E %d" % (t0, w0, l0, E))
budgets = [int(a) for a in sys.argv[1:]] or [E // 2, E // 4]
for B in budgets:
    tb, wb, lb, (st, pk, cap) = timed(maxEdges=B, returnCap=True)
    K = int(cap[0])   # (read back here, once, after the timing)
    tc, wc, lc, (cst, cpk) = timed(maxNeighbors=K)
    assert torch.equal(st, cst) and torch.equal(pk, cpk)
    print("maxEdges %-9d K* %-5d E %-9d budget search ms %.4f (worst of 5: %.4f)  launches %.1f | maxNeighbors=K* ms %.4f (worst of 5: "
          "%.4f)  launches %.1f | selection + clamped scan - plain scan: %+.4f ms" % (B, K, pk.shape[0], tb, wb, lb, tc, wc, lc, tb - tc))
