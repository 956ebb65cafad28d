"""The budgeted search inside a native geometry's chain (native.build_geometry(maxEdges=B)) on the 100k room, B = E/2 and E/4 of
the uncapped list (or the budgets on the command line): ms per chain and launches per chain (HIP events around 50 builds, best
and worst of five runs) of a geometry that shares its grid and computes no PDFs -- head clear, search, a fill of ones -- with
    the budget                 count, three selection levels, clamped scan, fill
    maxNeighbors = K*          count, scan, fill: the yardstick inside the chain (the same count and fill kernels)
beside the op-level find_neighbors(maxEdges=B) with its edge-count read-back (tools/nb_budget_time.py times that one alone).
Then a small list -- 4000 centres of the room over the same grid, at most 4096: three search launches in the chain (count,
one-workgroup selection, a fill pass that clamps and scans) against the op's four."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd import MCConvModule as M, _lib, native  # noqa: E402
from mccnn_amd.workloads import make_room  # noqa: E402

lib = _lib.load()
R = 0.1
P = torch.from_numpy(make_room(100000, 20180601)).cuda()
Bi = torch.zeros((P.shape[0], 1), dtype=torch.int32, device=P.device)
mn, mx = M.compute_aabb(P, Bi, 1, False)
nc = M._num_cells(mn, mx, 1, R, False)
sP, sB, cells, idx, inv = M.build_grid(P, Bi, mn, mx, 1, R, False)
owner = native.build_geometry(P, Bi, P, Bi, mn, mx, 1, nc, R, False, 0.25, False)
owner.edges()


def timed(fn):
    """-> (best ms per call, worst of five runs of 50 calls, launches per call, the last result)"""
    for _ in range(10):
        res = fn()
    torch.cuda.synchronize()
    best = worst = None
    for _rep in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n0 = lib.mccnn_debug_launch_count()
        e0.record()
        for _ in range(50):
            res = fn()
        e1.record()
        torch.cuda.synchronize()
        launches = (lib.mccnn_debug_launch_count() - n0) / 50.0
        t = e0.elapsed_time(e1) / 50
        best = t if best is None else min(best, t)
        worst = t if worst is None else max(worst, t)
    return best, worst, launches, res


def chain(C, Cb, **kw):
    def fn():
        g = native.build_geometry(P, Bi, C, Cb, mn, mx, 1, nc, R, False, 0.25, False, grid_from=owner, **kw)
        return g
    return fn


def report(label, C, Cb, budgets):
    t0, w0, l0, g0 = timed(chain(C, Cb))
    E = g0.edges()
    print("%s: %d centres, uncapped chain ms %.4f (worst of 5: %.4f)  launches %.1f  E %d" % (label, C.shape[0], t0, w0, l0, E))
    for B in budgets or [E // 2, E // 4]:
        tb, wb, lb, gb = timed(chain(C, Cb, maxEdges=B))
        K = int(gb.chosen_cap()[0])   # (read back here, once, after the timing)
        tc, wc, lc, gc = timed(chain(C, Cb, maxNeighbors=K))
        assert gb.edges() == gc.edges() and torch.equal(gb.neighbors()[1], gc.neighbors()[1])
        to, wo, lo, ro = timed(lambda: M.find_neighbors(C, Cb, sP, cells, mn, mx, R, 1, False, maxEdges=B, returnCap=True))
        assert torch.equal(ro[1], gb.neighbors()[1]) and int(ro[2][0]) == K
        print("%s maxEdges %-9d K* %-5d E %-9d | chain, budget: ms %.4f (worst %.4f) launches %.1f | chain, maxNeighbors=K*: ms %.4f "
              "(worst %.4f) launches %.1f | selection + clamp in the chain: %+.4f ms, %+.1f launches | op-level budget search: ms %.4f "
              "(worst %.4f) launches %.1f" % (label, B, K, gb.edges(), tb, wb, lb, tc, wc, lc, tb - tc, lb - lc, to, wo, lo))


budgets = [int(a) for a in sys.argv[1:]]
report("room", P, Bi, budgets)
sel = torch.randperm(P.shape[0], generator=torch.Generator().manual_seed(1))[:4000].cuda()
report("small list", P[sel].contiguous(), Bi[sel].contiguous(), [])
