"""Position gradients of the KDE, per-edge against per-point, on the SAME neighbour list: ms per call (HIP events, best and
worst of five runs of 50 calls after a warm-up) on
  room    the 100k room, same-level list, absolute radius 0.1, window 0.2
  pool_1  the Pool_1 list of workloads.mcclass_h on BASELINE cfg2 (32 clouds x 4096 points, level 0 -> level 1, relative
          radius 0.2, window 0.2)
 (a) the per-edge backward: mccnn_compute_pdf_bwd_points (every pair of a centre's row, [E,3] per-edge rows) and
     mccnn_edge_grad_reduce (their gather through the transposed list)
 (b) the per-point backward: mccnn_expand_pdf_bwd (the gather of the upstream gradient through the transposed list) and
     mccnn_compute_pdf_points_bwd (the forward's sweep again), with the forward sweep beside it
through the C entries on preallocated buffers; with a relative radius both forms also produce dR. The sweep backward runs
once per grid and window however many lists share the density; (a) runs once per list."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd import MCConvModule as M
from mccnn_amd import workloads as W
from mccnn_amd._lib import load, check, ptr, stream_handle
from mccnn_amd.MCConvBuilder import PointHierarchy


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    best = worst = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / 50
        best, worst = (t, t) if best is None else (min(best, t), max(worst, t))
    return best, worst


def case(name, P, Bi, C, Cb, mn, mx, B, radius, rel, window):
    lib = load()
    dev = P.device
    sP, sB, cells, idx, inv = M.build_grid(P, Bi, mn, mx, B, radius, rel)
    st, pk = M.find_neighbors(C, Cb, sP, cells, mn, mx, radius, B, rel)
    e, m, n, nc = pk.shape[0], st.shape[0], sP.shape[0], cells.shape[1]
    start_t, perm_t, _ = M._transposed_neighbors(pk, n)
    torch.manual_seed(0)
    g = torch.rand(e, device=dev)
    si = int(bool(rel))
    # (a) per edge
    dp = torch.empty((e, 3), device=dev)
    dpts_a = torch.empty((n, 3), device=dev)
    dR_a = torch.empty(B, device=dev) if rel else None
    ws_a = torch.empty(lib.mccnn_compute_pdf_bwd_points_workspace_bytes(m, B), dtype=torch.uint8, device=dev)

    def edge_bwd():
        check(lib.mccnn_compute_pdf_bwd_points(ptr(sP), ptr(sB), ptr(st), m, ptr(pk), e, ptr(mn), ptr(mx), B, window, radius, si,
                                               ptr(g), 0, ptr(dp), ptr(dR_a), ptr(ws_a), ws_a.numel(), stream_handle()), "pdf_bwd")

    def edge_reduce():
        check(lib.mccnn_edge_grad_reduce(ptr(dp), ptr(start_t), ptr(perm_t), n, e, ptr(dpts_a), stream_handle()), "reduce")
    # (b) per point
    density = torch.empty((n, 1), device=dev)
    counts = torch.empty((n, 1), dtype=torch.int32, device=dev)
    gd = torch.empty(n, device=dev)
    dpts_b = torch.empty((n, 3), device=dev)
    dR_b = torch.empty(B, device=dev) if rel else None
    ws_b = torch.empty(lib.mccnn_compute_pdf_points_bwd_workspace_bytes(n, B), dtype=torch.uint8, device=dev)

    def sweep_fwd():
        check(lib.mccnn_compute_pdf_points(ptr(sP), ptr(sB), n, ptr(cells), ptr(mn), ptr(mx), B, nc, window, radius, si,
                                           ptr(density), ptr(counts), stream_handle()), "pdf_points")

    def expand_bwd():
        check(lib.mccnn_expand_pdf_bwd(ptr(gd), ptr(g), ptr(st), m, ptr(pk), e, ptr(start_t), ptr(perm_t), n, stream_handle()),
              "expand_bwd")

    def sweep_bwd():
        check(lib.mccnn_compute_pdf_points_bwd(ptr(sP), ptr(sB), n, ptr(cells), ptr(mn), ptr(mx), B, nc, window, radius, si,
                                               ptr(gd), ptr(dpts_b), ptr(dR_b), ptr(ws_b), ws_b.numel(), stream_handle()),
              "pdf_points_bwd")
    expand_bwd()
    ta, tr = timed(edge_bwd), timed(edge_reduce)
    tf, te, tb = timed(sweep_fwd), timed(expand_bwd), timed(sweep_bwd)
    k = torch.diff(torch.cat([st.view(-1).long(), torch.tensor([e], device=dev)]))
    print("%-7s n %d  m %d  E %d  sum k^2 %.3g  mean own ball %.1f  dR %s" % (
        name, n, m, e, float((k.double() ** 2).sum()), float(counts.double().mean()), "yes" if rel else "no"))
    print("   (a)  compute_pdf_bwd_points    ms %.4f (worst of 5: %.4f)" % ta)
    print("        edge_grad_reduce          ms %.4f (worst of 5: %.4f)   per-edge backward %.4f" % (tr + (ta[0] + tr[0],)))
    print("   (b)  expand_pdf_bwd            ms %.4f (worst of 5: %.4f)" % te)
    print("        compute_pdf_points_bwd    ms %.4f (worst of 5: %.4f)   per-point backward %.4f" % (tb + (te[0] + tb[0],)))
    print("        compute_pdf_points (fwd)  ms %.4f (worst of 5: %.4f)   backward sweep / forward sweep %.2f" % (
        tf + (tb[0] / tf[0],)))
    print("        (a) / (b) %.1f" % ((ta[0] + tr[0]) / (te[0] + tb[0])))


def main():
    which = sys.argv[1:] or ["room", "pool_1"]
    dev = torch.device("cuda", 0)
    if "room" in which:
        P = torch.from_numpy(W.make_room(100000, 20180601)).to(dev)
        Bi = torch.zeros((P.shape[0], 1), dtype=torch.int32, device=dev)
        mn, mx = M.compute_aabb(P, Bi, 1, False)
        case("room", P, Bi, P, Bi, mn, mx, 1, 0.1, False, 0.2)
    if "pool_1" in which:
        cfg = W.CONFIGS["cfg2"]
        pts, bids, B = W.config_points(cfg)
        P, Bi = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev)
        ph = PointHierarchy(P, torch.ones((P.shape[0], 1), device=dev), Bi, cfg.hierarchy, "PH", B, cfg.relative)
        conv = [c for c in cfg.convs if c.name == "Pool_1"][0]
        case("pool_1", ph.points_[conv.lin], ph.batchIds_[conv.lin], ph.points_[conv.lout], ph.batchIds_[conv.lout], ph.aabbMin_,
             ph.aabbMax_, B, conv.radius, cfg.relative, conv.window)


if __name__ == "__main__":
    main()
