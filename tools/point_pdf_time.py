"""The per-point KDE (pdfMode='point': compute_pdf_points + expand_pdf) against the default-mode compute_pdf on the SAME
neighbour list: ms per call (HIP events, best and worst of five runs of 50 calls after a warm-up) on
  room    the 100k room, same-level list, absolute radius 0.1, window 0.2
  pool_1  the Pool_1 list of workloads.mcclass_h on BASELINE cfg2 (32 clouds x 4096 points, level 0 -> level 1, relative
          radius 0.2, window 0.2)
and, per case, the list's E, sum k^2 (the pair terms of the per-edge form) and the candidates the window sweep visits per
point. The density is shared by every list over the same grid and window: its time is printed apart from the expansion's."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd import MCConvModule as M
from mccnn_amd import workloads as W
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


def candidates_per_point(cells):
    """Points staged for a point's 27-cell window, averaged over the points."""
    ln = (cells[..., 1] - cells[..., 0]).double()
    pad = torch.nn.functional.pad(ln, (1, 1, 1, 1, 1, 1))
    nc = ln.shape[1]
    win = sum(pad[:, 1 + dx:1 + dx + nc, 1 + dy:1 + dy + nc, 1 + dz:1 + dz + nc]
              for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
    return float((ln * win).sum() / ln.sum())


def case(name, P, Bi, C, Cb, mn, mx, B, radius, rel, window):
    sP, sB, cells, idx, inv = M.build_grid(P, Bi, mn, mx, B, radius, rel)
    st, pk = M.find_neighbors(C, Cb, sP, cells, mn, mx, radius, B, rel)
    e, m, n = pk.shape[0], st.shape[0], sP.shape[0]
    k = torch.diff(torch.cat([st.view(-1).long(), torch.tensor([e], device=st.device)]))
    dens, cnt = M.compute_pdf_points(sP, sB, cells, mn, mx, window, radius, B, rel)
    edge = timed(lambda: M.compute_pdf(sP, sB, mn, mx, st, pk, window, radius, B, rel))
    point = timed(lambda: M.compute_pdf_points(sP, sB, cells, mn, mx, window, radius, B, rel))
    expand = timed(lambda: M.expand_pdf(dens, st, pk))
    print("%-7s n %d  m %d  E %d  sum k^2 %.3g  mean own ball %.1f  candidates per point %.1f" % (
        name, n, m, e, float((k.double() ** 2).sum()), float(cnt.double().mean()), candidates_per_point(cells)))
    print("        compute_pdf        ms %.4f (worst of 5: %.4f)" % edge)
    print("        compute_pdf_points ms %.4f (worst of 5: %.4f)" % point)
    print("        expand_pdf         ms %.4f (worst of 5: %.4f)   points + expand %.4f" % (expand + (point[0] + expand[0],)))


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
