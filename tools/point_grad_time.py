"""Cost of the gradients with respect to positions on the headline room (100 000 points, r = 0.1, absolute radius): per layer
shape (1to64, 3to8, dw256) the existing backward of the layer (feature + six MLP gradients) beside the three new pieces --
the conv-points kernel (mccnn_spatial_conv_bwd_points, with the PDF gradient), the KDE backward
(mccnn_compute_pdf_bwd_points) and the per-point reduction (mccnn_edge_grad_reduce). Milliseconds, median of interleaved
rounds. python tools/point_grad_time.py [--rounds 7] [--iters 10]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd import MCConvModule as M, _lib  # noqa: E402
from mccnn_amd._lib import check, ptr, stream_handle  # noqa: E402
from mccnn_amd.workloads import make_room, conv_nb  # noqa: E402

SHAPES = {"1to64": (1, 64, True), "3to8": (3, 8, True), "dw256": (256, 256, False)}


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--points", type=int, default=100000)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    radius, window, B, scaleInv = 0.1, 0.2, 1, False
    P = torch.from_numpy(make_room(args.points, 20180601)).to(dev)
    Bi = torch.zeros((P.shape[0], 1), dtype=torch.int32, device=dev)
    mn, mx = M.compute_aabb(P, Bi, B, scaleInv)
    keys, idx = M.sort_points_step1(P, Bi, mn, mx, B, radius, scaleInv)
    sP, sB, _, cells = M.sort_points_step2(P, Bi, torch.zeros((P.shape[0], 1), device=dev), keys, idx, mn, mx, B, radius,
                                           scaleInv)
    st, pk = M.find_neighbors(P, Bi, sP, cells, mn, mx, radius, B, scaleInv)
    pdfs = M.compute_pdf(sP, sB, mn, mx, st, pk, window, radius, B, scaleInv)
    n, m, e = sP.shape[0], P.shape[0], pk.shape[0]
    print("room: %d points, %d edges" % (n, e))
    lib = _lib.load()
    start_t, perm_t, _ = M._transposed_neighbors(pk, n)
    dp = torch.empty((e, 3), device=dev)
    dpts = torch.empty((n, 3), device=dev)
    gpdf = torch.rand((e, 1), device=dev)
    ws = torch.empty(lib.mccnn_compute_pdf_bwd_points_workspace_bytes(m, B), dtype=torch.uint8, device=dev)

    def pdf_bwd():
        check(lib.mccnn_compute_pdf_bwd_points(ptr(sP), ptr(sB), ptr(st), m, ptr(pk), e, ptr(mn), ptr(mx), B, window, radius,
                                               int(scaleInv), ptr(gpdf), 0, ptr(dp), None, ptr(ws), ws.numel(),
                                               stream_handle()), "pdf_bwd_points")

    def reduce():
        check(lib.mccnn_edge_grad_reduce(ptr(dp), ptr(start_t), ptr(perm_t), n, e, ptr(dpts), stream_handle()), "reduce")

    rng = np.random.default_rng(0)
    rows = {}
    for name, (fin, fout, combin) in SHAPES.items():
        nb = conv_nb(fin, fout, combin)
        w = {k: torch.from_numpy((0.5 * (2 * rng.random(s) - 1)).astype(np.float32)).to(dev).requires_grad_(True)
             for k, s in (("w1", (3, 8 * nb)), ("b1", (8 * nb,)), ("w2", (8, 8 * nb)), ("b2", (8 * nb,)),
                          ("w3", (8, 8 * nb)), ("b3", (8 * nb,)))}
        F = torch.rand((n, fin), device=dev).requires_grad_(True)
        outF = fout if combin else fin
        og = torch.rand((m, outF), device=dev)
        out = M.spatial_conv(sP, F, sB, pdfs, P, st, pk, mn, mx, w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"], fout,
                             combin, B, radius, scaleInv, True)

        def existing():
            torch.autograd.backward(out, og, retain_graph=True)

        dc = torch.empty((m, 3), device=dev)
        dpdf = torch.empty((e, 1), device=dev)
        ww = {k: v.detach() for k, v in w.items()}

        def conv_points():
            check(lib.mccnn_spatial_conv_bwd_points(ptr(sP), ptr(F), 0, ptr(sB), ptr(pdfs), ptr(P), ptr(st), ptr(pk), ptr(mn),
                                                    ptr(mx), ptr(ww["w1"]), ptr(ww["b1"]), ptr(ww["w2"]), ptr(ww["b2"]),
                                                    ptr(ww["w3"]), ptr(ww["b3"]), ptr(og), n, m, e, fin, fout, int(combin), B,
                                                    radius, int(scaleInv), 1, ptr(dp), ptr(dc), ptr(dpdf), None, None, 0,
                                                    stream_handle()), "conv_bwd_points")

        fns = dict(existing_bwd=existing, conv_points=conv_points, pdf_bwd=pdf_bwd, reduce=reduce)
        t = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.iters))
        rows[name] = {k: (float(np.median(v)), float(np.min(v))) for k, v in t.items()}
        del out
        torch.cuda.synchronize()
    print("%-7s %16s %16s %16s %16s" % ("layer", "existing bwd", "conv-points", "pdf bwd", "reduce"))
    for name, r in rows.items():
        print("%-7s %s" % (name, " ".join("%7.3f (%6.3f)" % r[k] for k in ("existing_bwd", "conv_points", "pdf_bwd", "reduce"))))
    print("(ms: median (min) of %d rounds x %d calls)" % (args.rounds, args.iters))


if __name__ == "__main__":
    main()
