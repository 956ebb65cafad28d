"""Backward pass of Fin = 1 combin layers: the one-wave-per-slice edge kernel (mccnn_debug_conv_impl bit 2) against the
cooperative one (bit 3) in ONE process, alternating, per block count and list: python tools/f1_coop_ab.py [rounds]
ms per backward call (centre pass + edge pass + reduce; HIP events, 20 calls per figure), chunks per resident workgroup
of the cooperative form beside it (the quantity the dispatch rule f1_coop_min_chunks tests)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mccnn_amd import MCConvModule as mc, _lib  # noqa: E402
from mccnn_amd.workloads import CONFIGS, config_points, make_room  # noqa: E402
from tests.helpers import make_mlp  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
cus = torch.cuda.get_device_properties(0).multi_processor_count
LISTS = ((100000, 0.1, 1), (100000, 0.1, 8), (100000, 0.05, 1), (20000, 0.1, 1), (5000, 0.1, 1), ("cfg2", 0.1, 1), ("cfg3", 0.03, 1))
if os.environ.get("LISTS"):  # a subset, by position
    LISTS = tuple(LISTS[int(i)] for i in os.environ["LISTS"].split(","))
for n_pts, radius, rooms in LISTS:
    rel, B = False, 1
    if isinstance(n_pts, str):  # a batch of small clouds, radius relative to each cloud's box
        pts, bids, B = config_points(CONFIGS[n_pts])
        rel = True
    else:
        # (rooms on a 2 x 2 x 2 lattice: in a row the box of 8 rooms has more cells than 32-bit keys hold)
        pts = np.concatenate([make_room(n_pts, 7 + k) + np.array([k & 1, (k >> 1) & 1, k >> 2], np.float32) * 20.0
                              for k in range(rooms)]).astype(np.float32)
        bids = np.zeros((len(pts), 1), np.int32)
    P, Bi = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev)
    mn, mx = mc.compute_aabb(P, Bi, B, rel)
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, B, radius, rel)
    start, packed = mc.find_neighbors(sP, sB, sP, cells, mn, mx, radius, B, rel)
    pdfs = mc.compute_pdf(sP, sB, mn, mx, start, packed, 0.25, radius, B, rel)
    E = int(packed.shape[0])
    for fout in [int(f) for f in os.environ.get("FOUTS", "16,32,64,128").split(",")]:
        nb = (fout + 7) // 8
        W = 8 if nb % 8 == 0 else 4 if nb % 4 == 0 else 2
        w = make_mlp(nb, 3)
        F = torch.rand((len(pts), 1), device=dev).requires_grad_(True)
        ws = [torch.from_numpy(w[k]).to(dev).requires_grad_(True) for k in ("w1", "w2", "w3", "b1", "b2", "b3")]
        og = torch.rand((len(pts), fout), device=dev)
        out = mc.spatial_conv(sP, F, sB, pdfs, sP, start, packed, mn, mx, *ws, fout, True, B, radius, rel, True)
        res = {4: [], 8: []}
        prev = lib.mccnn_debug_conv_impl(4)
        try:
            for _ in range(rounds):
                for mask in (4, 8):
                    lib.mccnn_debug_conv_impl(mask)
                    for _ in range(3):
                        torch.autograd.grad([out], [F] + ws, [og], retain_graph=True)
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(20):
                        torch.autograd.grad([out], [F] + ws, [og], retain_graph=True)
                    b.record()
                    b.synchronize()
                    res[mask].append(a.elapsed_time(b) / 20)
        finally:
            lib.mccnn_debug_conv_impl(prev)
        per_group = ((E + 63) // 64) / (cus * 8 // W)
        print("%s r=%g x%d: %d edges, %d blocks (W = %d, %.1f chunks per resident workgroup): slices %s ms, cooperative %s ms"
              % (n_pts, radius, rooms, E, nb, W, per_group, " ".join("%.4f" % v for v in res[4]), " ".join("%.4f" % v for v in res[8])),
              flush=True)
        del out
