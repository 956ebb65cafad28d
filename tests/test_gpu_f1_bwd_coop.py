"""Backward pass of combin layers with one input feature: the cooperative edge kernel (f1_bwd_edges_coop<W>, one MLP block
per wave, the W waves of a workgroup share each 64-edge chunk) against the one-wave-per-slice kernel (f1_bwd_edges) on the
same inputs. mccnn_debug_conv_impl: bit 3 sends every even block count to the cooperative kernel whatever the list length,
bit 2 never. The forward pass is the same code in both runs."""
import numpy as np
import pytest

from tests.helpers import assert_float_close, make_cloud, make_mlp

pytestmark = pytest.mark.gpu

COOP, CHUNK = 8, 4   # mask bits 3 / 2

# name -> points per cloud, clouds, radius, relative radius, averaged, pooling, clouds of ragged sizes
LISTS = {
    "one_chunk": (8, 1, 0.5, True, False, False, False),     # 0 < E < 64: ONE partial trip of one workgroup (E = 24)
    "tiny": (30, 1, 0.5, True, False, False, False),         # 30 points, r = 0.5: the blobs make it E = 248, four chunks
    "ragged": (1500, 2, 0.15, True, True, False, False),     # 1 500 x 2: E no multiple of 64, many workgroups, a ragged last one
    "room": (4000, 1, 0.08, False, False, False, False),     # 4 000 points, absolute radius, plain sums
    "pool": (900, 3, 0.3, True, True, True, True),           # the fast-paths test's pooling list: m != n, centres without neighbours
}
# Fout -> blocks: W = 8 one sweep | W = 8 two sweeps (the per-edge sum carried between sweeps) | W = 4 | W = 2 |
# two padded neurons | odd: no cooperative form
FOUTS = (64, 128, 32, 16, 60, 24)

_geometry = {}


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _list(mc, name):
    """The neighbour list of a case, built once per session and never written to."""
    if name in _geometry:
        return _geometry[name]
    n_per, B, radius, scale_inv, avg, pool, ragged = LISTS[name]
    pts, bids = make_cloud(n_per, B, 33, "clustered", ragged)
    rng = np.random.default_rng(10)
    P, Bi = _t(pts), _t(bids)
    mn, mx = mc.compute_aabb(P, Bi, B, scale_inv)
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, B, radius, scale_inv)
    if pool:
        sel = np.sort(rng.choice(len(pts), len(pts) // 7, replace=False))
        far = np.full((5, 3), 40.0, dtype=np.float32) + rng.random((5, 3), dtype=np.float32)  # no neighbours at all
        C = _t(np.concatenate([pts[sel][:50], far[:2], pts[sel][50:], far[2:]]))
        Cb = _t(np.concatenate([bids[sel][:50], bids[:2] * 0, bids[sel][50:], bids[:3] * 0]))
    else:
        C, Cb = P, Bi
    start, packed = mc.find_neighbors(C, Cb, sP, cells, mn, mx, radius, B, scale_inv)
    pdfs = mc.compute_pdf(sP, sB, mn, mx, start, packed, 0.2, radius, B, scale_inv)
    f_np = rng.random((len(pts), 1), dtype=np.float32) - 0.3
    g = dict(B=B, radius=radius, scale_inv=scale_inv, avg=avg, sP=sP, sB=sB, C=C, start=start, packed=packed, pdfs=pdfs,
             mn=mn, mx=mx, f=f_np, n=len(pts), m=int(C.shape[0]))
    # the property each list is there for
    E = int(packed.shape[0])
    if name == "one_chunk":
        assert 0 < E < 64, E
    elif name in ("ragged", "room"):  # (a workgroup owns >= 2 chunks: more than 2 chunks are more than one workgroup)
        assert len(pts) == n_per * B and E % 64 != 0 and E > 64 * 64, (len(pts), E)
    elif name == "pool":
        st = torch_cat_starts(start, E)
        assert g["m"] != g["n"] and int((st[1:] == st[:-1]).sum()) >= 5
    else:
        assert len(pts) == n_per and E > 0
    _geometry[name] = g
    return g


def torch_cat_starts(start, E):
    import torch
    return torch.cat([start.flatten().long(), torch.tensor([E], device=start.device)])


def _run(mc, g, w, og, fout, mask):
    """spatial_conv forward + backward under one value of the implementation mask -> (out, [dF, dw1, dw2, dw3, db1, db2, db3])"""
    import torch
    from mccnn_amd import _lib
    lib = _lib.load()
    prev = lib.mccnn_debug_conv_impl(mask)
    try:
        F = _t(g["f"]).requires_grad_(True)
        ws = [_t(w[k]).requires_grad_(True) for k in ("w1", "w2", "w3", "b1", "b2", "b3")]
        out = mc.spatial_conv(g["sP"], F, g["sB"], g["pdfs"], g["C"], g["start"], g["packed"], g["mn"], g["mx"], *ws, fout,
                              True, g["B"], g["radius"], g["scale_inv"], g["avg"])
        grads = torch.autograd.grad([out], [F] + ws, [og])
        torch.cuda.synchronize()
    finally:
        was = lib.mccnn_debug_conv_impl(prev)
    assert was == mask, (was, mask)  # the library kept bits 2 / 3 through the whole call
    return out.detach(), [x.detach() for x in grads]


@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("fout", FOUTS)
def test_cooperative_backward_equals_the_slice_kernel(mc, lst, fout):
    """Forward bit-identical (same code); the feature gradient and the six parameter gradients within float summation
    order, <= 2e-5 max|g| (the bound of the four-edges-per-lane test: the two kernels add the same per-edge terms, the
    parameter sums over other slices of the list, the per-edge sum over the blocks in the same ascending order); two
    cooperative runs give bit-identical parameter gradients (fixed-order reduce, no float atomics on them). An odd block
    count has no cooperative form: both runs are the slice kernel and everything but the feature gradient (float
    atomics) is bit-identical."""
    import torch
    g = _list(mc, lst)
    nb = (fout + 7) // 8
    w = make_mlp(nb, 6)
    og = _t(np.random.default_rng(fout).random((g["m"], fout), dtype=np.float32))
    ref_out, ref = _run(mc, g, w, og, fout, CHUNK)
    got_out, got = _run(mc, g, w, og, fout, COOP)
    _, again = _run(mc, g, w, og, fout, COOP)
    assert int(g["packed"].shape[0]) > 0
    assert torch.equal(ref_out, got_out)
    names = ("featGrad", "dw1", "dw2", "dw3", "db1", "db2", "db3")
    for nm, a, b in zip(names, ref, got):
        assert bool(torch.isfinite(b).all()), nm
        err, bound = float((a - b).abs().max()), 2e-5 * max(float(a.abs().max()), 1e-20)
        print("%s %s Fout %d: max|diff| %.3g, bound %.3g" % (lst, nm, fout, err, bound))
        assert err <= bound, nm
    for nm, a, b in zip(names[1:], got[1:], again[1:]):
        assert torch.equal(a, b), nm
    if nb % 2:
        for nm, a, b in zip(names[1:], ref[1:], got[1:]):
            assert torch.equal(a, b), nm
    if fout % 8:  # padded neurons of the last block take no output gradient: their layer-3 gradients are exact zeros
        assert float(got[3].flatten()[fout * 8:].abs().max()) == 0.0 and float(got[6][fout:].abs().max()) == 0.0


def test_cooperative_backward_against_the_oracle(mc, oracle):
    """Fout = 64 (W = 8, one sweep) on the ragged list against the CPU oracle's spatial_conv and its gradients, at the parity
    suite's 1e-4 (norm-wise and per element)."""
    import torch
    from tests.oracle_ops import OracleOps
    g = _list(mc, "ragged")
    fout = 64
    w = make_mlp(8, 6)
    og_np = np.random.default_rng(fout).random((g["m"], fout), dtype=np.float32)
    out, grads = _run(mc, g, w, _t(og_np), fout, COOP)
    oo = OracleOps(oracle)
    cpu = lambda t: t.detach().cpu()
    F = torch.from_numpy(g["f"]).requires_grad_(True)
    ws = [torch.from_numpy(w[k]).requires_grad_(True) for k in ("w1", "w2", "w3", "b1", "b2", "b3")]
    ref_out = oo.spatial_conv(cpu(g["sP"]), F, cpu(g["sB"]), cpu(g["pdfs"]), cpu(g["C"]), cpu(g["start"]), cpu(g["packed"]),
                              cpu(g["mn"]), cpu(g["mx"]), *ws, fout, True, g["B"], g["radius"], g["scale_inv"], g["avg"])
    ref = torch.autograd.grad([ref_out], [F] + ws, [torch.from_numpy(og_np)])
    assert_float_close(cpu(out).numpy(), ref_out.detach().numpy(), 1e-4, "out")
    for nm, a, b in zip(("featGrad", "dw1", "dw2", "dw3", "db1", "db2", "db3"), grads, ref):
        assert_float_close(cpu(a).numpy(), b.numpy(), 1e-4, nm)
