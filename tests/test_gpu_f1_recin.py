"""Combin layers with one input feature over a geometry whose KDE left the per-edge records (native.build_geometry(recordsAvg=),
ConvolutionBuilder): the forward kernels read the records (f1_fwd_edges<true> / f1_fwd_edges4<true>) instead of evaluating and
storing them, the backward pass reads the same records. Against the same layer over a geometry without records -- the path of
MCCNN_DEBUG=kde_records=0 --: the forward output bit for bit, the parameter gradients bit for bit under the cooperative backward
kernel, the feature gradient (float atomics) within 2e-5. Lists: the tiny, ragged and pooling lists of
tests/test_gpu_f1_bwd_coop.py; both forward kernels (mccnn_debug_f1_x4_min_edges)."""
import numpy as np
import pytest

from tests.helpers import make_cloud, make_mlp
from tests.test_gpu_f1_bwd_coop import LISTS, COOP

pytestmark = pytest.mark.gpu

WINDOW = 0.2
_geos = {}
# a list long enough that the forward kernels' slice count is set by their occupancy, not by the list (> 2 x 256 CUs x 32 waves
# of 64-edge chunks): the two forms of a kernel differ in registers, and must still cut the same slices (same sums, same bits)
WIDE = (30000, 1, 0.1, False, True, False, False)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _inputs(name):
    """The cloud (and, pooling, the centres) of tests/test_gpu_f1_bwd_coop.py's list `name`: the same generator calls."""
    n_per, B, radius, scale_inv, avg, pool, ragged = WIDE if name == "wide" else LISTS[name]
    pts, bids = make_cloud(n_per, B, 33, "uniform" if name == "wide" else "clustered", ragged)
    rng = np.random.default_rng(10)
    if pool:
        sel = np.sort(rng.choice(len(pts), len(pts) // 7, replace=False))
        far = np.full((5, 3), 40.0, dtype=np.float32) + rng.random((5, 3), dtype=np.float32)  # no neighbours at all
        c = np.concatenate([pts[sel][:50], far[:2], pts[sel][50:], far[2:]])
        cb = np.concatenate([bids[sel][:50], bids[:2] * 0, bids[sel][50:], bids[:3] * 0])
    else:
        c, cb = pts, bids
    f = rng.random((len(pts), 1), dtype=np.float32) - 0.3
    return pts, bids, c, cb, f, B, radius, scale_inv, avg


def _geometry(mc, name, records):
    """One native geometry per (list, with / without records), built once per session and only read afterwards."""
    from mccnn_amd import native
    key = (name, records)
    if key in _geos:
        return _geos[key]
    pts, bids, c, cb, f, B, radius, scale_inv, avg = _inputs(name)
    P, Bi = _t(pts), _t(bids)
    Cn, Cb = (P, Bi) if c is pts else (_t(c.astype(np.float32)), _t(cb.astype(np.int32)))
    mn, mx = mc.compute_aabb(P, Bi, B, scale_inv)
    nc = mc._num_cells(mn, mx, B, radius, scale_inv)
    geo = native.build_geometry(P, Bi, Cn, Cb, mn, mx, B, nc, radius, scale_inv, WINDOW, True, recordsAvg=(avg if records else None))
    e = geo.edges()
    rec = geo.records()
    if records:
        assert rec is not None and rec[0] == int(avg) and rec[1].shape == (e, 4)
    else:
        assert rec is None
    if name == "pool":   # the property the list is there for: m != n, centres without neighbours
        import torch
        st = geo.neighbors()[0].flatten().long()
        k = torch.diff(torch.cat([st, torch.tensor([e], device=st.device)]))
        assert geo.m != geo.n and int((k == 0).sum()) >= 5
    if name == "wide":
        assert e > 64 * 2 * 256 * 32, e
    g = dict(geo=geo, f=f, avg=avg, e=e)
    _geos[key] = g
    return g


def _layer(g, w, og, fout, count=None):
    """forward + backward of the layer over g -> (out, [dF, dw1, dw2, dw3, db1, db2, db3])"""
    import torch
    from mccnn_amd import native, _lib
    lib = _lib.load()
    F = _t(g["f"]).requires_grad_(True)
    ws = {k: _t(w[k]).requires_grad_(True) for k in ("w1", "w2", "w3", "b1", "b2", "b3")}
    torch.cuda.synchronize()
    l0, m0 = lib.mccnn_debug_launch_count(), torch.cuda.memory_allocated()
    out = native.conv(g["geo"], F, ws["w1"], ws["b1"], ws["w2"], ws["b2"], ws["w3"], ws["b3"], fout, True, g["avg"])
    held = torch.cuda.memory_allocated() - m0      # the output and what the graph keeps for the backward pass
    grads = torch.autograd.grad([out], [F] + [ws[k] for k in ("w1", "w2", "w3", "b1", "b2", "b3")], [og])
    torch.cuda.synchronize()
    if count is not None:
        count.append((lib.mccnn_debug_launch_count() - l0, held))
    return out.detach(), [x.detach() for x in grads]


@pytest.mark.parametrize("lst,fout,x4", [(l, f, x) for l in ("tiny", "ragged", "pool") for f in (8, 64) for x in (False, True)] +
                         [("wide", 8, False), ("wide", 8, True)])
def test_layer_over_kde_records_equals_the_layer_without(mc, lst, fout, x4):
    import torch
    from mccnn_amd import _lib
    lib = _lib.load()
    off, on = _geometry(mc, lst, False), _geometry(mc, lst, True)
    assert off["e"] == on["e"] > 0
    nb = (fout + 7) // 8
    w = make_mlp(nb, 6)
    og = _t(np.random.default_rng(fout).random((on["geo"].m, fout), dtype=np.float32))
    prev_x4 = lib.mccnn_debug_f1_x4_min_edges(0 if x4 else 2 ** 31 - 1)
    prev = lib.mccnn_debug_conv_impl(COOP)     # the cooperative backward kernel wherever the block count is even
    try:
        c_off, c_on = [], []
        _layer(off, w, og, fout)                   # (the process-wide scratch buffers reach their size: not part of what is counted)
        ref_out, ref = _layer(off, w, og, fout, c_off)
        got_out, got = _layer(on, w, og, fout, c_on)
    finally:
        lib.mccnn_debug_conv_impl(prev)
        lib.mccnn_debug_f1_x4_min_edges(prev_x4)
    assert torch.equal(ref_out, got_out)
    names = ("featGrad", "dw1", "dw2", "dw3", "db1", "db2", "db3")
    for nm, a, b in zip(names, ref, got):
        assert bool(torch.isfinite(b).all()), nm
        err, bound = float((a - b).abs().max()), 2e-5 * max(float(a.abs().max()), 1e-20)
        print("%s %s Fout %d x4 %d: max|diff| %.3g, bound %.3g, equal %s" % (lst, nm, fout, x4, err, bound, torch.equal(a, b)))
        assert err <= bound, nm
        if nm != "featGrad" and nb % 2 == 0:   # the cooperative form ran: fixed-order sums over identical records
            assert torch.equal(a, b), nm
    # no launch more than the layer that keeps its own records (whose backward pass reads them from its state: neither runs
    # f1_edge_records), and the graph holds 16 bytes per edge less: the forward pass stored no records
    (l_off, held_off), (l_on, held_on) = c_off[0], c_on[0]
    print("%s Fout %d: launches %d / %d, bytes held after the forward pass %d / %d (E = %d)" % (lst, fout, l_off, l_on, held_off, held_on, on["e"]))
    assert l_on == l_off
    assert held_off - held_on >= 16 * on["e"] - 1024


def _builder_steps(mc, lst, fout, records, pipelined_steps):
    """bench.py's step over the cloud of `lst` (one level, absolute radius): a sequential step, then `pipelined_steps` steps that
    prefetch the next step's geometry before their convolution -> (outputs, gradients of the sequential step, records seen)"""
    import torch
    from mccnn_amd import native
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    pts, bids, _c, _cb, f, B, radius, _si, _avg = _inputs(lst)
    P, Bi = _t(pts), _t(bids)
    F = _t(f).requires_grad_(True)
    og = _t(np.random.default_rng(fout).random((len(pts), fout), dtype=np.float32))
    was = native._KDE_RECORDS
    native._KDE_RECORDS = bool(records)   # (the Python half of MCCNN_DEBUG=kde_records: nothing asks for records)
    try:
        ph = PointHierarchy(P, F, Bi, [], "recin_PH", B, False)
        cb = ConvolutionBuilder(KDEWindow=WINDOW, relativeRadius=False)
        torch.manual_seed(1234)
        outs, seen, grads = [], [], None
        for k in range(1 + pipelined_steps):
            cb.reset()
            F.grad = None
            for p in cb.parameters():
                p.grad = None
            if k > 0:
                cb.prefetch_geometry(ph, 0, radius, KDEWindow=WINDOW)
            out = cb.create_convolution("Conv", ph, 0, F, 1, radius, outNumFeatures=fout, multiFeatureConv=True, KDEWindow=WINDOW)
            out.backward(og)
            geo = next(iter(cb.cacheGeo_.values()))
            seen.append(geo.records() is not None)
            outs.append(out.detach().clone())
            if k == 0:
                grads = [F.grad.detach().clone()] + [p.grad.detach().clone() for p in cb.parameters()]
        torch.cuda.synchronize()
        cb.reset()
    finally:
        native._KDE_RECORDS = was
    return outs, grads, seen


@pytest.mark.parametrize("lst,fout", (("tiny", 8), ("ragged", 64)))
def test_builder_asks_for_records_and_pipelined_steps_reproduce_the_sequential_one(mc, lst, fout):
    import torch
    from mccnn_amd import native
    if not native.side_streams_available():
        pytest.skip("prefetch_geometry on the native executor needs the torch extension")
    on, g_on, seen_on = _builder_steps(mc, lst, fout, True, 3)
    off, g_off, seen_off = _builder_steps(mc, lst, fout, False, 3)
    # the inline build of the first step and every prefetched build carry records (the layer is known / was seen); none when off
    assert all(seen_on) and not any(seen_off), (seen_on, seen_off)
    for k in range(1, 4):
        assert torch.equal(on[k], on[0]) and torch.equal(off[k], off[0]), k
    assert torch.equal(on[0], off[0])
    for k, (a, b) in enumerate(zip(g_off, g_on)):
        err, bound = float((a - b).abs().max()), 2e-5 * max(float(a.abs().max()), 1e-20)
        assert err <= bound, k
