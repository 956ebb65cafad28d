"""Gradients with respect to positions on the GPU (conv_points.hip): spatial_conv's point / centre / PDF / box gradients and
compute_pdf's point / box gradients against the float64 reference of tests/pointgrad_ref.py over the GPU's own discrete
structure, a builder graph end to end, the seven existing gradients unchanged, and bit-reproducibility."""
import numpy as np
import pytest

from tests import pointgrad_ref as ref
from tests.pointgrad_cases import RTOL, check_close  # noqa: F401  (the project's bar, shared with the edge tests)
from tests.helpers import make_cloud, make_mlp, run_chain
from mccnn_amd.workloads import conv_nb

pytestmark = pytest.mark.gpu


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geometry(mc, n_per, B, radius, scaleInv, seed=1, mode=None):
    pts, bids = make_cloud(n_per, B, seed, "clustered")
    f0 = np.zeros((len(pts), 1), np.float32)
    g = run_chain(mc, _wrap, lambda t: t.detach().cpu().numpy(), pts, bids, f0, B, radius, scaleInv, fout=1,
                  pdf_kwargs=None if mode is None else dict(mode=mode))
    return pts, bids, g


def _ref_grads(h, g, feats_sorted, w, og, fout, combin, B, radius, scaleInv, avg):
    import torch
    T = ref.t64
    sp = T(g["sortPts"]).requires_grad_(True)
    c = T(h["C"].detach().cpu().numpy()).requires_grad_(True)
    pd = T(h["pdfs"].detach().cpu().numpy()).requires_grad_(True)
    mn = T(g["aabbMin"]).requires_grad_(True)
    mx = T(g["aabbMax"]).requires_grad_(True)
    ws = {k: T(v) for k, v in w.items()}
    out = ref.spatial_conv(sp, T(feats_sorted), g["sortBatchs"], pd, c, g["startIndexs"], g["packedNeighs"], mn, mx,
                           ws["w1"], ws["b1"], ws["w2"], ws["b2"], ws["w3"], ws["b3"], fout, combin, B, radius, scaleInv, avg)
    (out * T(og)).sum().backward()
    return dict(pts=sp.grad.numpy(), centres=c.grad.numpy(), pdfs=pd.grad.numpy(),
                box=np.concatenate([mn.grad.numpy(), mx.grad.numpy()]) if scaleInv else None)


CASES = [  # combin, fin, fout, bf16, scaleInv, avg
    (True, 1, 64, False, True, True),     # the f1 shape
    (True, 3, 8, False, True, False),
    (True, 2, 16, False, False, True),
    (False, 16, 16, False, True, True),   # row kernels
    (False, 64, 64, False, False, False),
    (False, 32, 32, True, True, True),    # bf16 rows
    (False, 12, 12, False, True, True),   # depth-wise, Fin % 8 != 0: one whole block and one half padded
]


def _conv_call(mc, h, feats, w, fout, combin, B, radius, scaleInv, avg, grads, sortIndex=None, featIndex=None, pts=None):
    """One spatial_conv; grads=True: points, centres, PDFs and (scaleInv) box require a gradient."""
    import torch
    P = (h["sP"] if pts is None else pts).detach().clone()
    C = h["C"].detach().clone()
    pd = h["pdfs"].detach().clone()
    mn, mx = h["mn"].detach().clone(), h["mx"].detach().clone()
    if grads:
        for t in (P, C, pd) + ((mn, mx) if scaleInv else ()):
            t.requires_grad_(True)
    F = feats.detach().clone().requires_grad_(True)
    tw = {k: _wrap(v).requires_grad_(True) for k, v in w.items()}
    out = mc.spatial_conv(P, F, h["sB"] if pts is None else h["oB"], pd, C, h["start"], h["packed"], mn, mx, tw["w1"],
                          tw["w2"], tw["w3"], tw["b1"], tw["b2"], tw["b3"], fout, combin, B, radius, scaleInv, avg,
                          sortIndex=sortIndex, featIndex=featIndex)
    return out, P, C, pd, mn, mx, F, tw


@pytest.mark.parametrize("combin,fin,fout,bf16,scaleInv,avg", CASES)
def test_conv_point_grads_match_the_reference(mc, combin, fin, fout, bf16, scaleInv, avg):
    import torch
    B, radius = 2, 0.15
    pts, bids, g = _geometry(mc, 1024, B, radius, scaleInv)
    h = g["_handles"]
    rng = np.random.default_rng(fin * 100 + fout)
    fs = (2 * rng.random((len(pts), fin)) - 1).astype(np.float32)
    feats = _wrap(fs).to(torch.bfloat16) if bf16 else _wrap(fs)
    w = make_mlp(conv_nb(fin, fout, combin), 21)
    outF = fout if combin else fin
    og = (2 * rng.random((len(pts), outF)) - 1).astype(np.float32)
    ogt = _wrap(og).to(torch.bfloat16) if bf16 else _wrap(og)
    out, P, C, pd, mn, mx, F, tw = _conv_call(mc, h, feats, w, fout, combin, B, radius, scaleInv, avg, True)
    out.backward(ogt)
    torch.cuda.synchronize()
    r = _ref_grads(h, g, feats.float().cpu().numpy(), w, ogt.float().cpu().numpy(), fout, combin, B, radius, scaleInv, avg)
    check_close(P.grad.cpu().numpy(), r["pts"], "points")
    check_close(C.grad.cpu().numpy(), r["centres"], "centres")
    check_close(pd.grad.cpu().numpy(), r["pdfs"], "pdfs")
    if scaleInv:
        check_close(torch.cat([mn.grad, mx.grad]).cpu().numpy(), r["box"], "box")
    else:
        assert mn.grad is None and mx.grad is None


def test_conv_point_grads_with_sort_and_feat_index(mc):
    """The sortIndex / featIndex form (feature rows of the UNSORTED points, a small depth-wise level: read in place)."""
    import torch
    B, radius, fin, scaleInv = 2, 0.15, 16, True
    pts, bids = make_cloud(1024, B, 4, "clustered")
    P0, Bi = _wrap(pts), _wrap(bids)
    mn, mx = mc.compute_aabb(P0, Bi, B, scaleInv)
    oP, oB, cells, idx, inv = mc.build_grid(P0, Bi, mn, mx, B, radius, scaleInv)
    start, packed = mc.find_neighbors(P0, Bi, oP, cells, mn, mx, radius, B, scaleInv)
    pdfs = mc.compute_pdf(oP, oB, mn, mx, start, packed, 0.2, radius, B, scaleInv)
    h = dict(sP=oP, oB=oB, C=P0, pdfs=pdfs, mn=mn, mx=mx, start=start, packed=packed)
    rng = np.random.default_rng(8)
    fs = (2 * rng.random((len(pts), fin)) - 1).astype(np.float32)
    w = make_mlp(conv_nb(fin, fin, False), 22)
    og = (2 * rng.random((len(pts), fin)) - 1).astype(np.float32)
    out, P, C, pd, gmn, gmx, F, tw = _conv_call(mc, h, _wrap(fs), w, fin, False, B, radius, scaleInv, True, True,
                                                sortIndex=idx, featIndex=inv, pts=oP)
    out.backward(_wrap(og))
    torch.cuda.synchronize()
    g = dict(sortPts=oP.cpu().numpy(), sortBatchs=oB.cpu().numpy(), aabbMin=mn.cpu().numpy(), aabbMax=mx.cpu().numpy(),
             startIndexs=start.cpu().numpy(), packedNeighs=packed.cpu().numpy())
    r = _ref_grads(h, g, fs[inv.cpu().numpy().astype(np.int64)], w, og, fin, False, B, radius, scaleInv, True)
    check_close(P.grad.cpu().numpy(), r["pts"], "points")
    check_close(C.grad.cpu().numpy(), r["centres"], "centres")
    check_close(pd.grad.cpu().numpy(), r["pdfs"], "pdfs")
    check_close(torch.cat([gmn.grad, gmx.grad]).cpu().numpy(), r["box"], "box")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scaleInv", [True, False])
def test_pdf_point_grads_match_the_reference(mc, mode, scaleInv):
    import torch
    B, radius, window = 2, 0.15, 0.2
    pts, bids, g = _geometry(mc, 1024, B, radius, scaleInv, seed=2)
    h = g["_handles"]
    sP = h["sP"].detach().clone().requires_grad_(True)
    mn, mx = h["mn"].detach().clone(), h["mx"].detach().clone()
    if scaleInv:
        mn.requires_grad_(True)
        mx.requires_grad_(True)
    pdfs = mc.compute_pdf(sP, h["sB"], mn, mx, h["start"], h["packed"], window, radius, B, scaleInv, mode=mode)
    assert torch.equal(pdfs.detach(), mc.compute_pdf(h["sP"], h["sB"], h["mn"], h["mx"], h["start"], h["packed"], window,
                                                     radius, B, scaleInv, mode=mode))
    r = np.random.default_rng(3).random(pdfs.shape[0])
    (pdfs.view(-1) * _wrap(r.astype(np.float32))).sum().backward()
    torch.cuda.synchronize()
    T = ref.t64
    rp = T(g["sortPts"]).requires_grad_(True)
    rmn, rmx = T(g["aabbMin"]).requires_grad_(True), T(g["aabbMax"]).requires_grad_(True)
    rpdf = ref.compute_pdf(rp, g["sortBatchs"], rmn, rmx, g["startIndexs"], g["packedNeighs"], window, radius, scaleInv)
    (rpdf * T(r)).sum().backward()
    check_close(sP.grad.cpu().numpy(), rp.grad.numpy(), "points")
    if scaleInv:
        check_close(torch.cat([mn.grad, mx.grad]).cpu().numpy(), np.concatenate([rmn.grad.numpy(), rmx.grad.numpy()]), "box")


@pytest.mark.parametrize("combin,fin,fout,bf16,scaleInv,avg", CASES)
def test_existing_gradients_do_not_move(mc, combin, fin, fout, bf16, scaleInv, avg):
    """Asking for position gradients leaves the output and the seven existing gradients as they were: bitwise on the
    deterministic paths, within the 1e-4 bar on the float-atomic Fin = 1 path."""
    import torch
    B, radius = 2, 0.15
    pts, bids, g = _geometry(mc, 1024, B, radius, scaleInv, seed=5)
    h = g["_handles"]
    mc._transposed_neighbors(h["packed"], len(pts))   # the 2..4-feature combin layers then gather (deterministic)
    rng = np.random.default_rng(fin + fout)
    fs = (2 * rng.random((len(pts), fin)) - 1).astype(np.float32)
    feats = _wrap(fs).to(torch.bfloat16) if bf16 else _wrap(fs)
    w = make_mlp(conv_nb(fin, fout, combin), 23)
    outF = fout if combin else fin
    og = _wrap((2 * rng.random((len(pts), outF)) - 1).astype(np.float32))
    og = og.to(torch.bfloat16) if bf16 else og
    res = []
    for grads in (False, True):
        out, P, C, pd, mn, mx, F, tw = _conv_call(mc, h, feats, w, fout, combin, B, radius, scaleInv, avg, grads)
        out.backward(og)
        torch.cuda.synchronize()
        res.append([out.detach(), F.grad] + [tw[k].grad for k in ("w1", "b1", "w2", "b2", "w3", "b3")])
        if grads:
            assert P.grad is not None and C.grad is not None and pd.grad is not None
        else:
            assert P.grad is None
    exact = (not combin) or fin == 3
    for name, a, b in zip(("out", "features", "w1", "b1", "w2", "b2", "w3", "b3"), res[0], res[1]):
        if exact:
            assert torch.equal(a, b), name
        else:
            check_close(b.float().cpu().numpy(), a.float().cpu().numpy(), name)


@pytest.mark.parametrize("combin,fin,fout", [(True, 1, 64), (False, 16, 16)])
def test_position_gradients_are_bit_reproducible(mc, combin, fin, fout):
    import torch
    B, radius, scaleInv = 2, 0.15, True
    pts, bids, g = _geometry(mc, 1024, B, radius, scaleInv, seed=6)
    h = g["_handles"]
    rng = np.random.default_rng(9)
    feats = _wrap((2 * rng.random((len(pts), fin)) - 1).astype(np.float32))
    w = make_mlp(conv_nb(fin, fout, combin), 24)
    outF = fout if combin else fin
    og = _wrap((2 * rng.random((len(pts), outF)) - 1).astype(np.float32))
    tw = [_wrap(w[k]) for k in ("w1", "w2", "w3", "b1", "b2", "b3")]
    runs = []
    for _ in range(2):
        sP = h["sP"].detach().clone().requires_grad_(True)
        C = h["C"].detach().clone().requires_grad_(True)
        mn, mx = h["mn"].detach().clone().requires_grad_(True), h["mx"].detach().clone().requires_grad_(True)
        pdfs = mc.compute_pdf(sP, h["sB"], mn, mx, h["start"], h["packed"], 0.2, radius, B, scaleInv)
        out = mc.spatial_conv(sP, feats, h["sB"], pdfs, C, h["start"], h["packed"], mn, mx, *tw, fout, combin, B, radius,
                              scaleInv, True)
        out.backward(og)
        torch.cuda.synchronize()
        runs.append((sP.grad.clone(), C.grad.clone(), mn.grad.clone(), mx.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _builder_case(mc, relativeRadius):
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    B = 2
    pts, bids = make_cloud(2048, B, 12, "clustered")
    rng = np.random.default_rng(13)
    fs = (2 * rng.random((len(pts), 3)) - 1).astype(np.float32)
    P = _wrap(pts).requires_grad_(True)
    Bi, F = _wrap(bids), _wrap(fs)
    ph = PointHierarchy(P, F, Bi, [0.1], "PHg", B, relativeRadius)
    cb = ConvolutionBuilder(KDEWindow=0.2, relativeRadius=relativeRadius)
    specs = [  # name, inLevel, outLevel, radius, fin, fout, combin, usePDF
        ("c1", 0, 0, 0.12, 3, 8, True, True),
        ("c2", 0, 1, 0.15, 8, 8, False, True),   # pooling between levels
        ("c3", 1, 1, 0.25, 8, 16, True, False),  # usePDF=False
        ("c4", 1, 1, 0.25, 16, 16, False, True),
    ]
    state, mlps = {}, {}
    for k, (name, _, _, _, fin, fout, combin, _) in enumerate(specs):
        nb = conv_nb(fin, fout, combin)
        w = make_mlp(nb, 30 + k)
        mlps[name] = w
        state.update({name + "_weights": _wrap(w["w1"]), name + "_biases": _wrap(w["b1"]),
                      name + "_weights2": _wrap(w["w2"]).reshape(nb, 8, 8), name + "_biases2": _wrap(w["b2"]).reshape(nb, 8),
                      name + "_weights3": _wrap(w["w3"]).reshape(nb, 8, 8), name + "_biases3": _wrap(w["b3"]).reshape(nb, 8)})
    cb.load_state_dict(state)
    feats, outs = F, {}
    for name, lin, lout, radius, fin, fout, combin, usePDF in specs:
        src = F if name == "c1" else outs[{"c2": "c1", "c3": "c2", "c4": "c3"}[name]]
        outs[name] = cb.create_convolution(name, ph, lin, src, fin, radius, outPointHierarchy=ph, outPointLevel=lout,
                                           multiFeatureConv=combin, outNumFeatures=fout, usePDF=usePDF)
    r3 = (2 * rng.random(tuple(outs["c4"].shape)) - 1).astype(np.float32)
    r1 = (2 * rng.random(tuple(outs["c1"].shape)) - 1).astype(np.float32)
    loss = (outs["c4"] * _wrap(r3)).sum() + (outs["c1"] * _wrap(r1)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert P.grad is not None
    # the reference chain in float64 over the structure the GPU run produced
    T = ref.t64
    P64 = T(pts).requires_grad_(True)
    mn, mx = ref.box_of(P64, bids, B, relativeRadius)
    levels = [P64, P64[ph.sampledIndexs_[0].long().cpu()]]
    lbids = [bids, ph.batchIds_[1].cpu().numpy()]
    assert np.array_equal(ph.points_[1].detach().cpu().numpy(), levels[1].detach().numpy().astype(np.float32))
    routs = {}
    for name, lin, lout, radius, fin, fout, combin, usePDF in specs:
        kG, kN, _ = cb.__compute_dic_keys__(ph, ph, lin, lout, radius, 0.2, relativeRadius, usePDF)
        idx = cb.cacheGrids_[kG][3].long().cpu().numpy()
        inv = np.argsort(idx)
        start, packed = [t.cpu().numpy() for t in cb.cacheNeighs_[kN]]
        sp = levels[lin][torch.as_tensor(inv)]
        sb = lbids[lin].reshape(-1)[inv]
        if usePDF:
            pdfs = ref.compute_pdf(sp, sb, mn, mx, start, packed, 0.2, radius, relativeRadius)
        else:
            pdfs = torch.ones(packed.shape[0], dtype=torch.float64)
        src = T(fs) if name == "c1" else routs[{"c2": "c1", "c3": "c2", "c4": "c3"}[name]]
        w = {k: T(v) for k, v in mlps[name].items()}
        routs[name] = ref.spatial_conv(sp, src[torch.as_tensor(inv)], sb, pdfs, levels[lout], start, packed, mn, mx,
                                       w["w1"], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"], fout, combin, B, radius,
                                       relativeRadius, True)
    check_close(outs["c4"].detach().cpu().numpy(), routs["c4"].detach().numpy(), "output")
    rl = (routs["c4"] * T(r3)).sum() + (routs["c1"] * T(r1)).sum()
    rl.backward()
    check_close(P.grad.cpu().numpy(), P64.grad.numpy(), "points.grad")


@pytest.mark.parametrize("relativeRadius", [True, False])
def test_builder_point_grads_match_the_reference(mc, relativeRadius):
    _builder_case(mc, relativeRadius)
