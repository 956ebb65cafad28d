"""Position gradients of pdfMode='point' on the GPU: the sweep backward (compute_pdf_points: points and box) and the expansion
backward (expand_pdf: density) against torch float64 autograd of the DEFINITION over the oracle's rows
(tests/point_pdf_grad_ref.py -- it does not assume the symmetry the kernel uses), under the project's bar
(tests/pointgrad_cases.check_close: norm-wise and element-wise 1e-4); the forward unchanged under a gradient, two backward
passes bit for bit, and a builder graph (pointGrad=True) end to end.

Membership is exact against the oracle (the counts are bit-equal), so no pair is left out of any comparison.
Largest errors seen (MI355X): see NOTES.md, "Position gradients of the per-point KDE"."""
import numpy as np
import pytest

from tests import neighbor_cap_ref as geo
from tests import point_pdf_grad_ref as gref
from tests import point_pdf_ref as ref
from tests import pointgrad_ref as pg
from tests.pointgrad_cases import check_close, geometry
from tests.helpers import make_cloud, make_mlp
from mccnn_amd.workloads import conv_nb

pytestmark = pytest.mark.gpu

WINDOW = 0.25

_REFS = {}   # case name -> the oracle's grid, rows and reference gradients: computed once, never modified


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _weights(name, n):
    return np.random.default_rng(sum(map(ord, name))).random(n)   # upstream weights in [0, 1)


def _reference(oracle, name, pts, bids, B, radius, scaleInv, window=WINDOW):
    if name not in _REFS:
        mn, mx, sP, sB, cells, idx = ref.sorted_grid(oracle, pts, bids, B, radius, scaleInv)
        start, packed = ref.point_rows(oracle, sP, sB, cells, mn, mx, radius, B, scaleInv)
        packed = np.asarray(packed).reshape(-1, 2)
        gd = _weights(name, len(sP))
        dp, box = gref.sweep_grads(sP, sB, mn, mx, packed, window, radius, scaleInv, gd)
        counts = np.bincount(packed[:, 1], minlength=len(sP)).astype(np.int32)
        _REFS[name] = dict(mn=mn, mx=mx, sP=sP, sB=sB, cells=cells, idx=idx, packed=packed, gd=gd, dp=dp, box=box, counts=counts)
    return _REFS[name]


def _gpu_grid(mc, pts, bids, B, radius, scaleInv):
    P, Bi = _wrap(pts), _wrap(bids)
    mn, mx = mc.compute_aabb(P, Bi, B, scaleInv)
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, B, radius, scaleInv)
    return dict(mn=mn, mx=mx, sP=sP, sB=sB, cells=cells)


def _sweep(mc, h, B, radius, scaleInv, gd, window=WINDOW):
    """compute_pdf_points under a gradient and one backward pass -> (density, counts, dpts, box or None) tensors."""
    import torch
    sP = h["sP"].detach().clone().requires_grad_(True)
    mn, mx = h["mn"].detach().clone(), h["mx"].detach().clone()
    if scaleInv:
        mn.requires_grad_(True)
        mx.requires_grad_(True)
    density, counts = mc.compute_pdf_points(sP, h["sB"], h["cells"], mn, mx, window, radius, B, scaleInv)
    assert density.grad_fn is not None and not counts.requires_grad
    (density.view(-1) * _wrap(gd.astype(np.float32))).sum().backward()
    torch.cuda.synchronize()
    assert sP.grad is not None and sP.grad.shape == sP.shape and sP.grad.dtype == torch.float32
    return density.detach(), counts, sP.grad, torch.cat([mn.grad, mx.grad]) if scaleInv else None


def _check_sweep(mc, oracle, name, pts, bids, B, radius, scaleInv, window=WINDOW):
    import torch
    r = _reference(oracle, name, pts, bids, B, radius, scaleInv, window)
    h = _gpu_grid(mc, pts, bids, B, radius, scaleInv)
    assert np.array_equal(_unwrap(h["sP"]), r["sP"]) and np.array_equal(_unwrap(h["cells"]), r["cells"])
    density, counts, dpts, box = _sweep(mc, h, B, radius, scaleInv, r["gd"], window)
    # the forward under a gradient: the plain call's bytes, and the oracle's row lengths
    d0, c0 = mc.compute_pdf_points(h["sP"], h["sB"], h["cells"], h["mn"], h["mx"], window, radius, B, scaleInv)
    assert d0.grad_fn is None and torch.equal(d0, density) and torch.equal(c0, counts)
    assert np.array_equal(_unwrap(counts).reshape(-1), r["counts"])
    print("%s: n %d  max count %d  empty %d" % (name, len(pts), int(r["counts"].max()), int((r["counts"] == 0).sum())))
    check_close(_unwrap(dpts), r["dp"], name + " points")
    if scaleInv:
        check_close(_unwrap(box), r["box"], name + " box")
    return r, h, dpts, box


# ------------------------------------------------------------------------------------------------- 1. the sweep backward
@pytest.mark.parametrize("radius,scaleInv", [(0.1, False), (2.0, True)])
def test_sweep_grads_on_the_small_clouds(mc, oracle, radius, scaleInv):
    """Clouds of 37, 1 and 90 points inside every one of their balls. Under the relative radius the one-point cloud has zero
    extent: R = 0, s = inf, an empty row -- its gradient and its share of dR are exact zeros, never 0 * inf."""
    import torch
    from mccnn_amd import _lib as L
    pts, bids, B, sizes = ref.small_clouds()
    r, h, dpts, box = _check_sweep(mc, oracle, "small_%s" % scaleInv, pts, bids, B, radius, scaleInv)
    if not scaleInv:
        return
    one = _unwrap(h["sB"]).reshape(-1) == 1
    assert one.sum() == 1 and r["counts"][one][0] == 0
    g, bx = _unwrap(dpts), _unwrap(box)
    assert np.isfinite(g).all() and not g[one].any()
    assert np.isfinite(bx).all() and not bx[[1, B + 1]].any()
    # dR itself, through the C entry on NaN-poisoned outputs
    lib = L.load()
    n = len(pts)
    gd = _wrap(r["gd"].astype(np.float32))
    dp = torch.full((n, 3), float("nan"), device="cuda")
    dR = torch.full((B,), float("nan"), device="cuda")
    ws = torch.empty(lib.mccnn_compute_pdf_points_bwd_workspace_bytes(n, B), dtype=torch.uint8, device="cuda")
    L.check(lib.mccnn_compute_pdf_points_bwd(L.ptr(h["sP"]), L.ptr(h["sB"]), n, L.ptr(h["cells"]), L.ptr(h["mn"]), L.ptr(h["mx"]), B,
                                             h["cells"].shape[1], WINDOW, radius, 1, L.ptr(gd), L.ptr(dp), L.ptr(dR), L.ptr(ws),
                                             ws.numel(), L.stream_handle()), "compute_pdf_points_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dp, dpts) and np.isfinite(_unwrap(dR)).all() and float(dR[1]) == 0.0
    _, cdR = gref.closed_form(r["sP"], r["sB"], r["mn"], r["mx"], r["packed"], WINDOW, radius, True, r["gd"])
    check_close(_unwrap(dR), cdR, "dR")


@pytest.mark.parametrize("scaleInv", [True, False])
def test_sweep_grads_on_mixed(mc, oracle, scaleInv):
    """Two clouds of 700 and 300 points, radius 0.25 in both modes. Under the absolute radius 390 of the 1020 windows of
    the search geometry hold more than 256 points and 24 more than 512: several LDS segments carry gd[l]."""
    g = geo.geom_mixed()
    r, *_ = _check_sweep(mc, oracle, "mixed_%s" % scaleInv, g["pts"], g["bids"], g["B"], g["radius"], scaleInv)
    if not scaleInv:
        big = geo.window_sizes(g, dict(cellIndexs=r["cells"], aabbMin=r["mn"], aabbMax=r["mx"]))
        print("windows > 256: %d, > 512: %d of %d" % ((big > 256).sum(), (big > 512).sum(), len(big)))
        assert (big > 256).sum() == 390 and (big > 512).sum() == 24 and len(big) == 1020


def test_sweep_grads_on_mid_windows(mc, oracle):
    g = geo.geom_mid_windows()
    r, *_ = _check_sweep(mc, oracle, "mid_windows", g["pts"], g["bids"], g["B"], g["radius"], g["scaleInv"])
    assert r["counts"].max() > 200


@pytest.mark.parametrize("n,radius,scaleInv", [(8201, 0.08, False), (16390, 0.0625, True), (32771, 0.05, False)])
def test_every_group_size(mc, oracle, n, radius, scaleInv):
    """The backward follows the forward's thresholds up to four members: levels of 8192 / 16384 points and more put 2 / 4
    consecutive points on a wave (smaller ones, every case above: one; 32768 and more: still four, where the forward takes
    eight -- no threshold of its own); each N leaves the last wave's group part empty."""
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3), dtype=np.float32)
    bids = np.zeros((n, 1), np.int32)
    r, *_ = _check_sweep(mc, oracle, "group_%d" % n, pts, bids, 1, radius, scaleInv)
    assert 8 <= r["counts"].mean() <= 40


def test_coincident_points(mc, oracle):
    """200 points in one place (a second cloud gives the batch's box an extent): every pair contributes w * 0."""
    rng = np.random.default_rng(9)
    pts = np.concatenate([np.full((200, 3), 0.5, np.float32), rng.random((5, 3), dtype=np.float32) + np.float32(1.0)])
    bids = np.concatenate([np.zeros((200, 1), np.int32), np.ones((5, 1), np.int32)])
    r, h, dpts, _ = _check_sweep(mc, oracle, "coincident", pts, bids, 2, 0.1, False)
    own = _unwrap(h["sB"]).reshape(-1) == 0
    assert own.sum() == 200 and np.isfinite(_unwrap(dpts)).all() and not _unwrap(dpts)[own].any()


# ------------------------------------------------------------------------------------------------- 2. the expansion backward
def _expansion_case(oracle, name):
    key = "expand_" + name
    if key not in _REFS:
        g = geo.geom_many_centres() if name == "many_centres" else geometry(name)
        mn, mx, sP, sB, cells, idx = ref.sorted_grid(oracle, g["pts"], g["bids"], g["B"], g["radius"], g["scaleInv"])
        start, packed = oracle.find_neighbors(g["centres"], g["cbids"], sP, cells, mn, mx, g["radius"], g["B"], g["scaleInv"])
        packed = np.asarray(packed).reshape(-1, 2)
        w = _weights(key, len(packed))
        _REFS[key] = dict(g=g, sP=sP, idx=np.asarray(idx).reshape(-1).astype(np.int64), start=np.asarray(start), packed=packed,
                          w=w, gd=gref.expand_grads(len(sP), start, packed, w))
    return _REFS[key]


def _expand_backward(mc, r, density):
    import torch
    d = _wrap(density).requires_grad_(True)
    st, pk = _wrap(r["start"]), _wrap(r["packed"])
    pdfs = mc.expand_pdf(d, st, pk)
    assert pdfs.grad_fn is not None and torch.equal(pdfs.detach(), mc.expand_pdf(d.detach(), st, pk))
    (pdfs.view(-1) * _wrap(r["w"].astype(np.float32))).sum().backward()
    torch.cuda.synchronize()
    assert d.grad.shape == d.shape and d.grad.dtype == torch.float32
    return d.grad


@pytest.mark.parametrize("name", ["many_centres", "B"])
def test_expansion_grads(mc, oracle, name):
    """many_centres: shuffled centres, 5000 of 6000 points. B: 12 clouds, 2 of them empty, per cloud 3 lonely points that
    nobody reaches (their gd is exactly 0.f) and 2 far centres whose rows are empty."""
    r = _expansion_case(oracle, name)
    n, m, e = len(r["sP"]), len(r["start"]), len(r["packed"])
    k = ref.row_lengths(r["start"], e)
    indeg = np.bincount(r["packed"][:, 0], minlength=n)
    density = (0.5 + np.random.default_rng(n).random((n, 1))).astype(np.float32)
    gd = _unwrap(_expand_backward(mc, r, density)).reshape(-1)
    print("%s: n %d  m %d  E %d  empty rows %d  points without an edge %d" % (name, n, m, e, (k == 0).sum(), (indeg == 0).sum()))
    check_close(gd, r["gd"], name + " density gradient")
    assert not gd[indeg == 0].any()
    if name == "many_centres":
        assert m == 5000 and n == 6000
    else:
        g = r["g"]
        srt = np.asarray(r["sP"])
        # sorted position of every lonely point: nobody names it
        pos = [int(np.flatnonzero((srt == g["pts"][i]).all(1))[0]) for i in g["lonely"]]
        assert len(pos) == 30 and (indeg[pos] == 0).all() and not gd[pos].any()
        # the two far centres of every cloud (more than 0.5 from each of its points): empty rows
        cb_, pb_ = g["cbids"].reshape(-1), g["bids"].reshape(-1)
        reach = np.array([np.sqrt(((g["pts"][pb_ == cb_[i]].astype(np.float64) - g["centres"][i]) ** 2).sum(1)).min()
                          for i in range(m)])
        assert (reach > 0.5).sum() == 20 and not k[reach > 0.5].any()


# ------------------------------------------------------------------------------------------------- 3. reproducible
def test_two_backward_passes_give_the_same_bytes(mc, oracle):
    import torch
    g = geo.geom_mixed()
    r = _reference(oracle, "mixed_True", g["pts"], g["bids"], g["B"], g["radius"], True)
    h = _gpu_grid(mc, g["pts"], g["bids"], g["B"], g["radius"], True)
    runs = [_sweep(mc, h, g["B"], g["radius"], True, r["gd"]) for _ in range(2)]
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])
    x = _expansion_case(oracle, "many_centres")
    density = np.full((len(x["sP"]), 1), 0.75, np.float32)
    a, b = _expand_backward(mc, x, density), _expand_backward(mc, x, density)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 4. the builder
@pytest.mark.parametrize("relativeRadius", [True, False])
def test_builder_point_grads_match_the_reference(mc, relativeRadius):
    """The inputs and the reference treatment of tests/test_gpu_point_grads.py's builder test, in pdfMode='point' with
    pointGrad=True: c1 (same level) and c2 (pooling) read ONE density of level 0, so autograd sums two expansions into one
    sweep; c4 reads level 1's. P.grad against the float64 chain (density -> expand -> spatial_conv) over the structure the
    GPU run produced. Without the flag: today's error."""
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    from mccnn_amd.MCConvModule import InvalidArgumentError
    B, window = 2, 0.2
    pts, bids = make_cloud(2048, B, 12, "clustered")
    rng = np.random.default_rng(13)
    fs = (2 * rng.random((len(pts), 3)) - 1).astype(np.float32)
    P = _wrap(pts).requires_grad_(True)
    Bi, F = _wrap(bids), _wrap(fs)
    ph = PointHierarchy(P, F, Bi, [0.1], "PHg", B, relativeRadius)
    with pytest.raises(InvalidArgumentError, match="gradient"):
        ConvolutionBuilder(KDEWindow=window, relativeRadius=relativeRadius, pdfMode='point').create_convolution(
            "c1", ph, 0, F, 3, 0.12, outNumFeatures=8, multiFeatureConv=True)
    cb = ConvolutionBuilder(KDEWindow=window, relativeRadius=relativeRadius, pdfMode='point', pointGrad=True)
    cb.opTrace_ = []
    specs = [  # name, inLevel, outLevel, radius, fin, fout, combin, usePDF
        ("c1", 0, 0, 0.12, 3, 8, True, True),
        ("c2", 0, 1, 0.12, 8, 8, False, True),   # pooling between levels, over c1's grid: the same density
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
    outs = {}
    prev = {"c2": "c1", "c3": "c2", "c4": "c3"}
    for name, lin, lout, radius, fin, fout, combin, usePDF in specs:
        src = F if name == "c1" else outs[prev[name]]
        outs[name] = cb.create_convolution(name, ph, lin, src, fin, radius, outPointHierarchy=ph, outPointLevel=lout,
                                           multiFeatureConv=combin, outNumFeatures=fout, usePDF=usePDF)
    ops = [t[0] for t in cb.opTrace_]
    assert ops.count("compute_pdf_points") == 2 and ops.count("expand_pdf") == 3 and ops.count("compute_pdf") == 0
    assert len(cb.cachePointPDFs_) == 2 and not cb.cacheGeo_
    assert all(d.grad_fn is not None and not c.requires_grad for d, c in cb.cachePointPDFs_.values())
    r3 = (2 * rng.random(tuple(outs["c4"].shape)) - 1).astype(np.float32)
    r1 = (2 * rng.random(tuple(outs["c1"].shape)) - 1).astype(np.float32)
    loss = (outs["c4"] * _wrap(r3)).sum() + (outs["c1"] * _wrap(r1)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert P.grad is not None
    # the reference chain in float64 over the structure the GPU run produced
    T = pg.t64
    P64 = T(pts).requires_grad_(True)
    mn, mx = pg.box_of(P64, bids, B, relativeRadius)
    levels = [P64, P64[ph.sampledIndexs_[0].long().cpu()]]
    lbids = [bids, ph.batchIds_[1].cpu().numpy()]
    assert np.array_equal(ph.points_[1].detach().cpu().numpy(), levels[1].detach().numpy().astype(np.float32))
    routs, dens = {}, {}
    for name, lin, lout, radius, fin, fout, combin, usePDF in specs:
        kG, kN, _ = cb.__compute_dic_keys__(ph, ph, lin, lout, radius, window, relativeRadius, usePDF)
        grid = cb.cacheGrids_[kG]
        idx = grid[3].long().cpu().numpy()
        inv = np.argsort(idx)
        start, packed = [t.cpu().numpy() for t in cb.cacheNeighs_[kN]]
        sp = levels[lin][torch.as_tensor(inv)]
        sb = lbids[lin].reshape(-1)[inv]
        assert np.array_equal(grid[0].detach().cpu().numpy(), sp.detach().numpy().astype(np.float32))
        if usePDF:
            if kG not in dens:   # the rows of the grid's points over themselves, from the GPU's own search
                _, own = mc.find_neighbors(grid[0].detach(), grid[1], grid[0].detach(), grid[2], ph.aabbMin_.detach(),
                                           ph.aabbMax_.detach(), radius, B, relativeRadius)
                dens[kG] = gref.density(sp, sb, mn, mx, own.cpu().numpy(), window, radius, relativeRadius)
            pdfs = gref.expand(dens[kG], start, packed)
        else:
            pdfs = torch.ones(packed.shape[0], dtype=torch.float64)
        src = T(fs) if name == "c1" else routs[prev[name]]
        w = {k: T(v) for k, v in mlps[name].items()}
        routs[name] = pg.spatial_conv(sp, src[torch.as_tensor(inv)], sb, pdfs, levels[lout], start, packed, mn, mx,
                                      w["w1"], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"], fout, combin, B, radius,
                                      relativeRadius, True)
    assert len(dens) == 2
    check_close(outs["c4"].detach().cpu().numpy(), routs["c4"].detach().numpy(), "output")
    rl = (routs["c4"] * T(r3)).sum() + (routs["c1"] * T(r1)).sum()
    rl.backward()
    check_close(P.grad.cpu().numpy(), P64.grad.numpy(), "points.grad")
