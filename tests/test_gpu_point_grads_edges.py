"""Position gradients (conv_points.hip) on the geometries of tests/pointgrad_cases.py: long KDE rows (second 256-slot
pass, second and partial LDS tile), empty rows, points nobody reaches, empty clouds, box ties, a translated batch and two
rooms, over every layer shape of mccnn_spatial_conv_bwd. The C-ABI entries are called through _lib, so the per-edge
outputs are compared with the float64 per-edge reference of tests/pointgrad_ref.py:
  - per-edge dp on unambiguous edges; dpdf and the KDE's dp on all edges (no ReLU there);
  - the sums (dc, dpts after mccnn_edge_grad_reduce, dR) against a hybrid sum: the reference's per-edge values on
    unambiguous edges, the kernel's own on ambiguous ones;
  - ambiguous edges with at most 3 ambiguous neurons: the kernel's dp is the reference's under one of the 2^a masks.
Outputs are poisoned with NaN first. Bar: check_close (norm-wise and element-wise 1e-4) against float64."""
import itertools

import numpy as np
import pytest

from tests import pointgrad_cases as pc
from tests import pointgrad_ref as ref
from mccnn_amd.workloads import conv_nb

pytestmark = pytest.mark.gpu

check_close = pc.check_close
INT_KEYS = ("keys", "indexs", "sortBatchs", "cellIndexs", "startIndexs", "packedNeighs")


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().float().cpu().numpy()


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def chains(mc, oracle):
    """name -> (geometry, oracle chain, GPU handles); the GPU's integers must be the oracle's."""
    cache = {}

    def get(name):
        if name not in cache:
            g = pc.geometry(name)
            o = pc.build(g, oracle, lambda a: a, lambda a: a)
            gg = pc.build(g, mc, _wrap, lambda t: t.detach().cpu().numpy())
            for k in INT_KEYS:
                assert np.array_equal(np.asarray(gg[k]).reshape(-1), np.asarray(o[k]).reshape(-1)), (name, k)
            assert np.array_equal(gg["sortPts"], o["sortPts"]) and np.array_equal(gg["aabbMin"], o["aabbMin"])
            o["pdfs_gpu"] = gg["pdfs"].reshape(-1)
            cache[name] = (g, o, gg["_handles"])
        return cache[name]
    return get


def _lib():
    from mccnn_amd import _lib as L
    return L


def _transposed(mc, h, n):
    start_t, perm_t, _ = mc._transposed_neighbors(h["packed"], n)
    return start_t, perm_t


def _reduce(mc, h, dp, n, e):
    import torch
    L = _lib()
    start_t, perm_t = _transposed(mc, h, n)
    out = _nan(n, 3)
    L.check(L.load().mccnn_edge_grad_reduce(L.ptr(dp), L.ptr(start_t), L.ptr(perm_t), n, e, L.ptr(out), L.stream_handle()),
            "edge_grad_reduce")
    torch.cuda.synchronize()
    return _np(out)


def _conv_abi(mc, g, h, feats, og, w, shape, avg):
    """mccnn_spatial_conv_bwd_points + mccnn_edge_grad_reduce on NaN-poisoned outputs -> numpy dict."""
    import torch
    L = _lib()
    lib = L.load()
    combin, fin, fout, bf16 = shape
    n, m, e, B = h["sP"].shape[0], h["C"].shape[0], h["packed"].shape[0], g["B"]
    dp, dc, dpdf = _nan(max(e, 1), 3), _nan(m, 3), _nan(max(e, 1))
    dR = _nan(B) if g["scaleInv"] else None
    ws = torch.empty(lib.mccnn_spatial_conv_bwd_points_workspace_bytes(m, B), dtype=torch.uint8, device="cuda")
    tw = [_wrap(np.asarray(w[k], np.float32).reshape(-1)) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    C = h["C"].contiguous()
    L.check(lib.mccnn_spatial_conv_bwd_points(
        L.ptr(h["sP"]), L.ptr(feats), int(bf16), L.ptr(h["sB"]), L.ptr(h["pdfs"]), L.ptr(C), L.ptr(h["start"]),
        L.ptr(h["packed"]), L.ptr(h["mn"]), L.ptr(h["mx"]), *[L.ptr(t) for t in tw], L.ptr(og), n, m, e, fin,
        fout if combin else fin, int(combin), B, float(g["radius"]), int(g["scaleInv"]), int(avg), L.ptr(dp), L.ptr(dc),
        L.ptr(dpdf), L.ptr(dR), L.ptr(ws), ws.numel(), L.stream_handle()), "spatial_conv_bwd_points")
    torch.cuda.synchronize()
    out = dict(dp=_np(dp)[:e], dc=_np(dc), dpdf=_np(dpdf)[:e], dR=None if dR is None else _np(dR))
    out["dpts"] = _reduce(mc, h, dp, n, e)
    return out


def _pdf_abi(mc, g, h, gpdf, accumulate=0, prefill=None, want_dR=True):
    import torch
    L = _lib()
    lib = L.load()
    m, e, B = h["start"].shape[0], h["packed"].shape[0], g["B"]
    dp = _nan(max(e, 1), 3) if prefill is None else _wrap(prefill).clone()
    dR = _nan(B) if (g["scaleInv"] and want_dR) else None
    ws = torch.empty(lib.mccnn_compute_pdf_bwd_points_workspace_bytes(m, B), dtype=torch.uint8, device="cuda")
    gp = _wrap(np.asarray(gpdf, np.float32))
    L.check(lib.mccnn_compute_pdf_bwd_points(
        L.ptr(h["sP"]), L.ptr(h["sB"]), L.ptr(h["start"]), m, L.ptr(h["packed"]), e, L.ptr(h["mn"]), L.ptr(h["mx"]), B,
        pc.WINDOW, float(g["radius"]), int(g["scaleInv"]), L.ptr(gp), int(accumulate), L.ptr(dp), L.ptr(dR), L.ptr(ws),
        ws.numel(), L.stream_handle()), "compute_pdf_bwd_points")
    torch.cuda.synchronize()
    return dp, (None if dR is None else _np(dR))


def _check_dR(got, per_edge, o, g, what):
    """dR against the float64 sum of per-row terms, after asserting that a plain float32 summation of those terms in row
    order meets the same bar (dR is a signed sum over a batch: it may cancel)."""
    rows = pc.per_row(per_edge, o)
    rb = pc.row_batch(o, g)
    want = np.array([rows[rb == b].sum() for b in range(g["B"])])
    check_close(pc.batch_sums_f32(rows, rb, g["B"]), want, what + " (precondition: f32 row-order sum)")
    check_close(got, want, what)
    for b in pc.EMPTY_CLOUDS if g["B"] == 12 else ():
        assert got[b] == 0.0, (what, b)


def _structure(o):
    return pc.row_lengths(o), pc.in_degree(o)


# ---------------------------------------------------------------------------------------------- the conv's C-ABI entry
CONV_CASES = [(name, s, avg) for name in ("A_abs", "A_rel", "B", "D") for s in pc.SHAPES for avg in (True, False)]
CONV_CASES += [("E", (False, 16, 16, False), avg) for avg in (True, False)]


def _inputs(o, shape, seed):
    import torch
    combin, fin, fout, bf16 = shape
    rng = np.random.default_rng(seed)
    n, m = len(o["sortPts"]), len(o["startIndexs"])
    fs = (2 * rng.random((n, fin)) - 1).astype(np.float32)
    og = (2 * rng.random((m, fout if combin else fin)) - 1).astype(np.float32)
    feats = _wrap(fs).to(torch.bfloat16) if bf16 else _wrap(fs)
    return feats, _np(feats), _wrap(og), og


@pytest.mark.parametrize("name,shape,avg", CONV_CASES,
                         ids=["%s-%s-%s" % (n, pc.shape_id(s), "avg" if a else "sum") for n, s, a in CONV_CASES])
def test_conv_points_abi_per_edge(mc, chains, name, shape, avg):
    g, o, h = chains(name)
    combin, fin, fout, bf16 = shape
    feats, f64_feats, og_t, og = _inputs(o, shape, 17 * fin + fout)
    w = pc.mlp_for(shape)
    got = _conv_abi(mc, g, h, feats, og_t, w, shape, avg)
    for k in ("dp", "dc", "dpdf", "dpts"):
        assert np.isfinite(got[k]).all(), k
    C = pc.centres_of(g)
    args = (o["sortPts"], f64_feats, o["sortBatchs"], o["pdfs_gpu"], C, o["startIndexs"], o["packedNeighs"], o["aabbMin"],
            o["aabbMax"], w, og, fout, combin, g["radius"], g["scaleInv"], avg)
    r = ref.conv_edge_grads(*args)
    e = len(o["packedNeighs"])
    amb = pc.ambiguity(g, o, shape)
    amb_e = np.unique(amb[:, 0])
    share = len(amb_e) / e
    print("\n%s %s avg=%d: E = %d, ambiguous edges %d (%.3f %%)" % (name, pc.shape_id(shape), avg, e, len(amb_e), 100 * share))
    assert share <= pc.AMBIGUITY_CAP
    un = np.ones(e, bool)
    un[amb_e] = False
    check_close(got["dp"][un], r["dp"][un], "dp (unambiguous edges)")
    check_close(got["dpdf"], r["dpdf"], "dpdf")
    # hybrid per-edge values
    dp_h, dc_h, dR_h = r["dp"].copy(), r["dc"].copy(), r["dR"].copy()
    dp_h[amb_e] = got["dp"][amb_e]
    dc_h[amb_e] = -got["dp"][amb_e]
    dR_h[amb_e] = -(got["dp"][amb_e].astype(np.float64) * r["delta"][amb_e]).sum(1)
    j, i = o["packedNeighs"][:, 0], o["packedNeighs"][:, 1]
    deg, tdeg = _structure(o)
    dc_want = np.stack([np.bincount(i, weights=dc_h[:, d], minlength=len(C)) for d in range(3)], 1)
    dpts_want = np.stack([np.bincount(j, weights=dp_h[:, d], minlength=len(o["sortPts"])) for d in range(3)], 1)
    check_close(got["dc"], dc_want, "dc (hybrid)")
    check_close(got["dpts"], dpts_want, "dpts (hybrid)")
    assert (got["dc"][deg == 0] == 0).all() and (deg == 0).sum() >= (4 if name != "E" else 0)
    assert (got["dpts"][tdeg == 0] == 0).all()
    if g["scaleInv"]:
        _check_dR(got["dR"], dR_h, o, g, "dR (hybrid)")
    # ambiguous edges: the kernel's dp is the reference's under one of the 2^a masks
    scale = float(np.abs(r["dp"]).max())
    worst = 0.0
    edges, f1, f2, owner, n_rep = [], ([], [], []), ([], [], []), [], 0
    for ed in amb_e:
        pairs = amb[amb[:, 0] == ed]
        if len(pairs) > 3:
            continue
        for bits in itertools.product((0.0, 1.0), repeat=len(pairs)):
            for (_, layer, nu), v in zip(pairs, bits):
                f = f1 if layer == 1 else f2
                f[0].append(n_rep)
                f[1].append(nu)
                f[2].append(v)
            edges.append(ed)
            owner.append(ed)
            n_rep += 1
    if edges:
        rr = ref.conv_edge_grads(*args, edges=np.array(edges), force={1: f1, 2: f2})
        owner = np.array(owner)
        for ed in np.unique(owner):
            d = np.abs(rr["dp"][owner == ed] - got["dp"][ed]).max(1).min() / scale
            worst = max(worst, d)
            assert d <= pc.RTOL, (name, int(ed), d)
    print("  ambiguous edges checked under their masks: %d, worst element-wise %.3e" % (len(np.unique(owner)) if edges else 0,
                                                                                      worst))


# ---------------------------------------------------------------------------------------------- the KDE's C-ABI entry
@pytest.mark.parametrize("name", ["A_abs", "A_rel", "B", "D", "E"])
def test_pdf_points_abi_per_edge(mc, chains, name):
    g, o, h = chains(name)
    e, n = len(o["packedNeighs"]), len(o["sortPts"])
    rng = np.random.default_rng(23)
    gpdf = (2 * rng.random(e) - 1).astype(np.float32)
    dp_t, dR = _pdf_abi(mc, g, h, gpdf)
    dp = _np(dp_t)[:e]
    assert np.isfinite(dp).all()
    r_dp, r_dR = ref.pdf_edge_grads(o["sortPts"], o["sortBatchs"], o["aabbMin"], o["aabbMax"], o["startIndexs"],
                                    o["packedNeighs"], pc.WINDOW, g["radius"], g["scaleInv"], gpdf)
    print("\n%s: E = %d, longest row %d" % (name, e, pc.row_lengths(o).max()))
    check_close(dp, r_dp, "kde dp")
    dpts = _reduce(mc, h, dp_t, n, e)
    j = o["packedNeighs"][:, 0]
    check_close(dpts, np.stack([np.bincount(j, weights=r_dp[:, d], minlength=n) for d in range(3)], 1), "kde dpts")
    assert (dpts[pc.in_degree(o) == 0] == 0).all()
    if g["scaleInv"]:
        _check_dR(dR, r_dR, o, g, "kde dR")
    # accumulate = 1: prefill + gradient (the same per-slot value, added once)
    pre = ((2 * rng.random((e, 3)) - 1) * np.abs(r_dp).max()).astype(np.float32)
    acc_t, _ = _pdf_abi(mc, g, h, gpdf, accumulate=1, prefill=pre, want_dR=False)
    acc = _np(acc_t)
    assert np.array_equal(acc, (pre + dp).astype(np.float32))
    check_close(acc, pre.astype(np.float64) + r_dp, "kde dp (accumulate = 1)")


# ---------------------------------------------------------------------------------------------- bits
def test_position_gradients_repeat_bit_for_bit_on_long_rows(mc, chains):
    g, o, h = chains("A_rel")
    shape = (True, 1, 64, False)
    feats, _, og_t, _ = _inputs(o, shape, 5)
    w = pc.mlp_for(shape)
    runs = [_conv_abi(mc, g, h, feats, og_t, w, shape, True) for _ in range(2)]
    for k in ("dp", "dc", "dpdf", "dR", "dpts"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    gpdf = np.random.default_rng(4).random(len(o["packedNeighs"])).astype(np.float32)
    p = [_pdf_abi(mc, g, h, gpdf) for _ in range(2)]
    assert np.array_equal(_np(p[0][0]), _np(p[1][0])) and np.array_equal(p[0][1], p[1][1])


# ---------------------------------------------------------------------------------------------- end to end (autograd)
def _box_to_points(pts, bids, mn, mx, dR, radius, B):
    """dR [B] -> per-point gradients through R_b = radius * extent along the longest axis (the lowest on a tie) and the
    box extremes (split equally among the points that attain them)."""
    out = np.zeros((len(pts), 3))
    b = bids.reshape(-1)
    ext = mx.astype(np.float64) - mn
    for k in range(B):
        sel = b == k
        if not sel.any():
            continue
        ax = int(np.argmax(ext[k]))
        for box, sign in ((mx, 1.0), (mn, -1.0)):
            hit = sel & (pts[:, ax] == box[k, ax])
            out[hit, ax] += sign * radius * dR[k] / hit.sum()
    return out


def _hybrid_chain(mc, g, o, h, shape, avg, feats, f64_feats, og_t, og, w):
    """The per-point float64 gradients of sum(out * og) through compute_aabb (scaleInv), compute_pdf and spatial_conv:
    per-edge reference values, the kernel's own per-edge dp on ambiguous edges (hybrid). -> (dpts, dcentres, dR)"""
    combin, fin, fout, _ = shape
    C = pc.centres_of(g)
    e, n = len(o["packedNeighs"]), len(o["sortPts"])
    pdf64 = ref.compute_pdf(ref.t64(o["sortPts"]), o["sortBatchs"], ref.t64(o["aabbMin"]), ref.t64(o["aabbMax"]),
                            o["startIndexs"], o["packedNeighs"], pc.WINDOW, g["radius"], g["scaleInv"],
                            pair_budget=1 << 20).numpy()
    r = ref.conv_edge_grads(o["sortPts"], f64_feats, o["sortBatchs"], pdf64, C, o["startIndexs"], o["packedNeighs"],
                            o["aabbMin"], o["aabbMax"], w, og, fout, combin, g["radius"], g["scaleInv"], avg)
    amb_e = np.unique(pc.ambiguity(g, o, shape)[:, 0])
    assert len(amb_e) <= pc.AMBIGUITY_CAP * e
    if len(amb_e):
        k = _conv_abi(mc, g, h, feats, og_t, w, shape, avg)["dp"]
        r["dp"][amb_e] = k[amb_e]
        r["dc"][amb_e] = -k[amb_e]
        r["dR"][amb_e] = -(k[amb_e].astype(np.float64) * r["delta"][amb_e]).sum(1)
    kdp, kdR = ref.pdf_edge_grads(o["sortPts"], o["sortBatchs"], o["aabbMin"], o["aabbMax"], o["startIndexs"],
                                  o["packedNeighs"], pc.WINDOW, g["radius"], g["scaleInv"], r["dpdf"])
    j, i = o["packedNeighs"][:, 0], o["packedNeighs"][:, 1]
    dp = r["dp"] + kdp
    dpts = np.stack([np.bincount(j, weights=dp[:, d], minlength=n) for d in range(3)], 1)
    dcen = np.stack([np.bincount(i, weights=r["dc"][:, d], minlength=len(C)) for d in range(3)], 1)
    dR = np.bincount(o["sortBatchs"].reshape(-1)[j], weights=r["dR"] + kdR, minlength=g["B"])
    if g["scaleInv"]:
        dpts += _box_to_points(o["sortPts"], o["sortBatchs"], o["aabbMin"], o["aabbMax"], dR, g["radius"], g["B"])
    return dpts, dcen, dR, len(amb_e)


E2E = [("A_rel", (True, 1, 64, False)), ("B", (False, 16, 16, False)), ("D", (True, 3, 8, False)),
       ("E", (False, 16, 16, False))]


@pytest.mark.parametrize("name,shape", E2E, ids=[n for n, _ in E2E])
def test_autograd_end_to_end(mc, chains, name, shape):
    import torch
    g, o, h = chains(name)
    combin, fin, fout, _ = shape
    feats, f64_feats, og_t, og = _inputs(o, shape, 31)
    w = pc.mlp_for(shape)
    sP = h["sP"].detach().clone().requires_grad_(True)
    C = h["C"].detach().clone().requires_grad_(True)
    B = g["B"]
    if g["scaleInv"]:
        mn, mx = mc.compute_aabb(sP, h["sB"], B, True)
        mn.retain_grad()
        mx.retain_grad()
        assert torch.equal(mn.detach(), h["mn"]) and torch.equal(mx.detach(), h["mx"])
    else:
        mn, mx = h["mn"], h["mx"]
    pdfs = mc.compute_pdf(sP, h["sB"], mn, mx, h["start"], h["packed"], pc.WINDOW, g["radius"], B, g["scaleInv"])
    tw = {k: _wrap(v) for k, v in w.items()}
    out = mc.spatial_conv(sP, feats, h["sB"], pdfs, C, h["start"], h["packed"], mn, mx, tw["w1"], tw["w2"], tw["w3"],
                          tw["b1"], tw["b2"], tw["b3"], fout, combin, B, g["radius"], g["scaleInv"], True)
    out.backward(og_t)
    torch.cuda.synchronize()
    dpts, dcen, dR, n_amb = _hybrid_chain(mc, g, o, h, shape, True, feats, f64_feats, og_t, og, w)
    print("\n%s %s: ambiguous edges %d (hybridised)" % (name, pc.shape_id(shape), n_amb))
    check_close(_np(sP.grad), dpts, "points.grad")
    check_close(_np(C.grad), dcen, "centres.grad")
    if g["scaleInv"]:
        gmx = _np(mx.grad)
        assert np.isfinite(gmx).all() and np.isfinite(_np(mn.grad)).all()
        if B == 12:
            for b in pc.EMPTY_CLOUDS:
                assert (gmx[b] == 0).all() and (_np(mn.grad)[b] == 0).all()


def test_autograd_builder_on_a_quantised_cloud(mc, chains):
    """Geometry C through PointHierarchy and ConvolutionBuilder: the box is differentiated through _ComputeAabb (ties on
    every face, and equal x / y extents in cloud 1). Points that touch an ambiguous edge, and the box points of their
    cloud, are not compared."""
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    g, o, _ = chains("C")
    B, radius, shape = g["B"], g["radius"], (True, 3, 8, False)
    combin, fin, fout, _ = shape
    rng = np.random.default_rng(53)
    fs = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)
    P = _wrap(g["pts"]).requires_grad_(True)
    ph = PointHierarchy(P, _wrap(fs), _wrap(g["bids"]), [0.1], "PHq", B, True)
    cb = ConvolutionBuilder(KDEWindow=pc.WINDOW, relativeRadius=True)
    nb = conv_nb(fin, fout, combin)
    w = pc.mlp_for(shape)
    cb.load_state_dict({"q_weights": _wrap(w["w1"]), "q_biases": _wrap(w["b1"]), "q_weights2": _wrap(w["w2"]).reshape(nb, 8, 8),
                        "q_biases2": _wrap(w["b2"]).reshape(nb, 8), "q_weights3": _wrap(w["w3"]).reshape(nb, 8, 8),
                        "q_biases3": _wrap(w["b3"]).reshape(nb, 8)})
    out = cb.create_convolution("q", ph, 0, _wrap(fs), fin, radius, outPointHierarchy=ph, outPointLevel=0,
                                multiFeatureConv=combin, outNumFeatures=fout, usePDF=True)
    og = (2 * rng.random(tuple(out.shape)) - 1).astype(np.float32)
    (out * _wrap(og)).sum().backward()
    torch.cuda.synchronize()
    kG, kN, _ = cb.__compute_dic_keys__(ph, ph, 0, 0, radius, pc.WINDOW, True, True)
    start, packed = [t.cpu().numpy() for t in cb.cacheNeighs_[kN]]
    assert np.array_equal(start.reshape(-1), o["startIndexs"].reshape(-1)) and np.array_equal(packed, o["packedNeighs"])
    inv = np.argsort(cb.cacheGrids_[kG][3].long().cpu().numpy())
    assert np.array_equal(g["pts"][inv], o["sortPts"])
    # reference: sorted-order per-edge chain (the conv reads the sorted rows of the features), then back to input order
    T = ref.t64
    pdf64 = ref.compute_pdf(T(o["sortPts"]), o["sortBatchs"], T(o["aabbMin"]), T(o["aabbMax"]), o["startIndexs"],
                            o["packedNeighs"], pc.WINDOW, radius, True).numpy()
    r = ref.conv_edge_grads(o["sortPts"], fs[inv], o["sortBatchs"], pdf64, g["pts"], o["startIndexs"], o["packedNeighs"],
                            o["aabbMin"], o["aabbMax"], w, og, fout, combin, radius, True, True)
    kdp, kdR = ref.pdf_edge_grads(o["sortPts"], o["sortBatchs"], o["aabbMin"], o["aabbMax"], o["startIndexs"],
                                  o["packedNeighs"], pc.WINDOW, radius, True, r["dpdf"])
    j, i = o["packedNeighs"][:, 0], o["packedNeighs"][:, 1]
    n = len(g["pts"])
    dsorted = np.stack([np.bincount(j, weights=(r["dp"] + kdp)[:, d], minlength=n) for d in range(3)], 1)
    dR = np.bincount(o["sortBatchs"].reshape(-1)[j], weights=r["dR"] + kdR, minlength=B)
    want = np.zeros((n, 3))
    want[inv] = dsorted
    want += np.stack([np.bincount(i, weights=r["dc"][:, d], minlength=n) for d in range(3)], 1)
    want += _box_to_points(g["pts"], g["bids"], o["aabbMin"], o["aabbMax"], dR, radius, B)
    amb_e = np.unique(pc.ambiguity(g, o, shape)[:, 0])
    keep = np.ones(n, bool)
    keep[inv[j[amb_e]]] = False
    keep[i[amb_e]] = False
    for b in np.unique(o["sortBatchs"].reshape(-1)[j[amb_e]]):
        sel = g["bids"].reshape(-1) == b
        keep[sel & ((g["pts"] == o["aabbMin"][b]) | (g["pts"] == o["aabbMax"][b])).any(1)] = False
    print("\nC %s: ambiguous edges %d, points compared %d of %d" % (pc.shape_id(shape), len(amb_e), keep.sum(), n))
    assert keep.sum() >= 0.9 * n
    check_close(_np(P.grad)[keep], want[keep], "points.grad")
