"""find_neighbors(maxNeighbors=K, sampleSeed=s) on the GPU: startIndexs and packedNeighs bit for bit against the oracle's uncapped
list thinned by tests/neighbor_sample_ref.py, over the geometries of tests/test_gpu_neighbor_cap.py (which reach every regime of
the search kernel; tests/test_neighbor_cap_cpu.py asserts their figures without a GPU); the ops downstream of a sampled list
against the oracle fed the same list; the builder end to end.

Centres are never the tensor the grid was built from, so no search here gets a visiting-order hint."""
import zlib

import numpy as np
import pytest

from tests import neighbor_sample_ref as ref
from tests import pointgrad_ref
from tests.pointgrad_cases import check_close
from tests.helpers import make_mlp, conv_nb, assert_float_close

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's bar for float outputs (norm-wise and per element: tests/helpers.py)
WINDOW = 0.2

_ORACLE_LISTS = {}   # (geometry name, scaleInv) -> (geometry, the oracle's uncapped chain): computed once, never modified
_GRIDS = {}          # the same key -> the GPU's grid of that geometry


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _oracle_list(oracle, name, scaleInv=None):
    g = ref.GEOMETRIES[name]()
    if scaleInv is not None:
        g = dict(g, scaleInv=scaleInv)
    key = (name, g["scaleInv"])
    if key not in _ORACLE_LISTS:
        _ORACLE_LISTS[key] = (g, ref.uncapped(oracle, g))
    return _ORACLE_LISTS[key]


def _gpu_grid(mc, name, g):
    key = (name, g["scaleInv"])
    if key not in _GRIDS:
        P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
        mn, mx = mc.compute_aabb(P, Bi, g["B"], g["scaleInv"])
        sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, g["B"], g["radius"], g["scaleInv"])
        _GRIDS[key] = dict(P=P, Bi=Bi, mn=mn, mx=mx, sP=sP, sB=sB, cells=cells, idx=idx, C=_wrap(g["centres"]),
                           Cb=_wrap(g["cbids"]))
    return _GRIDS[key]


def _search(mc, g, h, K, seed):
    kw = {} if seed is None else {"sampleSeed": seed}
    return mc.find_neighbors(h["C"], h["Cb"], h["sP"], h["cells"], h["mn"], h["mx"], g["radius"], g["B"], g["scaleInv"],
                             maxNeighbors=K, **kw)


def _check_list(mc, oracle, name, K, seed, scaleInv=None):
    g, r = _oracle_list(oracle, name, scaleInv)
    st, pk = ref.sample_list(r["startIndexs"], r["packedNeighs"], K, seed)
    h = _gpu_grid(mc, name, g)
    assert np.array_equal(_unwrap(h["sP"]), r["sortPts"]) and np.array_equal(_unwrap(h["cells"]), r["cellIndexs"])
    got_st, got_pk = _search(mc, g, h, K, seed)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    print(name, "K", K, "seed", seed, "scaleInv", g["scaleInv"], "uncapped E", len(r["packedNeighs"]), "sampled E", len(pk),
          "rows sampled", int((k > K).sum()), "of", len(k))
    assert got_st.shape == (len(k), 1) and got_pk.shape == (len(pk), 2)
    assert np.array_equal(_unwrap(got_st), st), "startIndexs differ in %d rows" % int((_unwrap(got_st) != st).sum())
    assert np.array_equal(_unwrap(got_pk), pk), "packedNeighs differ in %d rows" % int((_unwrap(got_pk) != pk).any(axis=1).sum())
    return g, r, h, k


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1])
@pytest.mark.parametrize("scaleInv", [True, False])
def test_mixed_rows(mc, oracle, scaleInv, seed):
    """Rows under the cap, over it and empty in one list of at most 4096 centres. scaleInv on: windows of up to 256 points and
    70 of 257..315; off: the absolute radius 0.25 in the whole batch's box -- 390 windows above 256 points and 24 above 512
    (up to 586), which the fill pass searches again: all three window regimes in one list."""
    g, r, h, k = _check_list(mc, oracle, "mixed", 16, seed, scaleInv)
    assert (k > 16).mean() >= 0.1 and (k <= 16).mean() >= 0.1 and (k[-20:] == 0).all()
    w = ref.window_sizes(g, r)
    assert ((w <= 256) & (k > 16)).any() and ((w > 256) & (w <= 512) & (k > 16)).any()
    if not scaleInv:
        assert ((w > 512) & (k > 16)).any()


def test_windows_of_257_to_512_points(mc, oracle):
    """Several segments per window, the fill pass compacts the saved hit masks."""
    g, r, h, k = _check_list(mc, oracle, "mid_windows", 32, 3)
    w = ref.window_sizes(g, r)
    assert w.max() <= 512 and ((w > 256) & (k > 32)).any()


@pytest.mark.parametrize("K", [64, 1])
def test_windows_of_more_than_512_points(mc, oracle, K):
    """The fill pass searches these windows again: the canonical rank carries across the segments, the true row length
    (up to 1015) comes from the workspace."""
    g, r, h, k = _check_list(mc, oracle, "big_windows", K, 4)
    w = ref.window_sizes(g, r)
    assert ((w > 512) & (k > 600)).any() and k.max() == 1015


def test_more_than_4096_centres(mc, oracle):
    """Absolute radius, two clouds, 5000 shuffled centres that are not the gridded points: a scan of its own between the
    passes, and a visiting position that is not the centre's index (the hash takes the index)."""
    g, r, h, k = _check_list(mc, oracle, "many_centres", 24, 5)
    assert len(g["centres"]) > 4096 and mc._order_hint(h["C"], len(g["centres"])) is None


def test_runs_and_seeds(mc, oracle):
    """Two runs give identical bytes; seeds 1 and 2 differ (same startIndexs); without a seed the canonical capped call."""
    import torch
    for name, K in (("mixed", 16), ("big_windows", 64)):
        g, r = _oracle_list(oracle, name)
        h = _gpu_grid(mc, name, g)
        a, b, c = _search(mc, g, h, K, 1), _search(mc, g, h, K, 1), _search(mc, g, h, K, 2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0], c[0]) and a[1].shape == c[1].shape and not torch.equal(a[1], c[1])
        n, canon = _search(mc, g, h, K, None), mc.find_neighbors(h["C"], h["Cb"], h["sP"], h["cells"], h["mn"], h["mx"],
                                                                 g["radius"], g["B"], g["scaleInv"], maxNeighbors=K)
        assert torch.equal(n[0], canon[0]) and torch.equal(n[1], canon[1])
        assert torch.equal(a[0], canon[0]) and not torch.equal(a[1], canon[1])


def test_cap_that_does_not_bind(mc, oracle):
    """K = max k and K = 2^30 with a seed: the uncapped bytes."""
    g, r = _oracle_list(oracle, "mixed")
    h = _gpu_grid(mc, "mixed", g)
    kmax = int(ref.row_lengths(r["startIndexs"], len(r["packedNeighs"])).max())
    for K in (kmax, 1 << 30):
        st, pk = _search(mc, g, h, K, 11)
        assert np.array_equal(_unwrap(st), r["startIndexs"]) and np.array_equal(_unwrap(pk), r["packedNeighs"]), K


# ------------------------------------------------------------------------------------------------- downstream of a sampled list
@pytest.fixture(scope="module")
def sampled_mixed(mc, oracle):
    """The mixed geometry under K = 16 and seed 9 on both sides: the GPU's list (checked against the expected one) and the
    oracle's KDE over that list."""
    g, r = _oracle_list(oracle, "mixed")
    st, pk = ref.sample_list(r["startIndexs"], r["packedNeighs"], 16, 9)
    h = dict(_gpu_grid(mc, "mixed", g))
    h["start"], h["packed"] = _search(mc, g, h, 16, 9)
    assert np.array_equal(_unwrap(h["start"]), st) and np.array_equal(_unwrap(h["packed"]), pk)
    pdfs = oracle.compute_pdf(r["sortPts"], r["sortBatchs"], r["aabbMin"], r["aabbMax"], st, pk, WINDOW, g["radius"], g["B"],
                              g["scaleInv"])
    return g, r, h, st, pk, pdfs


def test_compute_pdf_over_a_sampled_list(mc, sampled_mixed):
    g, r, h, st, pk, pdfs = sampled_mixed
    got = mc.compute_pdf(h["sP"], h["sB"], h["mn"], h["mx"], h["start"], h["packed"], WINDOW, g["radius"], g["B"], g["scaleInv"])
    assert_float_close(_unwrap(got), pdfs, RTOL, "pdfs")


def test_spatial_conv_over_a_sampled_list(mc, oracle, sampled_mixed):
    import torch
    g, r, h, st, pk, pdfs = sampled_mixed
    B, radius, si = g["B"], g["radius"], g["scaleInv"]
    fin, fout, combin, avg = 3, 8, True, True
    rng = np.random.default_rng(10 * fin + fout)
    feats = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)       # rows of the SORTED points
    w = make_mlp(conv_nb(fin, fout, combin), 31)
    og = (2 * rng.random((len(g["centres"]), fout)) - 1).astype(np.float32)
    args = (r["sortPts"], feats, r["sortBatchs"], pdfs, g["centres"], st, pk, r["aabbMin"], r["aabbMax"], w["w1"], w["w2"],
            w["w3"], w["b1"], w["b2"], w["b3"])
    want = oracle.spatial_conv(*args, fout, combin, B, radius, si, avg)
    wg = oracle.spatial_conv_grad(*args, og, fout, combin, B, radius, si, avg)
    tw = {k: _wrap(v).requires_grad_(True) for k, v in w.items()}
    F = _wrap(feats).requires_grad_(True)
    out = mc.spatial_conv(h["sP"], F, h["sB"], _wrap(pdfs), h["C"], h["start"], h["packed"], h["mn"], h["mx"], tw["w1"],
                          tw["w2"], tw["w3"], tw["b1"], tw["b2"], tw["b3"], fout, combin, B, radius, si, avg)
    assert_float_close(_unwrap(out), want, RTOL, "spatial_conv")
    out.backward(_wrap(og))
    torch.cuda.synchronize()
    got = [F.grad, tw["w1"].grad, tw["b1"].grad, tw["w2"].grad, tw["b2"].grad, tw["w3"].grad, tw["b3"].grad]
    for nm, a, b in zip(["featGrad", "dw1", "db1", "dw2", "db2", "dw3", "db3"], got, wg):
        assert_float_close(_unwrap(a), b, RTOL, nm)


def test_position_gradients_over_a_sampled_list(mc, sampled_mixed):
    """Points, centres, PDFs and the box require a gradient: the backward pass runs over the transposed list of the sampled
    list. Reference: tests/pointgrad_ref.py in float64 over the same list."""
    import torch
    g, r, h, st, pk, _ = sampled_mixed
    B, radius, si = g["B"], g["radius"], g["scaleInv"]
    fin, fout, combin, avg = 3, 8, True, True
    rng = np.random.default_rng(77)
    feats = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)
    w = make_mlp(conv_nb(fin, fout, combin), 32)
    og = (2 * rng.random((len(g["centres"]), fout)) - 1).astype(np.float32)
    P = h["sP"].detach().clone().requires_grad_(True)
    C = h["C"].detach().clone().requires_grad_(True)
    mn, mx = h["mn"].detach().clone().requires_grad_(True), h["mx"].detach().clone().requires_grad_(True)
    pdfs = mc.compute_pdf(P, h["sB"], mn, mx, h["start"], h["packed"], WINDOW, radius, B, si)
    tw = {k: _wrap(v) for k, v in w.items()}
    out = mc.spatial_conv(P, _wrap(feats), h["sB"], pdfs, C, h["start"], h["packed"], mn, mx, tw["w1"], tw["w2"], tw["w3"],
                          tw["b1"], tw["b2"], tw["b3"], fout, combin, B, radius, si, avg)
    out.backward(_wrap(og))
    torch.cuda.synchronize()
    T = pointgrad_ref.t64
    rp, rc = T(r["sortPts"]).requires_grad_(True), T(g["centres"]).requires_grad_(True)
    rmn, rmx = T(r["aabbMin"]).requires_grad_(True), T(r["aabbMax"]).requires_grad_(True)
    rpdf = pointgrad_ref.compute_pdf(rp, r["sortBatchs"], rmn, rmx, st, pk, WINDOW, radius, si)
    ws = {k: T(v) for k, v in w.items()}
    rout = pointgrad_ref.spatial_conv(rp, T(feats), r["sortBatchs"], rpdf, rc, st, pk, rmn, rmx, ws["w1"], ws["b1"], ws["w2"],
                                      ws["b2"], ws["w3"], ws["b3"], fout, combin, B, radius, si, avg)
    (rout * T(og)).sum().backward()
    check_close(_unwrap(out), rout.detach().numpy(), "output")
    check_close(_unwrap(P.grad), rp.grad.numpy(), "points")
    check_close(_unwrap(C.grad), rc.grad.numpy(), "centres")
    check_close(_unwrap(torch.cat([mn.grad, mx.grad])), np.concatenate([rmn.grad.numpy(), rmx.grad.numpy()]), "box")


# ------------------------------------------------------------------------------------------------- the builder end to end
def test_builder_with_a_seed(mc, oracle):
    """The pooling layer of test_builder_with_and_without_a_cap under ConvolutionBuilder(maxNeighbors=16, sampleSeed=7): the
    oracle's op chain over the list sampled with the CRC-derived seed, op by op; sampleSeed_ reassigned and reset(): another
    output; the first seed again: the first output's bytes."""
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    g, _ = _oracle_list(oracle, "mixed")
    B, radius, K, fin, fout = g["B"], g["radius"], 16, 3, 8
    rng = np.random.default_rng(55)
    fs = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)
    P, Bi, F = _wrap(g["pts"]), _wrap(g["bids"]), _wrap(fs)
    ph = PointHierarchy(P, F, Bi, [0.2], "PHcap", B, True)
    w = make_mlp(conv_nb(fin, fout, True), 33)
    nb = conv_nb(fin, fout, True)
    state = {"c_weights": _wrap(w["w1"]), "c_biases": _wrap(w["b1"]), "c_weights2": _wrap(w["w2"]).reshape(nb, 8, 8),
             "c_biases2": _wrap(w["b2"]).reshape(nb, 8), "c_weights3": _wrap(w["w3"]).reshape(nb, 8, 8),
             "c_biases3": _wrap(w["b3"]).reshape(nb, 8)}
    cb = ConvolutionBuilder(KDEWindow=WINDOW, maxNeighbors=K, sampleSeed=7)
    cb.load_state_dict(state)
    layer = lambda: cb.create_convolution("c", ph, 0, F, fin, radius, outPointLevel=1, multiFeatureConv=True, outNumFeatures=fout)
    cb.opTrace_ = []
    out7 = layer()
    kG, kN0, kP0 = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True, K)
    kG, kN, kP = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True, K, 7)
    assert kN == kN0 + "|s7" and kN0.endswith("|16") and kP == kP0 + "|s7"
    assert ("find_neighbors", kN) in cb.opTrace_ and kN in cb.cacheNeighs_ and isinstance(cb.cacheNeighs_[kN], tuple)
    assert not cb.cacheGeo_                                         # the layer ran op by op
    lists = tuple(_unwrap(t) for t in cb.cacheNeighs_[kN])
    # the oracle's chain over the same two levels
    c1, cb1 = _unwrap(ph.points_[1]), _unwrap(ph.batchIds_[1])
    mn, mx = oracle.compute_aabb(g["pts"], g["bids"], B, True)
    keys, idx = oracle.sort_points_step1(g["pts"], g["bids"], mn, mx, B, radius, True)
    sp, sb, sf, cells = oracle.sort_points_step2(g["pts"], g["bids"], fs, keys, idx, mn, mx, B, radius, True)
    op_seed = (7 + zlib.crc32(kN0.encode())) & 0xFFFFFFFF
    st, pk = ref.sample_list(*oracle.find_neighbors(c1, cb1, sp, cells, mn, mx, radius, B, True), K, op_seed)
    assert np.array_equal(lists[0], st) and np.array_equal(lists[1], pk)
    pdfs = oracle.compute_pdf(sp, sb, mn, mx, st, pk, WINDOW, radius, B, True)
    want = oracle.spatial_conv(sp, sf, sb, pdfs, c1, st, pk, mn, mx, w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"],
                               fout, True, B, radius, True, True)
    assert_float_close(_unwrap(out7), want, RTOL, "layer (seed 7)")
    cb.sampleSeed_ = 8
    cb.reset()
    out8 = layer()
    assert kN0 + "|s8" in cb.cacheNeighs_ and kN not in cb.cacheNeighs_ and not cb.cacheGeo_
    assert out8.shape == out7.shape and not torch.equal(out8, out7)
    cb.sampleSeed_ = 7
    cb.reset()
    assert torch.equal(layer(), out7) and not cb.cacheGeo_
