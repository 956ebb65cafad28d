"""find_neighbors(maxNeighbors=K) on the GPU: startIndexs and packedNeighs bit for bit against the oracle's uncapped list thinned
by tests/neighbor_cap_ref.py, over geometries that reach every regime of the search kernel; the ops downstream of a capped
list against the oracle fed the same list; the builder end to end.

The geometries (tests/neighbor_cap_ref.py), measured from the oracle's lists -- tests/test_neighbor_cap_cpu.py asserts these
very figures without a GPU:

    name          centres  uncapped E  max k  empty rows  max window
    mixed            1020       28868     59          20         315   (70 windows of 257..315 points, the others <= 256)
    mid_windows      1500       99172    240           0         498   (498 of the windows hold 257..512 points)
    big_windows      3000     1032324   1015           0        1056   (1057 windows of more than 512 points)
    many_centres     5000       97982     40           0         191

Centres are never the tensor the grid was built from, so no search here gets a visiting-order hint."""
import numpy as np
import pytest

from tests import neighbor_cap_ref as ref
from tests import pointgrad_ref
from tests.pointgrad_cases import check_close
from tests.helpers import make_mlp, conv_nb, assert_float_close

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's bar for float outputs (norm-wise and per element: tests/helpers.py)
WINDOW = 0.2

_ORACLE_LISTS = {}   # geometry name -> (geometry, the oracle's uncapped chain): computed once, never modified


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _oracle_list(oracle, name):
    if name not in _ORACLE_LISTS:
        g = ref.GEOMETRIES[name]()
        _ORACLE_LISTS[name] = (g, ref.uncapped(oracle, g))
    return _ORACLE_LISTS[name]


def _gpu_grid(mc, g, scaleInv=None):
    si = g["scaleInv"] if scaleInv is None else scaleInv
    P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
    mn, mx = mc.compute_aabb(P, Bi, g["B"], si)
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, g["B"], g["radius"], si)
    return dict(P=P, Bi=Bi, mn=mn, mx=mx, sP=sP, sB=sB, cells=cells, idx=idx, C=_wrap(g["centres"]), Cb=_wrap(g["cbids"]))


def _search(mc, g, h, K, scaleInv=None):
    si = g["scaleInv"] if scaleInv is None else scaleInv
    return mc.find_neighbors(h["C"], h["Cb"], h["sP"], h["cells"], h["mn"], h["mx"], g["radius"], g["B"], si, maxNeighbors=K)


def _expect(oracle, name, K, scaleInv=None):
    """(geometry, oracle chain, expected startIndexs, expected packedNeighs); scaleInv flipped: a chain of its own."""
    g, r = _oracle_list(oracle, name)
    if scaleInv is not None and scaleInv != g["scaleInv"]:
        key = (name, scaleInv)
        if key not in _ORACLE_LISTS:
            g2 = dict(g, scaleInv=scaleInv)
            _ORACLE_LISTS[key] = (g2, ref.uncapped(oracle, g2))
        g, r = _ORACLE_LISTS[key]
    st, pk = ref.cap_list(r["startIndexs"], r["packedNeighs"], K)
    return g, r, st, pk


def _check_list(mc, oracle, name, K, scaleInv=None):
    g, r, st, pk = _expect(oracle, name, K, scaleInv)
    h = _gpu_grid(mc, g)
    assert np.array_equal(_unwrap(h["sP"]), r["sortPts"]) and np.array_equal(_unwrap(h["cells"]), r["cellIndexs"])
    got_st, got_pk = _search(mc, g, h, K)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    print(name, "K", K, "scaleInv", g["scaleInv"], "uncapped E", len(r["packedNeighs"]), "capped E", len(pk), "rows capped",
          int((k > K).sum()), "of", len(k))
    assert got_st.shape == (len(k), 1) and got_pk.shape == (len(pk), 2)
    assert np.array_equal(_unwrap(got_st), st), "startIndexs differ in %d rows" % int((_unwrap(got_st) != st).sum())
    assert np.array_equal(_unwrap(got_pk), pk), "packedNeighs differ in %d rows" % int((_unwrap(got_pk) != pk).any(axis=1).sum())
    return g, r, h, got_st, got_pk


@pytest.mark.parametrize("scaleInv", [True, False])
def test_mixed_rows(mc, oracle, scaleInv):
    """Rows under the cap, over it and empty in one list of at most 4096 centres; windows of up to 256 points and 70 of
    257..315. scaleInv off: the same clouds under the absolute radius 0.25 in the whole batch's box (extent 1.25, 4 cells
    per axis): uncapped E 29008, max k 60, 390 windows above 256 points and 24 above 512 (up to 586), which the fill pass
    searches again -- all three window regimes in one list."""
    g, r, h, st, pk = _check_list(mc, oracle, "mixed", 16, scaleInv)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    assert (k > 16).mean() >= 0.1 and (k <= 16).mean() >= 0.1 and (k[-20:] == 0).all()


@pytest.mark.parametrize("K", [32, 100])
def test_windows_of_257_to_512_points(mc, oracle, K):
    """Several segments per window, the fill pass compacts the saved hit masks."""
    g, r, h, st, pk = _check_list(mc, oracle, "mid_windows", K)
    w = ref.window_sizes(g, r)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    assert w.max() <= 512 and ((w > 256) & (k > K)).any()


@pytest.mark.parametrize("K", [64, 1])
@pytest.mark.parametrize("scaleInv", [True, False])
def test_windows_of_more_than_512_points(mc, oracle, K, scaleInv):
    """The fill pass searches these windows again: the canonical rank carries across the segments, the true row length
    comes from the workspace."""
    g, r, h, st, pk = _check_list(mc, oracle, "big_windows", K, scaleInv)
    w = ref.window_sizes(g, r)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    assert ((w > 512) & (k > 600)).any()


def test_more_than_4096_centres(mc, oracle):
    """Absolute radius, two clouds, 5000 shuffled centres that are not the gridded points (no visiting-order hint)."""
    g, r, h, st, pk = _check_list(mc, oracle, "many_centres", 24)
    assert len(g["centres"]) > 4096 and mc._order_hint(h["C"], len(g["centres"])) is None


def test_cap_that_does_not_bind(mc, oracle):
    """K = max k and K = 2^30: the bytes of maxNeighbors=0."""
    import torch
    g, r = _oracle_list(oracle, "mixed")
    h = _gpu_grid(mc, g)
    st0, pk0 = _search(mc, g, h, 0)
    assert np.array_equal(_unwrap(st0), r["startIndexs"]) and np.array_equal(_unwrap(pk0), r["packedNeighs"])
    kmax = int(ref.row_lengths(r["startIndexs"], len(r["packedNeighs"])).max())
    for K in (kmax, 1 << 30):
        st, pk = _search(mc, g, h, K)
        assert torch.equal(st, st0) and torch.equal(pk, pk0), K


def test_two_runs_give_identical_bytes(mc, oracle):
    import torch
    for name, K in (("mixed", 16), ("big_windows", 64)):
        g, r = _oracle_list(oracle, name)
        h = _gpu_grid(mc, g)
        a, b = _search(mc, g, h, K), _search(mc, g, h, K)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------- downstream of a capped list
@pytest.fixture(scope="module")
def capped_mixed(mc, oracle):
    """The mixed geometry under K = 16 on both sides: the GPU's capped list (checked against the expected one) and the
    oracle's KDE over that list."""
    g, r, st, pk = _expect(oracle, "mixed", 16)
    h = _gpu_grid(mc, g)
    h["start"], h["packed"] = _search(mc, g, h, 16)
    assert np.array_equal(_unwrap(h["start"]), st) and np.array_equal(_unwrap(h["packed"]), pk)
    pdfs = oracle.compute_pdf(r["sortPts"], r["sortBatchs"], r["aabbMin"], r["aabbMax"], st, pk, WINDOW, g["radius"], g["B"],
                              g["scaleInv"])
    return g, r, h, st, pk, pdfs


def test_compute_pdf_over_a_capped_list(mc, capped_mixed):
    g, r, h, st, pk, pdfs = capped_mixed
    for mode in (0, 1, 2):
        got = mc.compute_pdf(h["sP"], h["sB"], h["mn"], h["mx"], h["start"], h["packed"], WINDOW, g["radius"], g["B"],
                             g["scaleInv"], mode=mode)
        assert_float_close(_unwrap(got), pdfs, RTOL, "pdfs (mode %d)" % mode)


@pytest.mark.parametrize("avg", [True, False])
@pytest.mark.parametrize("fin,fout,combin", [(1, 8, True), (3, 8, True), (8, 8, False)])
def test_spatial_conv_over_a_capped_list(mc, oracle, capped_mixed, fin, fout, combin, avg):
    import torch
    g, r, h, st, pk, pdfs = capped_mixed
    B, radius, si = g["B"], g["radius"], g["scaleInv"]
    rng = np.random.default_rng(10 * fin + fout)
    feats = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)       # rows of the SORTED points
    w = make_mlp(conv_nb(fin, fout, combin), 31)
    outF = fout if combin else fin
    og = (2 * rng.random((len(g["centres"]), outF)) - 1).astype(np.float32)
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


def test_position_gradients_over_a_capped_list(mc, capped_mixed):
    """Points, centres, PDFs and the box require a gradient: the backward pass runs over the transposed list of the capped
    list. Reference: tests/pointgrad_ref.py in float64 over the same list."""
    import torch
    g, r, h, st, pk, _ = capped_mixed
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
def test_builder_with_and_without_a_cap(mc, oracle):
    """A pooling layer between the two levels of a hierarchy over the mixed clouds: ConvolutionBuilder(maxNeighbors=16)
    equals the oracle's op chain over the capped list and runs op by op; the same builder without a cap still goes
    through the native executor."""
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
    outs = {}
    for cap in (K, 0):
        cb = ConvolutionBuilder(KDEWindow=WINDOW, maxNeighbors=cap)
        cb.load_state_dict(state)
        cb.opTrace_ = []
        outs[cap] = cb.create_convolution("c", ph, 0, F, fin, radius, outPointLevel=1, multiFeatureConv=True, outNumFeatures=fout)
        kG, kN, kP = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True, cap)
        assert ("find_neighbors", kN) in cb.opTrace_ and kN in cb.cacheNeighs_
        if cap:
            assert not cb.cacheGeo_ and kN.endswith("|16") and isinstance(cb.cacheNeighs_[kN], tuple)
        elif cb.native_:
            assert kP in cb.cacheGeo_           # the native executor built and filed this geometry
        lists = tuple(_unwrap(t) for t in cb.cacheNeighs_[kN])
        # the oracle's chain over the same two levels
        c1, cb1 = _unwrap(ph.points_[1]), _unwrap(ph.batchIds_[1])
        mn, mx = oracle.compute_aabb(g["pts"], g["bids"], B, True)
        keys, idx = oracle.sort_points_step1(g["pts"], g["bids"], mn, mx, B, radius, True)
        sp, sb, sf, cells = oracle.sort_points_step2(g["pts"], g["bids"], fs, keys, idx, mn, mx, B, radius, True)
        st, pk = ref.cap_list(*oracle.find_neighbors(c1, cb1, sp, cells, mn, mx, radius, B, True), cap)
        assert np.array_equal(lists[0], st) and np.array_equal(lists[1], pk)
        pdfs = oracle.compute_pdf(sp, sb, mn, mx, st, pk, WINDOW, radius, B, True)
        want = oracle.spatial_conv(sp, sf, sb, pdfs, c1, st, pk, mn, mx, w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"],
                                   fout, True, B, radius, True, True)
        assert_float_close(_unwrap(outs[cap]), want, RTOL, "layer (cap %d)" % cap)
    assert not torch.equal(outs[K], outs[0])    # the cap binds on this level
