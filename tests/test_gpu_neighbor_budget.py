"""find_neighbors(maxEdges=B) on the GPU: the search picks the cap K* on the device and returns, byte for byte, the list of
find_neighbors(maxNeighbors=K*) -- checked against the oracle's uncapped list thinned in NumPy at the K* that
tests/neighbor_budget_ref.py computes from the oracle's row lengths (tests/test_neighbor_budget_cpu.py asserts that table without
a GPU), never against the code under test alone.

    geometry      centres  uncapped E   max k   selection
    mixed            1020       28868      59   one workgroup (20 empty rows; the floor, S(K*) = B - 1, the uncapped list)
    mid_windows      1500       99172     240   one workgroup
    big_windows      3000     1032324    1015   one workgroup, two levels deep
    many_centres     5000       97982      40   three chip-wide levels (5 workgroups), chained scan over 3 tiles
    tall_rows           6      273288   70000   one workgroup, rows above 2^16: all three levels, S(K*) = B exactly"""
import numpy as np
import pytest

from tests import neighbor_budget_ref as bref
from tests import neighbor_cap_ref as ref
from tests import neighbor_sample_ref as sref
from tests.helpers import make_mlp, conv_nb

pytestmark = pytest.mark.gpu

_ORACLE_LISTS = {}   # (geometry name, scaleInv) -> (geometry, the oracle's uncapped chain, row lengths): computed once, never modified


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _oracle_list(oracle, name, scaleInv=None):
    g = bref.BUDGET_GEOMETRIES[name]()
    if scaleInv is not None:
        g = dict(g, scaleInv=scaleInv)
    key = (name, g["scaleInv"])
    if key not in _ORACLE_LISTS:
        r = ref.uncapped(oracle, g)
        _ORACLE_LISTS[key] = (g, r, ref.row_lengths(r["startIndexs"], len(r["packedNeighs"])))
    return _ORACLE_LISTS[key]


def _gpu_grid(mc, g):
    P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
    mn, mx = mc.compute_aabb(P, Bi, g["B"], g["scaleInv"])
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, g["B"], g["radius"], g["scaleInv"])
    return dict(mn=mn, mx=mx, sP=sP, sB=sB, cells=cells, C=_wrap(g["centres"]), Cb=_wrap(g["cbids"]))


def _search(mc, g, h, **kw):
    return mc.find_neighbors(h["C"], h["Cb"], h["sP"], h["cells"], h["mn"], h["mx"], g["radius"], g["B"], g["scaleInv"], **kw)


def _check_budget(mc, g, r, k, h, B, K, Ku=0):
    """One budgeted search against cap_list(oracle list, K) -- K from the oracle's row lengths."""
    st, pk = ref.cap_list(r["startIndexs"], r["packedNeighs"], K)
    got_st, got_pk, got_cap = _search(mc, g, h, maxEdges=B, maxNeighbors=Ku, returnCap=True)
    print("B", B, "Ku", Ku, "K*", K, "got", int(got_cap[0]), "E", len(pk), "got", tuple(got_pk.shape))
    assert got_cap.dtype.is_floating_point is False and got_cap.is_cuda and tuple(got_cap.shape) == (1,)
    assert int(got_cap[0]) == K
    assert got_st.shape == (len(k), 1) and got_pk.shape == (len(pk), 2)
    assert len(got_pk) <= max(B, int((k > 0).sum()))
    assert np.array_equal(_unwrap(got_st), st), "startIndexs differ in %d rows" % int((_unwrap(got_st) != st).sum())
    assert np.array_equal(_unwrap(got_pk), pk), "packedNeighs differ in %d rows" % int((_unwrap(got_pk) != pk).any(axis=1).sum())
    return got_st, got_pk


@pytest.mark.parametrize("name", ["mixed", "mid_windows", "big_windows", "many_centres", "tall_rows"])
def test_every_table_row(mc, oracle, name):
    g, r, k = _oracle_list(oracle, name)
    m, E, kmax, rows = bref.TABLE[name]
    assert (len(k), int(k.sum()), int(k.max())) == (m, E, kmax)
    h = _gpu_grid(mc, g)
    assert np.array_equal(_unwrap(h["sP"]), r["sortPts"]) and np.array_equal(_unwrap(h["cells"]), r["cellIndexs"])
    for B, K, EK in rows:
        assert bref.budget_cap(k, B) == K     # (the table is the rule's, from the oracle's rows)
        _check_budget(mc, g, r, k, h, B, K)


@pytest.mark.parametrize("name", ["mixed", "tall_rows"])
def test_chip_wide_levels_on_short_lists(mc, oracle, name):
    """The three chip-wide levels (what lists of more than 4096 centres take) over lists the one-workgroup selection takes
    by default: the same caps and bytes -- on tall_rows with rows above 2^16, where every level does work."""
    from mccnn_amd import _lib
    lib = _lib.load()
    g, r, k = _oracle_list(oracle, name)
    h = _gpu_grid(mc, g)
    prev = lib.mccnn_debug_small_kernels(0)
    try:
        for B, K, EK in bref.TABLE[name][3]:
            _check_budget(mc, g, r, k, h, B, K)
    finally:
        lib.mccnn_debug_small_kernels(prev)


def test_mixed_under_the_absolute_radius(mc, oracle):
    g, r, k = _oracle_list(oracle, "mixed", scaleInv=False)
    assert int(k.sum()) == 29008
    h = _gpu_grid(mc, g)
    for B, K in ((7252, 7), (14504, 15)):
        assert bref.budget_cap(k, B) == K
        _check_budget(mc, g, r, k, h, B, K)


def test_budget_with_a_user_cap(mc, oracle):
    g, r, k = _oracle_list(oracle, "mixed")
    h = _gpu_grid(mc, g)
    for Ku, K in ((10, 10), (40, 15)):
        assert bref.budget_cap(k, 14434, Ku) == K
        _check_budget(mc, g, r, k, h, 14434, K, Ku)


@pytest.mark.parametrize("name,B,K", [("mixed", 14434, 15), ("big_windows", 258081, 237), ("tall_rows", 200000, 49999)])
def test_budget_with_a_seed(mc, oracle, name, B, K):
    """Equal to the product's find_neighbors(maxNeighbors=K*, sampleSeed=s) and to tests/neighbor_sample_ref.py's list."""
    import torch
    g, r, k = _oracle_list(oracle, name)
    assert bref.budget_cap(k, B) == K
    h = _gpu_grid(mc, g)
    seen = []
    for seed in (3, 0x9E3779B1):
        st, pk, cap = _search(mc, g, h, maxEdges=B, sampleSeed=seed, returnCap=True)
        cst, cpk = _search(mc, g, h, maxNeighbors=K, sampleSeed=seed)
        want_st, want_pk = sref.sample_list(r["startIndexs"], r["packedNeighs"], K, seed)
        assert int(cap[0]) == K
        assert torch.equal(st, cst) and torch.equal(pk, cpk)
        assert np.array_equal(_unwrap(st), want_st) and np.array_equal(_unwrap(pk), want_pk)
        seen.append(pk)
    assert not torch.equal(seen[0], seen[1])   # the seed draws


def test_two_calls_give_the_same_bytes(mc, oracle):
    import torch
    for name, B in (("mixed", 7217), ("many_centres", 48991), ("tall_rows", 270000)):
        g, r, k = _oracle_list(oracle, name)
        h = _gpu_grid(mc, g)
        a, b = _search(mc, g, h, maxEdges=B, returnCap=True), _search(mc, g, h, maxEdges=B, returnCap=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_guess_tables_do_not_leak(mc, oracle):
    """A budgeted call, then an unbudgeted and a capped one of the same shape: the uncapped list and the capped one, and
    returnCap without a budget gives maxNeighbors."""
    g, r, k = _oracle_list(oracle, "mixed")
    h = _gpu_grid(mc, g)
    _check_budget(mc, g, r, k, h, 2040, 2)
    st, pk = _search(mc, g, h)
    assert np.array_equal(_unwrap(st), r["startIndexs"]) and np.array_equal(_unwrap(pk), r["packedNeighs"])
    st, pk, cap = _search(mc, g, h, maxNeighbors=16, returnCap=True)
    want = ref.cap_list(r["startIndexs"], r["packedNeighs"], 16)
    assert np.array_equal(_unwrap(st), want[0]) and np.array_equal(_unwrap(pk), want[1]) and int(cap[0]) == 16
    _check_budget(mc, g, r, k, h, 28869, 59)
    st, pk, cap = _search(mc, g, h, returnCap=True)
    assert np.array_equal(_unwrap(pk), r["packedNeighs"]) and int(cap[0]) == 0


def test_builder_layer_with_a_budget(mc, oracle):
    """One 3 -> 8 layer over the mid_windows list (the points are their own centres), B = 49 586 -> K* = 38, against the same
    layer with maxNeighbors=38: lists, PDFs, output and all seven gradients bit for bit; chosenCaps_ holds 38. Both are
    prefetched with transposed="list" (op by op on the side stream), so the feature gradient is gathered through the
    transposed list in a fixed order and not added with float atomics."""
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    g, r, k = _oracle_list(oracle, "mid_windows")
    B, radius, fin, fout = g["B"], g["radius"], 3, 8
    assert bref.budget_cap(k, 49586) == 38
    rng = np.random.default_rng(56)
    fs = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)
    og = _wrap((2 * rng.random((len(g["pts"]), fout)) - 1).astype(np.float32))
    P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
    ph = PointHierarchy(P, _wrap(fs), Bi, [], "PHbudget", B, True)
    w = make_mlp(conv_nb(fin, fout, True), 34)
    nb = conv_nb(fin, fout, True)
    state = {"c_weights": _wrap(w["w1"]), "c_biases": _wrap(w["b1"]), "c_weights2": _wrap(w["w2"]).reshape(nb, 8, 8),
             "c_biases2": _wrap(w["b2"]).reshape(nb, 8), "c_weights3": _wrap(w["w3"]).reshape(nb, 8, 8),
             "c_biases3": _wrap(w["b3"]).reshape(nb, 8)}
    res = {}
    for tag, kw in (("budget", dict(maxEdges=49586)), ("cap", dict(maxNeighbors=38))):
        cb = ConvolutionBuilder(KDEWindow=0.2, **kw)   # (both op by op: a capped layer without capNative, a budgeted one always)
        cb.load_state_dict(state)
        cb.prefetch_geometry(ph, 0, radius, transposed="list")
        cb.reset()
        cb.opTrace_ = []
        F = _wrap(fs).requires_grad_(True)
        out = cb.create_convolution("c", ph, 0, F, fin, radius, multiFeatureConv=True, outNumFeatures=fout)
        out.backward(og)
        torch.cuda.synchronize()
        kG, kN, kP = cb.__compute_dic_keys__(ph, ph, 0, 0, radius, 0.2, True, True, kw.get("maxNeighbors", 0), None,
                                             kw.get("maxEdges", 0))
        grads = [F.grad] + [p.grad for _, p in sorted(cb.named_parameters())]
        assert len(grads) == 7 and all(x is not None for x in grads)
        res[tag] = (tuple(cb.cacheNeighs_[kN]), cb.cachePDFs_[kP], out.detach(), grads, cb, kN)
    cb, kN = res["budget"][4], res["budget"][5]
    assert kN.endswith("|e49586") and res["cap"][5].endswith("|38")
    assert int(cb.chosenCaps_[kN][0]) == 38 and not cb.cacheGeo_ and not res["cap"][4].chosenCaps_
    want = ref.cap_list(r["startIndexs"], r["packedNeighs"], 38)
    assert np.array_equal(_unwrap(res["budget"][0][0]), want[0]) and np.array_equal(_unwrap(res["budget"][0][1]), want[1])
    for a, b in zip(res["budget"][0], res["cap"][0]):
        assert torch.equal(a, b)
    assert torch.equal(res["budget"][1], res["cap"][1]), "PDFs"
    assert torch.equal(res["budget"][2], res["cap"][2]), "output"
    for i, (a, b) in enumerate(zip(res["budget"][3], res["cap"][3])):
        print("gradient", i, "max |diff|", float((a - b).abs().max()))
    for i, (a, b) in enumerate(zip(res["budget"][3], res["cap"][3])):
        assert torch.equal(a, b), "gradient %d" % i
