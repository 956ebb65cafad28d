"""The per-edge float64 reference of tests/pointgrad_ref.py (chunked KDE, per-edge gradients, ReLU ambiguity detector) and
the geometries of tests/pointgrad_cases.py, built with the CPU oracle: what each one reaches (exact row lengths, empty
rows, points nobody reaches, empty clouds, box ties) and the ambiguity cap of every layer shape that runs on it."""
import numpy as np
import pytest
import torch

from tests import pointgrad_cases as pc
from tests import pointgrad_ref as ref
from tests.helpers import make_mlp
from mccnn_amd.workloads import conv_nb

T = ref.t64


@pytest.fixture(scope="module")
def chains(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            g = pc.geometry(name)
            cache[name] = (g, pc.build(g, oracle, lambda a: a, lambda a: a))
        return cache[name]
    return get


@pytest.mark.parametrize("budget", [50, 4096])
def test_chunked_kde_equals_unchunked(chains, budget):
    """Budget 50 splits rows (up to 78 long) between groups; 4096 puts many rows in one group. The pairs of a slot are
    summed in the same order either way; what may differ is float64 rounding: a sum of k positive terms is within
    k 2^-53 of itself in any order, so the bound is 2 k 2^-53 |pdf|."""
    g, r = chains("B")
    args = (r["sortBatchs"], T(r["aabbMin"]), T(r["aabbMax"]), r["startIndexs"], r["packedNeighs"], pc.WINDOW,
            g["radius"], g["scaleInv"])
    assert len(ref._slot_groups(pc.row_lengths(r)[r["packedNeighs"][:, 1]], budget)) > 1
    want = ref.compute_pdf(T(r["sortPts"]), *args).numpy()
    got = ref.compute_pdf(T(r["sortPts"]), *args, pair_budget=budget).numpy()
    k = pc.row_lengths(r)[r["packedNeighs"][:, 1]]
    assert got.shape == want.shape
    assert (np.abs(got - want) <= 2 * k * 2.0 ** -53 * np.abs(want)).all()


def test_chunked_kde_gradients_equal_the_unchunked_reference(chains):
    """pdf_edge_grads (per-slot leaves, slot groups) summed to points and batches = autograd of the existing
    compute_pdf."""
    g, r = chains("B")
    gp = np.random.default_rng(5).random(len(r["packedNeighs"]))
    sp = T(r["sortPts"]).requires_grad_(True)
    mn, mx = T(r["aabbMin"]).requires_grad_(True), T(r["aabbMax"]).requires_grad_(True)
    pdf = ref.compute_pdf(sp, r["sortBatchs"], mn, mx, r["startIndexs"], r["packedNeighs"], pc.WINDOW, g["radius"], True)
    (pdf * T(gp)).sum().backward()
    dp, dR = ref.pdf_edge_grads(r["sortPts"], r["sortBatchs"], r["aabbMin"], r["aabbMax"], r["startIndexs"],
                                r["packedNeighs"], pc.WINDOW, g["radius"], True, gp, pair_budget=50)
    j = r["packedNeighs"][:, 0]
    dpts = np.zeros_like(r["sortPts"], dtype=np.float64)
    np.add.at(dpts, j, dp)
    assert np.allclose(dpts, sp.grad.numpy(), rtol=1e-10, atol=1e-12 * np.abs(dpts).max())
    dRb = np.bincount(r["sortBatchs"].reshape(-1)[j], weights=dR, minlength=g["B"])
    ext = r["aabbMax"].astype(np.float64) - r["aabbMin"]
    axis = ext.argmax(1)
    want_mx = np.zeros((g["B"], 3))
    want_mx[np.arange(g["B"]), axis] = dRb * g["radius"]
    assert np.allclose(want_mx, mx.grad.numpy(), rtol=1e-10, atol=1e-12 * np.abs(want_mx).max())
    assert np.allclose(-want_mx, mn.grad.numpy(), rtol=1e-10, atol=1e-12 * np.abs(want_mx).max())


@pytest.mark.parametrize("combin,fin,fout", [(True, 2, 5), (False, 16, 16)])
@pytest.mark.parametrize("avg", [True, False])
def test_per_edge_conv_gradients_sum_to_the_reference(chains, combin, fin, fout, avg):
    """conv_edge_grads summed per point, per centre and per batch = autograd of the existing spatial_conv reference."""
    g, r = chains("B")
    rng = np.random.default_rng(fin + fout)
    C = pc.centres_of(g)
    f = (2 * rng.random((len(r["sortPts"]), fin)) - 1).astype(np.float32)
    og = (2 * rng.random((len(C), fout if combin else fin)) - 1).astype(np.float32)
    w = make_mlp(conv_nb(fin, fout, combin), 3)
    pd = r["pdfs"].reshape(-1)
    sp, c, p64 = T(r["sortPts"]).requires_grad_(True), T(C).requires_grad_(True), T(pd).requires_grad_(True)
    mn, mx = T(r["aabbMin"]).requires_grad_(True), T(r["aabbMax"]).requires_grad_(True)
    out = ref.spatial_conv(sp, T(f), r["sortBatchs"], p64, c, r["startIndexs"], r["packedNeighs"], mn, mx, T(w["w1"]),
                           T(w["b1"]), T(w["w2"]), T(w["b2"]), T(w["w3"]), T(w["b3"]), fout, combin, g["B"], g["radius"],
                           True, avg)
    (out * T(og)).sum().backward()
    e = ref.conv_edge_grads(r["sortPts"], f, r["sortBatchs"], pd, C, r["startIndexs"], r["packedNeighs"], r["aabbMin"],
                            r["aabbMax"], w, og, fout, combin, g["radius"], True, avg, chunk=1000)
    j, i = r["packedNeighs"][:, 0], r["packedNeighs"][:, 1]
    close = lambda a, b: np.allclose(a, b, rtol=1e-10, atol=1e-12 * max(np.abs(b).max(), 1e-300))
    dpts = np.zeros((len(r["sortPts"]), 3))
    np.add.at(dpts, j, e["dp"])
    dc = np.zeros((len(C), 3))
    np.add.at(dc, i, e["dc"])
    assert close(dpts, sp.grad.numpy()) and close(dc, c.grad.numpy()) and close(e["dpdf"], p64.grad.numpy())
    assert np.array_equal(e["dc"], -e["dp"])
    dRb = np.bincount(r["sortBatchs"].reshape(-1)[j], weights=e["dR"], minlength=g["B"])
    assert close(dRb, mx.grad.numpy().max(1) / g["radius"] + mx.grad.numpy().min(1) / g["radius"])
    assert close(e["dR"], -(e["dp"] * e["delta"]).sum(1))


def test_per_edge_forms_pass_gradcheck(chains):
    """torch.autograd.gradcheck of the tensor forms behind conv_edge_grads and pdf_edge_grads, on a few edges of B."""
    g, r = chains("B")
    pk = r["packedNeighs"]
    sel = np.arange(40)
    w = make_mlp(conv_nb(3, 4, True), 4)
    rng = np.random.default_rng(6)
    j, c = pk[sel, 0], pk[sel, 1]
    P = T(r["sortPts"][j]).requires_grad_(True)
    Cc = T(pc.centres_of(g)[c]).requires_grad_(True)
    pd = T(r["pdfs"].reshape(-1)[sel]).requires_grad_(True)
    R = T(np.full(len(sel), 0.13)).requires_grad_(True)
    Fj, Oc, K = T(rng.random((len(sel), 3))), T(rng.random((len(sel), 4))), T(rng.integers(1, 9, len(sel)))
    conv = lambda P, Cc, pd, R: ref.conv_edge_terms(P, Cc, pd, R, Fj, Oc, K, w, 4, True)[0]
    assert torch.autograd.gradcheck(conv, (P, Cc, pd, R), eps=1e-6, atol=1e-6, rtol=1e-4)
    rows = pc.row_lengths(r)
    e1 = int(np.argmax(np.cumsum(rows) >= 60))          # the slots of the first rows, about 60
    ne = int(np.cumsum(rows)[e1])
    X = T(r["sortPts"][pk[:ne, 0]]).requires_grad_(True)
    Re = T(np.full(ne, 0.12) + 0.01 * rng.random(ne)).requires_grad_(True)
    first = np.repeat(r["startIndexs"].reshape(-1)[:e1 + 1], rows[:e1 + 1])
    k = np.repeat(rows[:e1 + 1], rows[:e1 + 1])
    pdf = lambda X, Re: torch.cat([ref._pdf_slots(X, Re, first, k, a, b, pc.WINDOW) for a, b in ref._slot_groups(k, 40)])
    assert torch.autograd.gradcheck(pdf, (X, Re), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_ambiguity_detector_flags_zero_and_spares_twice_tau():
    """One edge, R = 1, delta = (0.5, 0.25, 0.125). Layer-1 neuron 0: pre = delta . (1, 1, 1) + b with b = -0.875 (exactly
    0: flagged), then with b chosen so that pre = 2 tau S1 (not flagged). Every other neuron sits at pre = S = 1."""
    w1 = np.zeros((3, 8))
    w1[:, 0] = 1.0
    b1 = np.ones(8)
    w = dict(w1=w1.T.copy(), b1=b1, w2=np.zeros((8, 8)), b2=np.ones(8), w3=np.zeros((8, 8)), b3=np.zeros(8))
    pts = np.array([[0.5, 0.25, 0.125]])
    smp = np.zeros((1, 3))
    args = (pts, smp, np.zeros(1, np.int64), np.array([[0, 0]]), np.zeros((1, 3)), np.ones((1, 3)), w, 1.0, False)
    w["b1"][0] = -0.875
    pre1, S1, _, _ = ref.conv_preacts(*args[:-2], 1.0, False, np.arange(1))
    assert float(pre1[0, 0]) == 0.0
    assert ref.conv_ambiguity(*args).tolist() == [[0, 1, 0]]
    x = 0.875
    w["b1"][0] = -x * (1 - 2 * ref.TAU) / (1 + 2 * ref.TAU)
    pre1, S1, pre2, S2 = ref.conv_preacts(*args[:-2], 1.0, False, np.arange(1))
    assert abs(float(pre1[0, 0]) / float(S1[0, 0]) - 2 * ref.TAU) <= 1e-9 * ref.TAU
    assert len(ref.conv_ambiguity(*args)) == 0
    # layer 2 as well: pre2 of neuron 3 driven to 0 by its bias (h1 = 1 from neuron 1 with w2 = 1)
    w["w2"] = np.zeros((8, 8))
    w["w2"][3, 1] = 1.0    # flat layout w2[q*64 + o*8 + k]: out 3 reads in 1
    w["b2"][3] = -1.0
    assert ref.conv_ambiguity(*args).tolist() == [[0, 2, 3]]


def _claims(name, g, r):
    deg, tdeg = pc.row_lengths(r), pc.in_degree(r)
    B = g["B"]
    if name in ("A_abs", "A_rel"):
        assert deg.tolist() == list(pc.CLUMPS) + [0] * pc.FAR_CENTRES
        assert int(deg.sum()) == 8962 and int((deg.astype(np.int64) ** 2).sum()) == 16984070
    if name in ("B", "D"):
        sb = r["sortBatchs"].reshape(-1)
        for b in pc.EMPTY_CLOUDS:
            assert not (sb == b).any() and not (g["cbids"].reshape(-1) == b).any()
            assert (r["aabbMin"][b] == np.finfo(np.float32).max).all() and (r["aabbMax"][b] == -np.finfo(np.float32).max).all()
        assert (deg == 0).sum() >= 2 * (B - len(pc.EMPTY_CLOUDS))
        # the added far points (unsorted indices) are reached by nobody
        far = set(map(tuple, g["pts"][g["lonely"]].tolist()))
        hit = [tuple(p) in far for p in r["sortPts"].tolist()]
        assert sum(hit) == len(g["lonely"]) and (tdeg[np.array(hit)] == 0).all()
        # centres outside their cloud's box
        lo, hi = r["aabbMin"][g["cbids"].reshape(-1)], r["aabbMax"][g["cbids"].reshape(-1)]
        assert ((g["centres"] < lo) | (g["centres"] > hi)).any(1).sum() >= 4 * (B - len(pc.EMPTY_CLOUDS))
    if name == "C":
        p, b = g["pts"], g["bids"].reshape(-1)
        for k in range(B):
            q = p[b == k]
            assert ((q == q.min(0)).sum(0) >= 2).all() and ((q == q.max(0)).sum(0) >= 2).all()
            assert np.array_equal(q.min(0), r["aabbMin"][k]) and np.array_equal(q.max(0), r["aabbMax"][k])
        ext = r["aabbMax"][g["equal_xy"]] - r["aabbMin"][g["equal_xy"]]
        assert ext[0] == ext[1] > ext[2]
        assert (np.abs(p * 64 - np.round(p * 64)) == 0).all()
    if name == "E":
        assert len(r["packedNeighs"]) == 394222 and deg.max() == 31
    return deg


SHAPES_OF = {n: pc.SHAPES for n in ("A_abs", "A_rel", "B", "C", "D")}
SHAPES_OF["E"] = [(False, 16, 16, False)]


@pytest.mark.parametrize("name", pc.GEOMS)
def test_geometry_reaches_what_it_claims(chains, name):
    g, r = chains(name)
    deg = _claims(name, g, r)
    e = int(deg.sum())
    for s in SHAPES_OF[name]:
        a = pc.ambiguity(g, r, s)
        share = len(np.unique(a[:, 0])) / e
        print("  %s %-12s E = %d, ambiguous edges %.3f %%" % (name, pc.shape_id(s), e, 100 * share))
        assert share <= pc.AMBIGUITY_CAP, (name, pc.shape_id(s), share)


def test_d_is_b_translated(chains):
    gb, _ = chains("B")
    gd, _ = chains("D")
    assert np.array_equal(gd["pts"], (gb["pts"].astype(np.float64) + 500.0).astype(np.float32))
    assert np.array_equal(gd["bids"], gb["bids"]) and np.array_equal(gd["cbids"], gb["cbids"])
