"""Edge-budgeted neighbour lists through the native step executor (mccnn_geometry_build_budget / _build_batch_budget,
native.build_geometry(maxEdges=), Geometry.chosen_cap(), ConvolutionBuilder(budgetNative=True)).

Two exact references: (a) the oracle's uncapped list thinned at the K* of tests/neighbor_budget_ref.py's TABLE (asserted on the
CPU by tests/test_neighbor_budget_cpu.py) with tests/neighbor_cap_ref.py / tests/neighbor_sample_ref.py, and (b) the HIP op
chain find_neighbors(maxEdges=B, returnCap=True) + compute_pdf. startIndexs, packedNeighs, the edge total and the chosen cap
equal both; the PDFs equal (b) bit for bit (the same kernels over the same list).

Geometries: `mixed` (1020 centres), `big_windows` (3000) and `tall_rows` (6, rows of 70 000 hits: radix level 0 of the
selection is crossed) have <= 4096 centres -- three search launches: count, selection in one workgroup, a fill pass that clamps
and scans the row lengths itself; `many_centres` has 5000 -- count, three chip-wide selection levels, the chained clamp scan,
fill."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import neighbor_cap_ref as cref
from tests import neighbor_sample_ref as sref
from tests import neighbor_budget_ref as bref
from tests.helpers import make_mlp, conv_nb, assert_float_close, make_cloud

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's bar for float outputs (norm-wise and per element: tests/helpers.py)
WINDOW = 0.2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ORACLE = {}   # geometry name -> (geometry, the oracle's uncapped chain, its row lengths): computed once, never modified
_EXPECT = {}   # (name, B, Ku, seed) -> (K*, startIndexs, packedNeighs) of reference (a)
_GPU = {}      # geometry name -> device tensors of the inputs (points, boxes, cell count)


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _oracle_list(oracle, name):
    if name not in _ORACLE:
        g = bref.BUDGET_GEOMETRIES[name]()
        r = cref.uncapped(oracle, g)
        _ORACLE[name] = (g, r, cref.row_lengths(r["startIndexs"], len(r["packedNeighs"])))
    return _ORACLE[name]


def _table_cap(name, B):
    for b, K, _e in bref.TABLE[name][3]:
        if b == B:
            return K
    raise KeyError((name, B))


def _expect(oracle, name, B, Ku=0, seed=None):
    """Reference (a): (K*, the oracle's list at K*) -- K* from TABLE, or (B = 0) no budget: the cap is Ku."""
    key = (name, B, Ku, seed)
    if key not in _EXPECT:
        _, r, k = _oracle_list(oracle, name)
        if B == 0:
            K = Ku
        elif Ku == 0:
            K = _table_cap(name, B)
            assert K == bref.budget_cap(k, B)
        else:
            K = bref.budget_cap(k, B, Ku)
        if K == 0 or K >= int(k.max()):
            lst = (r["startIndexs"], r["packedNeighs"])          # nothing is cut: the uncapped list, whatever the seed
        elif seed is None:
            lst = cref.cap_list(r["startIndexs"], r["packedNeighs"], K)
        else:
            lst = sref.sample_list(r["startIndexs"], r["packedNeighs"], K, seed)
        _EXPECT[key] = (K,) + tuple(lst)
    return _EXPECT[key]


def _inputs(mc, g, name):
    if name not in _GPU:
        P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
        mn, mx = mc.compute_aabb(P, Bi, g["B"], g["scaleInv"])
        nc = mc._num_cells(mn, mx, g["B"], g["radius"], g["scaleInv"])
        _GPU[name] = dict(P=P, Bi=Bi, C=_wrap(g["centres"]), Cb=_wrap(g["cbids"]), mn=mn, mx=mx, nc=nc)
    return _GPU[name]


def _build(native, g, h, B=0, Ku=0, seed=None, usePDF=True, grid_from=None, side=-1, fork=False):
    return native.build_geometry(h["P"], h["Bi"], h["C"], h["Cb"], h["mn"], h["mx"], g["B"], h["nc"], g["radius"], g["scaleInv"],
                                 WINDOW, usePDF, grid_from=grid_from, side=side, fork=fork, maxNeighbors=Ku, sampleSeed=seed,
                                 maxEdges=B)


def _op_chain(mc, g, h, B, Ku=0, seed=None, usePDF=True):
    """Reference (b): the HIP ops one by one. -> (startIndexs, packedNeighs, pdfs, cap tensor)"""
    import torch
    sP, sB, cells, _idx, _inv = mc.build_grid(h["P"], h["Bi"], h["mn"], h["mx"], g["B"], g["radius"], g["scaleInv"])
    kw = dict(returnCap=True)
    if B:
        kw["maxEdges"] = B
    if Ku:
        kw["maxNeighbors"] = Ku
    if seed is not None:
        kw["sampleSeed"] = seed
    st, pk, cap = mc.find_neighbors(h["C"], h["Cb"], sP, cells, h["mn"], h["mx"], g["radius"], g["B"], g["scaleInv"], **kw)
    if usePDF:
        pdf = mc.compute_pdf(sP, sB, h["mn"], h["mx"], st, pk, WINDOW, g["radius"], g["B"], g["scaleInv"])
    else:
        pdf = torch.ones((pk.shape[0], 1), dtype=torch.float32, device=pk.device)
    return st, pk, pdf, cap


def _arrays(geo):
    st, pk = geo.neighbors()
    return st, pk, geo.pdfs(), geo.chosen_cap()


def _launches():
    from mccnn_amd import _lib
    return int(_lib.load().mccnn_debug_launch_count())


def _check(mc, oracle, native, name, B, Ku=0, seed=None, usePDF=True):
    """One geometry through the single chain against (a) and (b). -> its arrays"""
    import torch
    g, _r, _k = _oracle_list(oracle, name)
    h = _inputs(mc, g, name)
    K, want_st, want_pk = _expect(oracle, name, B, Ku, seed)
    geo = _build(native, g, h, B, Ku, seed, usePDF)
    st, pk, pdf, cap = _arrays(geo)
    print(name, "B", B, "Ku", Ku, "seed", seed, "m", geo.m, "K*", int(cap[0]), "E", geo.edges(), "capacity", geo.e_cap)
    assert cap.dtype == torch.int32 and tuple(cap.shape) == (1,) and cap.is_cuda and int(cap[0]) == K
    assert geo.edges() == len(want_pk) and geo.edges() <= geo.e_cap <= max(B, geo.m)
    assert np.array_equal(_unwrap(st), want_st) and np.array_equal(_unwrap(pk), want_pk)            # (a)
    bst, bpk, bpdf, bcap = _op_chain(mc, g, h, B, Ku, seed, usePDF)
    assert torch.equal(st, bst) and torch.equal(pk, bpk) and torch.equal(pdf, bpdf) and torch.equal(cap, bcap)   # (b)
    return st, pk, pdf, cap


def _search_launches(mc, oracle, native, name, B, seed=None):
    """Launches of the search inside a budgeted geometry's chain: those of the whole build, less those of the uncapped build of
    the same geometry, plus the uncapped search's own (two up to 4096 centres -- count, fill --, else count, scan, fill). The
    capacities are learned first: nothing is built twice inside a counted span."""
    import torch
    g, _r, _k = _oracle_list(oracle, name)
    h = _inputs(mc, g, name)
    _build(native, g, h).edges()
    _build(native, g, h, B, 0, seed).edges()
    torch.cuda.synchronize()
    l0 = _launches()
    a = _build(native, g, h)
    l1 = _launches()
    b = _build(native, g, h, B, 0, seed)
    l2 = _launches()
    assert a.edges() <= a.e_cap and b.edges() <= b.e_cap
    plain_search = 2 if len(g["centres"]) <= 4096 else 3
    return (l2 - l1) - (l1 - l0) + plain_search


@pytest.fixture(scope="module")
def native(mc):
    from mccnn_amd import native as nat
    return nat


# ------------------------------------------------------------------------------------------------- 1. small lists
@pytest.mark.parametrize("B", [500, 2040, 7217, 28867, 28869])
def test_single_chain_small_lists(mc, oracle, native, B):
    """`mixed`, m = 1020: the floor below m, budgets that bind and one the list fits -- canonical and with a seed."""
    import torch
    for seed in (None, 7):
        got = _check(mc, oracle, native, "mixed", B, 0, seed)
        if B == 28869:   # the list fits: the uncapped bytes
            g, _r, _k = _oracle_list(oracle, "mixed")
            plain = _build(native, g, _inputs(mc, g, "mixed"))
            assert torch.equal(got[0], plain.neighbors()[0]) and torch.equal(got[1], plain.neighbors()[1])
            assert torch.equal(got[2], plain.pdfs())


def test_a_cap_of_the_callers_binds_beside_the_budget(mc, oracle, native):
    """maxNeighbors = 5 beside B = 14434 (whose own K* is 15): the chosen cap is 5."""
    for seed in (None, 7):
        got = _check(mc, oracle, native, "mixed", 14434, 5, seed)
        assert int(got[3][0]) == 5 and _table_cap("mixed", 14434) == 15


def test_small_lists_take_three_search_launches(mc, oracle, native):
    for name, B, seed in (("mixed", 7217, None), ("mixed", 7217, 7), ("big_windows", 258081, None), ("tall_rows", 200000, None)):
        n = _search_launches(mc, oracle, native, name, B, seed)
        print(name, B, seed, "search launches", n)
        assert n == 3


# ------------------------------------------------------------------------------------------------- 2. large lists, tall rows
LARGE = [("many_centres", 5000), ("many_centres", 24495), ("many_centres", 97981), ("tall_rows", 6), ("tall_rows", 200000),
         ("tall_rows", 262149), ("big_windows", 258081)]


@pytest.mark.parametrize("name,B", LARGE, ids=["%s-%d" % nb for nb in LARGE])
def test_single_chain_large_lists(mc, oracle, native, name, B):
    """`many_centres`: the chip-wide levels and the chained clamp scan; `tall_rows`: rows of 70 000 hits."""
    for seed in (None, 7):
        _check(mc, oracle, native, name, B, 0, seed)


def test_large_lists_take_six_search_launches(mc, oracle, native):
    n = _search_launches(mc, oracle, native, "many_centres", 24495)
    print("many_centres search launches", n)
    assert n == 6   # count, three levels, clamp scan, fill


def test_use_pdf_false(mc, oracle, native):
    _check(mc, oracle, native, "mixed", 7217, 0, None, usePDF=False)
    _check(mc, oracle, native, "many_centres", 24495, 0, 7, usePDF=False)


# ------------------------------------------------------------------------------------------------- 3. shared grids
@pytest.mark.parametrize("owner_budgeted", [True, False], ids=["owner-budgeted", "owner-uncapped"])
def test_shared_grid_budgeted_and_uncapped(mc, oracle, native, owner_budgeted):
    import torch
    g, _r, _k = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, "mixed")
    for seed in (None, 9):
        bo, bs = (7217, 0) if owner_budgeted else (0, 7217)
        owner = _build(native, g, h, bo, 0, seed if bo else None)
        user = _build(native, g, h, bs, 0, seed if bs else None, grid_from=owner)
        assert user.grid_owner is owner
        for geo, B in ((owner, bo), (user, bs)):
            sd = seed if B else None
            own = _arrays(_build(native, g, h, B, 0, sd))           # the same geometry with a grid of its own
            got = _arrays(geo)
            K, want_st, want_pk = _expect(oracle, "mixed", B, 0, sd)
            assert np.array_equal(_unwrap(got[0]), want_st) and np.array_equal(_unwrap(got[1]), want_pk) and int(got[3][0]) == K
            for a, b in zip(got, own):
                assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 4. batch form
def test_batch_form_mixes_budgeted_requests_with_the_other_kinds(mc, oracle, native):
    """One begin_batch() / end_batch() of 20 requests, the chunk flush at 16 crossed: every array of every geometry equals its
    single chain's byte for byte, every chosen cap is TABLE's."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    specs = []   # (name, B, Ku, seed, shares the grid of spec #)
    for rep in range(2):
        specs += [("mixed", 0, 0, None, None), ("mixed", 7217, 0, None, None), ("mixed", 2040, 0, None, None),
                  ("mixed", 0, 16, None, None), ("mixed", 0, 16, 7 + rep, None), ("many_centres", 24495, 0, None, None),
                  ("big_windows", 258081, 0, None, None), ("mixed", 7217, 0, 3 + rep, None), ("mixed", 14434, 5, None, None),
                  ("many_centres", 97981, 0, 5 + rep, None)]
    specs[1] = ("mixed", 7217, 0, None, 0)       # budgeted over the grid of an uncapped owner
    specs[10] = ("mixed", 0, 0, None, 2)         # uncapped over the grid of a budgeted owner
    assert len(specs) >= 17
    singles = {}
    for name, B, Ku, seed, _s in specs:
        if (name, B, Ku, seed) not in singles:
            g, _r, _k = _oracle_list(oracle, name)
            singles[(name, B, Ku, seed)] = _arrays(_build(native, g, _inputs(mc, g, name), B, Ku, seed))
    torch.cuda.synchronize()
    geos = []
    native.begin_batch()
    try:
        for k, (name, B, Ku, seed, share) in enumerate(specs):
            g, _r, _k = _oracle_list(oracle, name)
            geos.append(_build(native, g, _inputs(mc, g, name), B, Ku, seed, grid_from=(geos[share] if share is not None else None),
                               side=0, fork=(k == 0)))
    finally:
        native.end_batch()
    for (name, B, Ku, seed, share), geo in zip(specs, geos):
        want = singles[(name, B, Ku, seed)]
        got = _arrays(geo)
        K, want_st, want_pk = _expect(oracle, name, B, Ku, seed)
        assert geo.edges() == len(want_pk) and int(got[3][0]) == K, (name, B, Ku, seed)
        assert np.array_equal(_unwrap(got[0]), want_st) and np.array_equal(_unwrap(got[1]), want_pk), (name, B, Ku, seed)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (name, B, Ku, seed, share)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 5. launch accounting
def _capi_batch(mc, oracle, reqs_spec, entry):
    """The requests (geometry name, B, Ku, seed) -- each with a grid of its own -- through ONE call of the C-ABI on the current
    stream: entry = "point" (mccnn_geometry_build_batch_point; no budgets), "null" (mccnn_geometry_build_batch_budget with
    budgets == NULL), "zero" (an all-zero budgets array) or "budgets". -> (launches issued, edge totals, chosen caps)"""
    import ctypes as C
    import torch
    from mccnn_amd import _lib
    lib = _lib.load()

    class Request(C.Structure):   # mccnn_geometry_request (include/mccnn.h)
        _fields_ = [("geometry", C.c_void_p), ("pts", C.c_void_p), ("batch_ids", C.c_void_p), ("n", C.c_int),
                    ("centres", C.c_void_p), ("centre_batch_ids", C.c_void_p), ("m", C.c_int), ("aabb_min", C.c_void_p),
                    ("aabb_max", C.c_void_p), ("batch_size", C.c_int), ("num_cells", C.c_int), ("radius", C.c_float),
                    ("scale_inv", C.c_int), ("window", C.c_float), ("use_pdf", C.c_int), ("e_capacity", C.c_int),
                    ("grid_from", C.c_void_p), ("buffer", C.c_void_p), ("buffer_bytes", C.c_size_t), ("total_host", C.c_void_p)]

    class Cap(C.Structure):       # mccnn_neighbor_cap
        _fields_ = [("max_neighbors", C.c_int), ("sampled", C.c_int), ("seed", C.c_uint)]

    class Budget(C.Structure):    # mccnn_neighbor_budget
        _fields_ = [("max_edges", C.c_int)]

    cnt = len(reqs_spec)
    reqs, capv, budv = (Request * cnt)(), (Cap * cnt)(), (Budget * cnt)()
    keep = []
    for k, (name, B, Ku, seed) in enumerate(reqs_spec):
        g, r, _k = _oracle_list(oracle, name)
        h = _inputs(mc, g, name)
        n, m = h["P"].shape[0], h["C"].shape[0]
        ecap = max(B, m) if B else (m * Ku if Ku else len(r["packedNeighs"]) + 64)    # nothing overflows
        nbytes = lib.mccnn_geometry_bytes_budget(n, m, g["B"], h["nc"], ecap, 1, Ku, B if entry == "budgets" else 0)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        slot = torch.empty(1, dtype=torch.int32).pin_memory()
        handle = lib.mccnn_geometry_create()
        keep.append((buf, slot, handle))
        reqs[k] = Request(handle, h["P"].data_ptr(), h["Bi"].data_ptr(), n, h["C"].data_ptr(), h["Cb"].data_ptr(), m,
                          h["mn"].data_ptr(), h["mx"].data_ptr(), g["B"], h["nc"], g["radius"], int(g["scaleInv"]), WINDOW, 1,
                          ecap, None, buf.data_ptr(), nbytes, slot.data_ptr())
        capv[k] = Cap(Ku, 0 if seed is None else 1, 0 if seed is None else seed)
        budv[k] = Budget(B if entry == "budgets" else 0)
    torch.cuda.synchronize()
    l0 = _launches()
    stream = _lib.stream_handle()
    if entry == "point":
        rc = lib.mccnn_geometry_build_batch_point(C.addressof(reqs), C.addressof(capv), None, cnt, stream)
    else:
        rc = lib.mccnn_geometry_build_batch_budget(C.addressof(reqs), C.addressof(capv), None,
                                                   None if entry == "null" else C.addressof(budv), cnt, stream)
    assert rc == 0
    torch.cuda.synchronize()
    launches = _launches() - l0
    totals = [int(slot[0]) for _buf, slot, _h in keep]
    caps = []
    for (buf, _slot, handle), (name, B, Ku, seed) in zip(keep, reqs_spec):
        addr = lib.mccnn_geometry_cap(handle)
        if B and entry == "budgets":
            off = addr - buf.data_ptr()
            caps.append(int(buf[off:off + 4].view(torch.int32)[0]))
        else:
            assert not addr        # no budget: no cap word (the cap is the caller's max_neighbors)
            caps.append(Ku)
        lib.mccnn_geometry_destroy(handle)
    return launches, totals, caps


def test_launch_accounting_through_the_c_abi(mc, oracle, native):
    others = [("mixed", 0, 0, None), ("mixed", 0, 16, None), ("mixed", 0, 16, 3), ("many_centres", 0, 0, None)]
    base = _capi_batch(mc, oracle, others, "point")
    print("launches of mccnn_geometry_build_batch_point over", len(others), "requests without a budget:", base[0])
    assert base[0] > 0
    assert _capi_batch(mc, oracle, others, "null") == base          # budgets == NULL
    assert _capi_batch(mc, oracle, others, "zero") == base          # an all-zero budgets array
    assert _capi_batch(mc, oracle, others, "budgets") == base       # (no request carries one)
    # budgeted requests in the chunk, beside a capped one (whose count launch they join): the selection of the small lists, the
    # three levels of the larger ones, one clamped prefix sum, one fill launch per budget kind
    small = [("mixed", 7217, 0, None), ("mixed", 2040, 0, None)]
    got = _capi_batch(mc, oracle, others + small, "budgets")
    print("with two small budgeted requests:", got[0])
    assert got[0] == base[0] + 1 + 1 + 1
    every = small + [("many_centres", 24495, 0, None), ("big_windows", 258081, 0, None), ("mixed", 7217, 0, 9), ("mixed", 14434, 5, None)]
    got = _capi_batch(mc, oracle, others + every, "budgets")
    print("with small, large, sampled and capped budgeted requests:", got[0])
    assert got[0] == base[0] + 1 + 3 + 1 + 2 and got[0] <= base[0] + 1 + 3 + 1 + 2
    for (name, B, Ku, seed), e, K in zip(others + every, got[1], got[2]):
        want = _expect(oracle, name, B, Ku, seed)
        assert e == len(want[2]) and K == want[0], (name, B, Ku, seed)
    # budgeted requests alone: the count launch is the capped one, and theirs
    alone = _capi_batch(mc, oracle, small, "budgets")
    plain = _capi_batch(mc, oracle, [("mixed", 0, 0, None)] * 2, "point")
    print("two small budgeted requests alone:", alone[0], "two uncapped ones:", plain[0])
    assert alone[0] == plain[0] + 1         # the selection; the clamped prefix sum stands where the plain one stood


# ------------------------------------------------------------------------------------------------- 6. capacity
def test_capacity_is_bounded_by_the_budget(mc, oracle, native):
    """The first geometry of a shape: capacity = min(max(B, m), the plain guess)."""
    g, _r, _k = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, "mixed")
    m = len(g["centres"])
    native._EDGE_GUESS.clear()
    native._EDGE_RATIO.clear()
    guess = 48 * m + 1024
    for B, seed in ((7217, None), (500, 2), (10 ** 6, None)):
        native._EDGE_GUESS.clear()
        native._EDGE_RATIO.clear()
        geo = _build(native, g, h, B, 0, seed)
        assert geo.e_cap == min(max(B, m), guess), (B, geo.e_cap)
        assert 0 < geo.edges() <= geo.e_cap
    geo = _build(native, g, h, 14434, 5)
    assert geo.e_cap <= min(max(14434, m), 5 * m)
    # the budgeted totals have not touched the guess of the uncapped geometry of this shape
    native._EDGE_GUESS.clear()
    native._EDGE_RATIO.clear()
    _build(native, g, h, 7217).edges()
    assert _build(native, g, h).e_cap == guess


def test_starved_guess_rebuilds_with_the_same_budget_and_seed(mc, oracle, native, monkeypatch):
    import torch
    g, _r, _k = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, "mixed")
    for B, seed in ((7217, None), (7217, 21)):
        want = _arrays(_build(native, g, h, B, 0, seed))
        native._EDGE_GUESS.clear()
        native._EDGE_RATIO.clear()
        monkeypatch.setattr(native, "_ECAP_SCALE", 0.02)
        geo = _build(native, g, h, B, 0, seed)
        starved = geo.e_cap
        monkeypatch.setattr(native, "_ECAP_SCALE", 1.0)
        e = geo.edges()
        assert starved < e <= geo.e_cap <= max(B, geo.m) and geo.budget == B and geo.cap == (0, seed)   # it overflowed, and was built again
        for a, b in zip(_arrays(geo), want):
            assert torch.equal(a, b)
        K, _st, want_pk = _expect(oracle, "mixed", B, 0, seed)
        assert np.array_equal(_unwrap(geo.neighbors()[1]), want_pk) and int(geo.chosen_cap()[0]) == K
    native._EDGE_GUESS.clear()
    native._EDGE_RATIO.clear()


# ------------------------------------------------------------------------------------------------- 7. layers
LAYERS = [(1, 64, True), (3, 8, True), (16, 16, False)]


@pytest.mark.parametrize("fin,fout,combin", LAYERS, ids=["1to64", "3to8", "dw16"])
def test_layers_over_a_budgeted_geometry(mc, oracle, native, fin, fout, combin):
    """Forward and all seven gradients of native.conv over a budgeted geometry against spatial_conv over the op-built list --
    the standard of the capped native layers (tests/test_gpu_native_cap.py::test_builder_cap_native): the 1e-4 bar."""
    import torch
    g, _r, _k = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, "mixed")
    B = 7217
    rng = np.random.default_rng(77)
    n, m = len(g["pts"]), len(g["centres"])
    fs = (2 * rng.random((n, fin)) - 1).astype(np.float32)
    og = _wrap((2 * rng.random((m, fout if combin else fin)) - 1).astype(np.float32))
    w = make_mlp(conv_nb(fin, fout, combin), 41)
    order = ("w1", "b1", "w2", "b2", "w3", "b3")

    def leaves():
        return _wrap(fs).requires_grad_(True), {k: _wrap(w[k]).requires_grad_(True) for k in order}

    geo = _build(native, g, h, B)
    F, W = leaves()
    out = native.conv(geo, F, W["w1"], W["b1"], W["w2"], W["b2"], W["w3"], W["b3"], fout, combin, True)
    got = [out.detach()] + list(torch.autograd.grad(out, [F] + [W[k] for k in order], og))
    sP, sB, cells, idx, _inv = mc.build_grid(h["P"], h["Bi"], h["mn"], h["mx"], g["B"], g["radius"], g["scaleInv"])
    st, pk, pdf, _cap = _op_chain(mc, g, h, B)
    F, W = leaves()
    ref = mc.spatial_conv(sP, F, sB, pdf, h["C"], st, pk, h["mn"], h["mx"], W["w1"], W["w2"], W["w3"], W["b1"], W["b2"], W["b3"],
                          fout, combin, g["B"], g["radius"], g["scaleInv"], True, sortIndex=idx)
    want = [ref.detach()] + list(torch.autograd.grad(ref, [F] + [W[k] for k in order], og))
    for k, (a, b) in enumerate(zip(got, want)):
        what = "output" if k == 0 else ("feature gradient" if k == 1 else "gradient of " + order[k - 2])
        print("%d -> %d %s: max |diff| %.3e of max |ref| %.3e" % (fin, fout, what, float((a - b).abs().max()), float(b.abs().max())))
        assert_float_close(_unwrap(a).reshape(-1), _unwrap(b).reshape(-1), RTOL, what)


# ------------------------------------------------------------------------------------------------- 8. builder
GRAPH = [  # name, lin, lout, fin, fout, combin, radius: six neighbour lists over four grids (tests/test_gpu_native_cap.py)
    ("Conv_f1", 0, 0, 1, 16, True, 0.12), ("Conv_dw", 0, 0, 16, 16, False, 0.12), ("Pool_dw", 0, 1, 16, 16, False, 0.2),
    ("Pool_f1", 0, 1, 1, 8, True, 0.12), ("Conv_l1", 1, 1, 32, 32, False, 0.3), ("Up_dw", 1, 0, 16, 16, False, 0.3),
    ("Conv_3to8", 0, 0, 3, 8, True, 0.16),
]
LISTS = [(0, 0, 0.12), (0, 1, 0.2), (0, 1, 0.12), (1, 1, 0.3), (1, 0, 0.3), (0, 0, 0.16)]   # (lin, lout, radius) of the six lists
SIZES = ((2500, 5), (1800, 6), (1200, 6), (3200, 7), (700, 8))   # (points per cloud, seed) of the batches below
# (centres, uncapped edges) of the six lists of batch SIZES[0], from the oracle on the CPU -- asserted against it below
TOTALS_0 = [(7045, 1097907), (1089, 76987), (1089, 21632), (1089, 32301), (7045, 226608), (7045, 1254049)]
# the budget of the graph's layers: it binds on four lists of that batch (two of 7045 centres each way, one of 1089) and not
# on the other two
B_GRAPH = 50000


class _Net:
    """The graph above over batches of different sizes, every layer budgeted: feature rows and output gradients fixed per batch."""

    def __init__(self, sizes):
        import torch
        self.clouds = [make_cloud(n, 3, s, "clustered", True) for n, s in sizes]
        self.dev = [(_wrap(p), _wrap(b)) for p, b in self.clouds]
        self.feats, self.ogs = {}, {}
        torch.manual_seed(5)

    def hierarchy(self, ci):
        import torch
        from mccnn_amd.MCConvBuilder import PointHierarchy
        P, Bi = self.dev[ci]
        return PointHierarchy(P, torch.ones((P.shape[0], 1), device="cuda"), Bi, [0.1], "PH", 3, True)

    def step(self, cb, ci, ph=None, then=None, layers=None, backward=True):
        import torch
        cb.reset()
        if then is not None:
            then()
        ph = ph if ph is not None else self.hierarchy(ci)
        outs, fts, idx = [], [], []
        for li, (name, lin, lout, fin, fout, combin, radius) in enumerate(GRAPH):
            if layers is not None and li not in layers:
                continue
            n = ph.points_[lin].shape[0]
            f = self.feats.setdefault((ci, name), 2 * torch.rand((n, fin), device="cuda") - 1).detach().clone().requires_grad_(True)
            fts.append(f)
            idx.append(li)
            outs.append(cb.create_convolution(name, ph, lin, f, fin, radius, ph, lout, combin, fout))
        for li, o in zip(idx, outs):
            self.ogs.setdefault((ci, li), 2 * torch.rand(o.shape, device="cuda") - 1)
        if not backward:
            return [o.detach() for o in outs], []
        grads = torch.autograd.grad(outs, fts + list(cb.parameters()), [self.ogs[(ci, li)] for li in idx], allow_unused=True)
        return [o.detach() for o in outs], [x for x in grads if x is not None]


def _builders(budget, seed, native_flag=True):
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    torch.manual_seed(1)
    run = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, maxEdges=budget, sampleSeed=seed, budgetNative=native_flag)
    quiet = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, maxEdges=budget, sampleSeed=seed, budgetNative=False)
    quiet.geoPrefetch_ = False     # the reference: op by op, nothing runs ahead
    return run, quiet


def _sync_state(src, dst):
    dst.load_state_dict({k: v.detach().clone() for k, v in src.state_dict().items()})


def _graph_totals(oracle, ph):
    """(centres, uncapped edges, row lengths) of the six lists of a hierarchy, from the oracle."""
    mn, mx = _unwrap(ph.aabbMin_), _unwrap(ph.aabbMax_)
    out = []
    for lin, lout, r in LISTS:
        pi, bi = _unwrap(ph.points_[lin]), _unwrap(ph.batchIds_[lin])
        keys, idx = oracle.sort_points_step1(pi, bi, mn, mx, 3, r, True)
        sp, _sb, _sf, cells = oracle.sort_points_step2(pi, bi, np.ones((len(pi), 1), np.float32), keys, idx, mn, mx, 3, r, True)
        st, pk = oracle.find_neighbors(_unwrap(ph.points_[lout]), _unwrap(ph.batchIds_[lout]), sp, cells, mn, mx, r, 3, True)
        out.append((len(st), len(pk), cref.row_lengths(st, len(pk))))
    return out


def _cap_value(v):
    return int((v.value() if hasattr(v, "value") else v)[0])


# The feature gradients of the combin layers with at most four input features (Conv_f1, Pool_f1, Conv_3to8: gradients 0, 3 and
# 6 of _Net.step) are summed with float atomics on BOTH paths: the op-by-op builder does not reproduce them bit for bit in a
# repeat of its own step (measured on the MI355X: 3.0e-7 of 1.28, 3.0e-8 of 0.36, 2.1e-7 of 0.59 against its repeat; the native
# path against it: 3.0e-7, 3.0e-8, 1.8e-7). They are held to the bar tests/test_gpu_native_cap.py holds them to, 1e-5 of the
# largest value; the other 46 gradients and every output are held bit for bit.
ATOMIC_GRADS = tuple(k for k, l in enumerate(GRAPH) if l[5] and l[3] <= 4)


def test_builder_budget_native(mc, oracle, native):
    """budgetNative=True against False over the graph: outputs and gradients bit for bit (ATOMIC_GRADS above: 1e-5), the same
    cache keys, chosenCaps_ with equal values -- and fewer launches."""
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    net = _Net(SIZES[:1])
    ph = net.hierarchy(0)
    tot = _graph_totals(oracle, ph)
    assert [(m, e) for m, e, _k in tot] == TOTALS_0
    binds = [e > B_GRAPH for _m, e, _k in tot]
    assert binds == [True, True, False, False, True, True]
    res = {}
    for seed in (None, 7):
        for bn in (True, False):
            torch.manual_seed(1)
            cb = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, maxEdges=B_GRAPH, sampleSeed=seed, budgetNative=bn)
            cb.geoPrefetch_ = False
            if (seed, not bn) in res:
                _sync_state(res[(seed, not bn)][0], cb)
            net.step(cb, 0, ph=ph)                       # shapes and capacities learned
            torch.cuda.synchronize()
            l0 = _launches()
            outs, grads = net.step(cb, 0, ph=ph)
            torch.cuda.synchronize()
            launches = _launches() - l0
            keys = (sorted(cb.cacheGrids_), sorted(cb.cacheNeighs_), sorted(cb.cachePDFs_), sorted(cb.chosenCaps_))
            assert len(keys[1]) == 6 and all(("|e%d" % B_GRAPH) in k for k in keys[1]) and keys[3] == keys[1]
            if bn:
                assert sorted(cb.cacheGeo_) == keys[2] and all(geo.budget == B_GRAPH for geo in cb.cacheGeo_.values())
            else:
                assert not cb.cacheGeo_
            caps = {k: _cap_value(v) for k, v in cb.chosenCaps_.items()}
            lists = {k: tuple(_unwrap(t) for t in cb.cacheNeighs_[k]) for k in keys[1]}
            res[(seed, bn)] = (cb, outs, grads, keys, caps, lists, launches)
        a, b = res[(seed, True)], res[(seed, False)]
        print("seed", seed, "launches per step: budgetNative", a[6], "op by op", b[6], "caps", sorted(a[4].values()))
        assert a[3] == b[3] and a[4] == b[4]
        for k in a[5]:
            assert np.array_equal(a[5][k][0], b[5][k][0]) and np.array_equal(a[5][k][1], b[5][k][1]), k
        # the caps are the oracle's: K* of every list's row lengths under the budget
        kN = {}
        for (lin, lout, r), (_m, _e, k) in zip(LISTS, tot):
            key = a[0].__compute_dic_keys__(ph, ph, lin, lout, r, 0.25, True, True, 0, seed, B_GRAPH)[1]
            kN[key] = bref.budget_cap(k, B_GRAPH)
        assert a[4] == kN
        for x, y in zip(a[1], b[1]):
            assert torch.equal(x, y)
        diffs = [(float((x - y).abs().max()), float(y.abs().max())) for x, y in zip(a[2], b[2])]
        again = net.step(b[0], 0, ph=ph)[1]          # the op-by-op builder once more: what it reproduces of itself
        self_diffs = [float((x - y).abs().max()) for x, y in zip(again, b[2])]
        for k, ((d, top), sd) in enumerate(zip(diffs, self_diffs)):
            print("gradient %d: max |diff| %.3e of %.3e; op by op against its own repeat %.3e" % (k, d, top, sd))
        for k, (x, y) in enumerate(zip(a[2], b[2])):
            if k in ATOMIC_GRADS:
                assert diffs[k][0] <= 1e-5 * diffs[k][1], k
            else:
                assert torch.equal(x, y), k
        assert a[6] < b[6]
    assert not torch.equal(res[(None, True)][1][0], res[(7, True)][1][0])      # the seed draws another sample


def test_prefetch_step_files_the_budgeted_geometries(mc, native):
    """prefetch_step under budgetNative_: the next step's budgeted geometries are parked, reset() installs them under the '|e'
    keys of the seed they were asked for, the layers find them and none is built twice; maxEdges_ and sampleSeed_ reassigned
    between steps (followed by reset()) are honoured."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    net = _Net(SIZES[:2])
    run, quiet = _builders(B_GRAPH, 100)
    for ci in (1, 0):
        net.step(run, ci)
    _sync_state(run, quiet)
    order = [0, 1, 1, 0, 1, 0]
    budgets = [B_GRAPH, B_GRAPH, 30000, 30000, 30000, B_GRAPH]
    # The learned plan a prefetch_step replays is the graph of the last COMPLETED step, budgets included: the geometries for
    # step s are started during step s - 1 from the plan of step s - 2 (as with a reassigned maxNeighbors_).
    planned = [B_GRAPH, B_GRAPH] + budgets[:-2]
    nxt, parked = None, {}     # the next step's hierarchy and the geometries prefetch_step parked for it (key -> Geometry)
    for s, ci in enumerate(order):
        seed, budget = 100 + s, budgets[s]
        quiet.sampleSeed_, quiet.maxEdges_ = seed, budget
        want = net.step(quiet, ci)
        torch.cuda.synchronize()
        run.sampleSeed_, run.maxEdges_ = seed, budget
        state = {}

        def start_next():
            if s + 1 < len(order):
                state["ph"] = net.hierarchy(order[s + 1])
                state["n"] = run.prefetch_step(state["ph"], sampleSeed=seed + 1)
                state["parked"] = {k: v[0] for k, v in run.prefetchedGeo_.items()}
        parked_before = parked
        got = net.step(run, ci, ph=nxt, then=start_next)
        tag = "|e%d|s%d" % (budget, seed)
        mine = {k: geo for k, geo in run.cacheGeo_.items() if k.endswith(tag)}      # the geometries this step's layers used
        assert len(mine) == 6 and all(geo.budget == budget for geo in mine.values()), (s, sorted(run.cacheGeo_))
        # (a prefetch_step made with the budget of the step before parks geometries under that budget's keys: after a
        # reassignment nobody asks for them, and the reset() after drops them)
        assert len(run.cacheGeo_) == (6 if s == 0 or budgets[s] == planned[s] else 12)
        # the plan remembers the budget of the step that made it: a step whose budget is the plan's finds its geometries parked
        if s >= 1 and budgets[s] == planned[s]:
            assert parked_before and all(run.cacheGeo_[k] is g for k, g in parked_before.items()), s    # found, not built twice
            assert set(parked_before) == set(run.cacheGeo_)
            assert all(geo.core.side >= 0 for geo in run.cacheGeo_.values())
        if s >= 1 and budgets[s] != planned[s]:
            assert parked_before and not (set(parked_before) & set(mine))
        if s + 1 < len(order) and s >= 1:
            assert state["n"] == 6
        parked = state.get("parked", {})
        nxt = state.get("ph")
        for a, b in zip(got[0], want[0]):
            assert torch.equal(a, b), s
        for a, b in zip(got[1], want[1]):   # (feature gradients of one-feature layers are summed with float atomics)
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
        caps = {k: v for k, v in run.chosenCaps_.items() if k.endswith(tag)}     # (views: of this step's geometries alone)
        assert len(caps) == 6 and len(run.chosenCaps_) == len(run.cacheGeo_) and set(caps) <= set(quiet.chosenCaps_)
        for k, v in caps.items():
            assert _cap_value(v) == _cap_value(quiet.chosenCaps_[k]), (s, k)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 9. soak
def test_soak_budgeted_pipelined_loop(mc, native):
    """A few hundred pipelined steps: the batch, the budget and the seed change every step, random layer subsets, skipped
    backward passes, the next batch's geometries started by prefetch_step under the current step -- no host synchronisation
    inside the loop. Every output is compared on the GPU with a reference computed op by op with nothing running ahead."""
    import time
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    net = _Net(SIZES[2:] + SIZES[1:2])
    run, quiet = _builders(20000, 0)
    net.step(run, 0)
    _sync_state(run, quiet)
    steps = 200
    rng = np.random.default_rng(11)
    order = rng.integers(0, len(net.clouds), steps)
    budgets = [int(b) for b in rng.choice([1500, 6000, 20000, 60000, 10 ** 7], steps)]
    subsets = [None if rng.random() < 0.5 else sorted(set(int(x) for x in rng.integers(0, len(GRAPH), 4))) for _ in range(steps)]
    backward = [bool(rng.random() < 0.7) for _ in range(steps)]
    refs = []
    for s in range(steps):
        quiet.sampleSeed_, quiet.maxEdges_ = s, budgets[s]
        refs.append(net.step(quiet, int(order[s]), layers=subsets[s], backward=backward[s]))
    torch.cuda.synchronize()
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    worst = torch.zeros((), dtype=torch.float32, device="cuda")
    nxt = None
    t0 = time.perf_counter()
    for s in range(steps):
        assert time.perf_counter() - t0 < 120.0, "the soak loop measures a few seconds: step %d after two minutes" % s
        run.sampleSeed_, run.maxEdges_ = s, budgets[s]
        state = {}

        def start_next():
            if s + 1 < steps:
                state["ph"] = net.hierarchy(int(order[s + 1]))
                run.prefetch_step(state["ph"], sampleSeed=s + 1)
        outs, grads = net.step(run, int(order[s]), ph=nxt, then=start_next, layers=subsets[s], backward=backward[s])
        nxt = state.get("ph")
        for o, r in zip(outs, refs[s][0]):
            bad += (o != r).sum()
        for a, b in zip(grads, refs[s][1]):
            worst = torch.maximum(worst, (a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    torch.cuda.synchronize()
    print("soak: %d steps in %.1f s, forward mismatches %d, worst relative gradient deviation %.2e" % (
        steps, time.perf_counter() - t0, int(bad), float(worst)))
    assert int(bad) == 0 and float(worst) < 1e-4


# ------------------------------------------------------------------------------------------------- 10. ctypes binding
def test_ctypes_binding_inner(mc, oracle, native):
    """(run by test_ctypes_binding in a child process with MCCNN_TORCH_EXT=0; with the extension loaded it checks that one)"""
    for name, B, seed in (("mixed", 7217, None), ("many_centres", 24495, 13)):
        _check(mc, oracle, native, name, B, 0, seed)


def test_ctypes_binding():
    """One budgeted and one budget-sampled geometry through the ctypes binding of the C-ABI (mccnn_geometry_build_budget)."""
    env = dict(os.environ, MCCNN_TORCH_EXT="0")
    code = ("import sys, pytest; from mccnn_amd import native; assert native._EXT is None; "
            "sys.exit(pytest.main([%r, '-m', 'gpu', '-x', '-q', '-k', 'test_ctypes_binding_inner']))"
            % os.path.join(ROOT, "tests", "test_gpu_native_budget.py"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
