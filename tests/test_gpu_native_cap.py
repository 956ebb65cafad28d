"""Capped and sampled neighbour lists through the native step executor (mccnn_geometry_build_capped / _build_batch_capped,
native.build_geometry(maxNeighbors=, sampleSeed=), ConvolutionBuilder(capNative=True)).

Two exact references: (a) the oracle's uncapped list thinned by tests/neighbor_cap_ref.py / tests/neighbor_sample_ref.py, and
(b) the HIP op-by-op chain, find_neighbors(maxNeighbors=, sampleSeed=) + compute_pdf. startIndexs, packedNeighs and the edge
total equal both; the PDFs equal (b) bit for bit (the same kernels over the same list).

Geometries (tests/neighbor_cap_ref.py; figures in tests/test_gpu_neighbor_cap.py): `mixed`, `mid_windows` and `big_windows`
have <= 4096 centres -- the executor's two-launch chain, whose fill pass scans the capped counts itself --, `many_centres`
has 5000 (count, scan, fill), `huge` below 17 000 foreign centres (a visiting order of the geometry's own)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import neighbor_cap_ref as ref
from tests import neighbor_sample_ref as sref
from tests.helpers import make_mlp, conv_nb, assert_float_close, make_cloud

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's bar for float outputs (norm-wise and per element: tests/helpers.py)
WINDOW = 0.2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ORACLE = {}   # geometry name -> (geometry, the oracle's uncapped chain): computed once, never modified
_EXPECT = {}   # (name, K, seed) -> (startIndexs, packedNeighs) of reference (a)
_GPU = {}      # geometry name -> device tensors of the inputs (points, boxes, cell count)


def geom_huge():
    """Two uniform clouds of 10 000 points each, absolute radius 0.12; centres = a shuffled subset of 17 000 points: more than
    the 16 384 from which a geometry over foreign centres builds a visiting order of its own. ~1.2 M uncapped edges."""
    rng = np.random.default_rng(105)
    pts, bids = ref._two_clouds(rng, (10000, 10000))
    sel = rng.permutation(len(pts))[:17000]
    return dict(pts=pts, bids=bids, centres=np.ascontiguousarray(pts[sel]), cbids=np.ascontiguousarray(bids[sel]), B=2,
                radius=0.12, scaleInv=False)


GEOMS = dict(ref.GEOMETRIES, huge=geom_huge)


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _oracle_list(oracle, name, scaleInv=None):
    key = name if scaleInv is None else (name, scaleInv)
    if key not in _ORACLE:
        g = GEOMS[name]()
        if scaleInv is not None:
            g = dict(g, scaleInv=scaleInv)
        _ORACLE[key] = (g, ref.uncapped(oracle, g))
    return _ORACLE[key]


def _expect(oracle, name, K, seed=None, scaleInv=None):
    """Reference (a): the oracle's list under cap K (0: uncapped) and the op's seed (None: the canonical ranks)."""
    key = (name, K, seed, scaleInv)
    if key not in _EXPECT:
        _, r = _oracle_list(oracle, name, scaleInv)
        if K == 0:
            _EXPECT[key] = (r["startIndexs"], r["packedNeighs"])
        elif seed is None:
            _EXPECT[key] = ref.cap_list(r["startIndexs"], r["packedNeighs"], K)
        else:
            _EXPECT[key] = sref.sample_list(r["startIndexs"], r["packedNeighs"], K, seed)
    return _EXPECT[key]


def _inputs(mc, g, key):
    if key not in _GPU:
        P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
        mn, mx = mc.compute_aabb(P, Bi, g["B"], g["scaleInv"])
        nc = mc._num_cells(mn, mx, g["B"], g["radius"], g["scaleInv"])
        _GPU[key] = dict(P=P, Bi=Bi, C=_wrap(g["centres"]), Cb=_wrap(g["cbids"]), mn=mn, mx=mx, nc=nc)
    return _GPU[key]


def _build(native, g, h, K=0, seed=None, usePDF=True, grid_from=None, side=-1, fork=False):
    return native.build_geometry(h["P"], h["Bi"], h["C"], h["Cb"], h["mn"], h["mx"], g["B"], h["nc"], g["radius"], g["scaleInv"],
                                 WINDOW, usePDF, grid_from=grid_from, side=side, fork=fork, maxNeighbors=K, sampleSeed=seed)


def _op_chain(mc, g, h, K, seed, usePDF=True):
    """Reference (b): the HIP ops one by one."""
    import torch
    sP, sB, cells, _idx, _inv = mc.build_grid(h["P"], h["Bi"], h["mn"], h["mx"], g["B"], g["radius"], g["scaleInv"])
    kw = {} if K == 0 else (dict(maxNeighbors=K) if seed is None else dict(maxNeighbors=K, sampleSeed=seed))
    st, pk = mc.find_neighbors(h["C"], h["Cb"], sP, cells, h["mn"], h["mx"], g["radius"], g["B"], g["scaleInv"], **kw)
    if usePDF:
        pdf = mc.compute_pdf(sP, sB, h["mn"], h["mx"], st, pk, WINDOW, g["radius"], g["B"], g["scaleInv"])
    else:
        pdf = torch.ones((pk.shape[0], 1), dtype=torch.float32, device=pk.device)
    return st, pk, pdf


def _arrays(geo):
    st, pk = geo.neighbors()
    return st, pk, geo.pdfs()


def _check(mc, oracle, native, name, K, seed=None, scaleInv=None, usePDF=True):
    """One geometry through the single chain against (a) and (b). -> its arrays"""
    import torch
    g, _ = _oracle_list(oracle, name, scaleInv)
    h = _inputs(mc, g, (name, scaleInv))
    want_st, want_pk = _expect(oracle, name, K, seed, scaleInv)
    geo = _build(native, g, h, K, seed, usePDF)
    st, pk, pdf = _arrays(geo)
    print(name, "K", K, "seed", seed, "scaleInv", g["scaleInv"], "m", geo.m, "E", geo.edges(), "capacity", geo.e_cap)
    assert geo.edges() == len(want_pk) and geo.edges() <= geo.e_cap
    assert np.array_equal(_unwrap(st), want_st) and np.array_equal(_unwrap(pk), want_pk)            # (a)
    bst, bpk, bpdf = _op_chain(mc, g, h, K, seed, usePDF)
    assert torch.equal(st, bst) and torch.equal(pk, bpk) and torch.equal(pdf, bpdf)                   # (b), PDFs bit for bit
    if K > 0:
        assert geo.e_cap <= geo.m * K
    return st, pk, pdf


@pytest.fixture(scope="module")
def native(mc):
    from mccnn_amd import native as nat
    return nat


# ------------------------------------------------------------------------------------------------- 1. small lists
SMALL = [("mixed", 1, None), ("mixed", 16, None), ("mixed", 1, False), ("mixed", 16, False),
         ("mid_windows", 16, None), ("big_windows", 1, None), ("big_windows", 64, None), ("big_windows", 300, None)]


@pytest.mark.parametrize("name,K,scaleInv", SMALL, ids=["%s-K%d%s" % (n, k, "" if s is None else "-abs") for n, k, s in SMALL])
def test_single_chain_small_lists(mc, oracle, native, name, K, scaleInv):
    """m <= 4096: capped count pass, then the capped / sampled fill pass that scans min(k, K) itself and publishes the capped
    total -- canonical and with two seeds."""
    for seed in (None, 7, 0xFFFFFFF1):
        _check(mc, oracle, native, name, K, seed, scaleInv)


def test_a_cap_that_does_not_bind_gives_the_uncapped_bytes(mc, oracle, native):
    import torch
    g, r = _oracle_list(oracle, "mixed")
    kmax = int(ref.row_lengths(r["startIndexs"], len(r["packedNeighs"])).max())
    plain = _check(mc, oracle, native, "mixed", 0)
    for seed in (None, 3):
        loose = _check(mc, oracle, native, "mixed", kmax + 1, seed)
        for a, b in zip(plain, loose):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 2. large lists
@pytest.mark.parametrize("name", ["many_centres", "huge"])
def test_single_chain_large_lists(mc, oracle, native, name):
    """count, scan, fill; `huge`: with the visiting order of the geometry's own (>= 16 384 foreign centres)."""
    _, r = _oracle_list(oracle, name)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    assert int((k > 16).sum()) > 0 and (name != "huge" or (len(k) >= 16384 and 10 ** 6 < len(r["packedNeighs"]) < 4 * 10 ** 6))
    for seed in (None, 11):
        _check(mc, oracle, native, name, 16, seed)


# ------------------------------------------------------------------------------------------------- 3. usePDF=False, shared grid
def test_use_pdf_false(mc, oracle, native):
    for seed in (None, 5):
        _check(mc, oracle, native, "mixed", 16, seed, usePDF=False)


@pytest.mark.parametrize("owner_capped", [True, False], ids=["owner-capped", "owner-uncapped"])
def test_shared_grid_capped_and_uncapped(mc, oracle, native, owner_capped):
    """A geometry that shares a grid is capped or not independently of the grid's owner."""
    import torch
    g, _ = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, ("mixed", None))
    for seed in (None, 9):
        ko, ks = (16, 0) if owner_capped else (0, 16)
        owner = _build(native, g, h, ko, seed if ko else None)
        user = _build(native, g, h, ks, seed if ks else None, grid_from=owner)
        assert user.grid_owner is owner
        for geo, K in ((owner, ko), (user, ks)):
            sd = seed if K else None
            want_st, want_pk = _expect(oracle, "mixed", K, sd)
            st, pk, pdf = _arrays(geo)
            assert np.array_equal(_unwrap(st), want_st) and np.array_equal(_unwrap(pk), want_pk)
            bst, bpk, bpdf = _op_chain(mc, g, h, K, sd)
            assert torch.equal(st, bst) and torch.equal(pk, bpk) and torch.equal(pdf, bpdf)


# ------------------------------------------------------------------------------------------------- 4. batch form
def _launches():
    from mccnn_amd import _lib
    return int(_lib.load().mccnn_debug_launch_count())


def test_batch_form_mixes_uncapped_capped_and_sampled(mc, oracle, native):
    """One begin_batch() / end_batch() of 19 requests -- uncapped, capped and sampled ones over three geometries, a
    shared-grid pair among them, the chunk flush at 16 crossed: every array equals the single chain's byte for byte."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    specs = []   # (name, K, seed, shares the grid of spec #)
    for rep in range(2):
        specs += [("mixed", 0, None, None), ("mixed", 16, None, None), ("mixed", 16, 7 + rep, None), ("mid_windows", 16, None, None),
                  ("mid_windows", 5, 1 + rep, None), ("many_centres", 16, None, None), ("many_centres", 0, None, None),
                  ("many_centres", 16, 3 + rep, None), ("big_windows", 64, 5 + rep, None)]
    specs[1] = ("mixed", 16, None, 0)        # capped over the grid of an uncapped owner
    specs.append(("mixed", 0, None, 2))      # uncapped over the grid of a sampled owner
    assert len(specs) >= 17
    singles = {}
    for name, K, seed, _s in specs:
        if (name, K, seed) not in singles:
            g, _ = _oracle_list(oracle, name)
            singles[(name, K, seed)] = _arrays(_build(native, g, _inputs(mc, g, (name, None)), K, seed))
    torch.cuda.synchronize()
    geos = []
    native.begin_batch()
    try:
        for k, (name, K, seed, share) in enumerate(specs):
            g, _ = _oracle_list(oracle, name)
            geos.append(_build(native, g, _inputs(mc, g, (name, None)), K, seed, grid_from=(geos[share] if share is not None else None),
                               side=0, fork=(k == 0)))
    finally:
        native.end_batch()
    for (name, K, seed, share), geo in zip(specs, geos):
        want = singles[(name, K, seed)]
        got = _arrays(geo)
        want_st, want_pk = _expect(oracle, name, K, seed)
        assert geo.edges() == len(want_pk)
        assert np.array_equal(_unwrap(got[0]), want_st) and np.array_equal(_unwrap(got[1]), want_pk), (name, K, seed)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (name, K, seed, share)
    torch.cuda.synchronize()


def _capi_batch(g, h, caps, entry):
    """The requests `caps` -- (K, seed) each, every geometry over the `mixed` inputs with a grid of its own -- through one call
    of the C-ABI on the current stream: entry = "plain" (mccnn_geometry_build_batch; uncapped requests only), "null"
    (mccnn_geometry_build_batch_capped, caps == NULL) or "caps". -> (launches issued, edge totals)"""
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

    n, m = h["P"].shape[0], h["C"].shape[0]
    reqs, capv = (Request * len(caps))(), (Cap * len(caps))()
    keep = []
    for k, (K, seed) in enumerate(caps):
        ecap = m * K if K else 64 * m          # (the longest row of `mixed` has 59 hits: nothing overflows)
        nbytes = lib.mccnn_geometry_bytes_capped(n, m, g["B"], h["nc"], ecap, 1, K)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        slot = torch.empty(1, dtype=torch.int32).pin_memory()
        handle = lib.mccnn_geometry_create()
        keep.append((buf, slot, handle))
        reqs[k] = Request(handle, h["P"].data_ptr(), h["Bi"].data_ptr(), n, h["C"].data_ptr(), h["Cb"].data_ptr(), m,
                          h["mn"].data_ptr(), h["mx"].data_ptr(), g["B"], h["nc"], g["radius"], int(g["scaleInv"]), WINDOW, 1,
                          ecap, None, buf.data_ptr(), nbytes, slot.data_ptr())
        capv[k] = Cap(K, 0 if seed is None else 1, 0 if seed is None else seed)
    torch.cuda.synchronize()
    l0 = _launches()
    stream = _lib.stream_handle()
    if entry == "plain":
        assert all(K == 0 for K, _ in caps)
        rc = lib.mccnn_geometry_build_batch(C.addressof(reqs), len(caps), stream)
    else:
        rc = lib.mccnn_geometry_build_batch_capped(C.addressof(reqs), C.addressof(capv) if entry == "caps" else None, len(caps), stream)
    assert rc == 0
    torch.cuda.synchronize()
    launches = _launches() - l0
    totals = [int(slot[0]) for _buf, slot, _h in keep]
    for _buf, _slot, handle in keep:
        lib.mccnn_geometry_destroy(handle)
    return launches, totals


def test_batch_without_a_cap_issues_the_launches_it_issued_before(mc, oracle, native):
    """The launches of a batch, from the library's launch counter. The yardstick is what mccnn_geometry_build_batch itself issues
    for the same uncapped requests: the capped entry with caps == NULL, with caps that are all zero, and the extension's queued
    batch issue exactly as many. Capped and sampled requests in a chunk add one count pass (the two kinds share theirs) and one
    fill pass per kind; a chunk of capped requests alone issues the uncapped number."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    g, _ = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, ("mixed", None))
    plain = [(0, None)] * 5
    mixed = [(0, None), (16, None), (16, 3), (0, None), (8, None)]
    base, totals = _capi_batch(g, h, plain, "plain")
    print("launches of mccnn_geometry_build_batch over 5 uncapped requests:", base)
    assert base > 0 and totals == [len(_expect(oracle, "mixed", 0)[1])] * 5
    assert _capi_batch(g, h, plain, "null") == (base, totals)
    assert _capi_batch(g, h, plain, "caps") == (base, totals)
    got, totals = _capi_batch(g, h, mixed, "caps")
    assert got == base + 1 + 2 and totals == [len(_expect(oracle, "mixed", K, sd)[1]) for K, sd in mixed]
    assert _capi_batch(g, h, [(16, None)] * 3, "caps")[0] == base

    def queued(caps):   # the extension's begin_batch() / end_batch()
        for K, seed in caps:      # (the shapes' capacity guesses are learned: no rebuild inside the counted span)
            _build(native, g, h, K, seed).edges()
        torch.cuda.synchronize()
        l0 = _launches()
        native.begin_batch()
        try:
            geos = [_build(native, g, h, K, seed, side=0, fork=(k == 0)) for k, (K, seed) in enumerate(caps)]
        finally:
            native.end_batch()
        for geo in geos:
            assert geo.edges() <= geo.e_cap
        torch.cuda.synchronize()
        return _launches() - l0

    assert queued(plain) == base
    assert queued(mixed) == base + 1 + 2


# ------------------------------------------------------------------------------------------------- 5. capacity
def test_capacity_is_bounded_by_the_cap(mc, oracle, native):
    """The first geometry of a shape: capacity = min(m * K, the plain guess) -- m * K wherever that is smaller, and then the
    total arrives within it."""
    g, _ = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, ("mixed", None))
    native._EDGE_GUESS.clear()
    native._EDGE_RATIO.clear()
    for K, seed in ((16, None), (4, 2)):
        geo = _build(native, g, h, K, seed)
        assert geo.e_cap == geo.m * K            # (the plain guess is 48 per centre)
        assert 0 < geo.edges() <= geo.e_cap and geo.edges() == len(_expect(oracle, "mixed", K, seed)[1])
    # the capped totals have not touched the guess of the uncapped geometry of this shape
    assert _build(native, g, h).e_cap == 48 * len(g["centres"]) + 1024


def test_starved_guess_rebuilds_with_the_same_cap_and_seed(mc, oracle, native, monkeypatch):
    """ecap_scale (the MCCNN_DEBUG switch of the capacity guesses) far below 1: the capped list overflows the buffer and is
    rebuilt once with the exact size -- the same cap and seed, the same bytes."""
    import torch
    g, _ = _oracle_list(oracle, "mixed")
    h = _inputs(mc, g, ("mixed", None))
    for K, seed in ((16, None), (16, 21)):
        want = _arrays(_build(native, g, h, K, seed))
        native._EDGE_GUESS.clear()
        native._EDGE_RATIO.clear()
        monkeypatch.setattr(native, "_ECAP_SCALE", 0.02)
        geo = _build(native, g, h, K, seed)
        starved = geo.e_cap
        monkeypatch.setattr(native, "_ECAP_SCALE", 1.0)
        e = geo.edges()
        assert starved < e <= geo.e_cap and geo.cap == (K, seed)     # it did overflow, and was built again
        for a, b in zip(_arrays(geo), want):
            assert torch.equal(a, b)
        want_st, want_pk = _expect(oracle, "mixed", K, seed)
        assert np.array_equal(_unwrap(geo.neighbors()[1]), want_pk)
    native._EDGE_GUESS.clear()
    native._EDGE_RATIO.clear()


# ------------------------------------------------------------------------------------------------- 6. builder
def _pool_layer(oracle):
    """The layer of tests/test_gpu_neighbor_cap.py::test_builder_with_and_without_a_cap."""
    from mccnn_amd.MCConvBuilder import PointHierarchy
    g, _ = _oracle_list(oracle, "mixed")
    B, radius, K, fin, fout = g["B"], g["radius"], 16, 3, 8
    rng = np.random.default_rng(55)
    fs = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)
    P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
    ph = PointHierarchy(P, _wrap(fs), Bi, [0.2], "PHcap", B, True)
    w = make_mlp(conv_nb(fin, fout, True), 33)
    nb = conv_nb(fin, fout, True)
    state = {"c_weights": _wrap(w["w1"]), "c_biases": _wrap(w["b1"]), "c_weights2": _wrap(w["w2"]).reshape(nb, 8, 8),
             "c_biases2": _wrap(w["b2"]).reshape(nb, 8), "c_weights3": _wrap(w["w3"]).reshape(nb, 8, 8),
             "c_biases3": _wrap(w["b3"]).reshape(nb, 8)}
    return g, ph, fs, w, state, (B, radius, K, fin, fout)


@pytest.mark.parametrize("seed", [None, 7], ids=["canonical", "seed7"])
def test_builder_cap_native(mc, oracle, seed):
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    g, ph, fs, w, state, (B, radius, K, fin, fout) = _pool_layer(oracle)
    og = _wrap((2 * np.random.default_rng(56).random((ph.points_[1].shape[0], fout)) - 1).astype(np.float32))
    res = {}
    for cn in (True, False):
        cb = ConvolutionBuilder(KDEWindow=WINDOW, maxNeighbors=K, sampleSeed=seed, capNative=cn)
        assert cb.capNative_ is cn
        cb.load_state_dict(state)
        cb.opTrace_ = []
        F = _wrap(fs).requires_grad_(True)
        layer = lambda: cb.create_convolution("c", ph, 0, F, fin, radius, outPointLevel=1, multiFeatureConv=True, outNumFeatures=fout)
        out = layer()
        kG, kN0, kP0 = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True, K)
        kG, kN, kP = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True, K, seed)
        assert kN0.endswith("|16") and (seed is None or kN == kN0 + "|s7")
        assert ("find_neighbors", kN) in cb.opTrace_ and kN in cb.cacheNeighs_ and kP in cb.cachePDFs_
        if cn:
            assert list(cb.cacheGeo_) == [kP] and cb.cacheGeo_[kP].cap[0] == K     # filed under the capped key
        else:
            assert not cb.cacheGeo_ and isinstance(cb.cacheNeighs_[kN], tuple)       # as today
        lists = tuple(_unwrap(t) for t in cb.cacheNeighs_[kN])
        grads = torch.autograd.grad(out, [F] + [dict(cb.named_parameters())[n] for n in sorted(state)], og)
        res[cn] = (out.detach().clone(), [x.detach().clone() for x in grads], lists)
        if cn and seed is not None:   # sampleSeed_ reassigned + reset(): another output; the first seed again: the first bytes
            cb.sampleSeed_ = 8
            cb.reset()
            out8 = layer()
            assert list(cb.cacheGeo_) == [kP0 + "|s8"] and out8.shape == out.shape and not torch.equal(out8, out)
            cb.sampleSeed_ = seed
            cb.reset()
            assert torch.equal(layer(), out) and list(cb.cacheGeo_) == [kP]
    # the oracle's chain over the same two levels, over the capped / sampled list
    c1, cb1 = _unwrap(ph.points_[1]), _unwrap(ph.batchIds_[1])
    mn, mx = oracle.compute_aabb(g["pts"], g["bids"], B, True)
    keys, idx = oracle.sort_points_step1(g["pts"], g["bids"], mn, mx, B, radius, True)
    sp, sb, sf, cells = oracle.sort_points_step2(g["pts"], g["bids"], fs, keys, idx, mn, mx, B, radius, True)
    full = oracle.find_neighbors(c1, cb1, sp, cells, mn, mx, radius, B, True)
    if seed is None:
        st, pk = ref.cap_list(*full, K)
    else:
        st, pk = sref.sample_list(*full, K, (seed + zlib.crc32(kN0.encode())) & 0xFFFFFFFF)
    for cn in (True, False):
        assert np.array_equal(res[cn][2][0], st) and np.array_equal(res[cn][2][1], pk)
    pdfs = oracle.compute_pdf(sp, sb, mn, mx, st, pk, WINDOW, radius, B, True)
    want = oracle.spatial_conv(sp, sf, sb, pdfs, c1, st, pk, mn, mx, w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"],
                               fout, True, B, radius, True, True)
    assert_float_close(_unwrap(res[True][0]), want, RTOL, "native capped layer against the oracle")
    assert_float_close(_unwrap(res[True][0]), _unwrap(res[False][0]), RTOL, "native against op by op")
    for k, (a, b) in enumerate(zip(res[True][1], res[False][1])):
        assert_float_close(_unwrap(a).reshape(-1), _unwrap(b).reshape(-1), RTOL, "gradient %d (0 = features, then the variables by name)" % k)


# ------------------------------------------------------------------------------------------------- 7. prefetch
GRAPH = [  # name, lin, lout, fin, fout, combin, radius: six neighbour lists over four grids
    ("Conv_f1", 0, 0, 1, 16, True, 0.12), ("Conv_dw", 0, 0, 16, 16, False, 0.12), ("Pool_dw", 0, 1, 16, 16, False, 0.2),
    ("Pool_f1", 0, 1, 1, 8, True, 0.12), ("Conv_l1", 1, 1, 32, 32, False, 0.3), ("Up_dw", 1, 0, 16, 16, False, 0.3),
    ("Conv_3to8", 0, 0, 3, 8, True, 0.16),
]
K_GRAPH = 16


class _Net:
    """The graph above over batches of different sizes, every layer capped: feature rows and output gradients fixed per batch."""

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

    def step(self, cb, ci, ph=None, then=None):
        import torch
        cb.reset()
        if then is not None:
            then()
        ph = ph if ph is not None else self.hierarchy(ci)
        outs, fts = [], []
        for (name, lin, lout, fin, fout, combin, radius) in GRAPH:
            n = ph.points_[lin].shape[0]
            f = self.feats.setdefault((ci, name), 2 * torch.rand((n, fin), device="cuda") - 1).detach().clone().requires_grad_(True)
            fts.append(f)
            outs.append(cb.create_convolution(name, ph, lin, f, fin, radius, ph, lout, combin, fout))
        for k, o in enumerate(outs):
            self.ogs.setdefault((ci, k), 2 * torch.rand(o.shape, device="cuda") - 1)
        grads = torch.autograd.grad(outs, fts + list(cb.parameters()), [self.ogs[(ci, k)] for k in range(len(outs))], allow_unused=True)
        return [o.detach() for o in outs], [x for x in grads if x is not None]


def _builders(seed):
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    torch.manual_seed(1)
    run = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, maxNeighbors=K_GRAPH, sampleSeed=seed, capNative=True)
    quiet = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, maxNeighbors=K_GRAPH, sampleSeed=seed, capNative=True)
    quiet.geoPrefetch_ = False     # the reference: nothing runs ahead
    return run, quiet


def _sync_state(src, dst):
    dst.load_state_dict({k: v.detach().clone() for k, v in src.state_dict().items()})


def test_prefetch_geometry_with_a_cap(mc, oracle, native):
    """prefetch_geometry(..., maxNeighbors=16) under capNative: parked as a native geometry, installed by reset() under the
    capped key, the layer's output the bytes of a builder that prefetched nothing."""
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    g, ph, fs, w, state, (B, radius, K, fin, fout) = _pool_layer(oracle)
    F = _wrap(fs)
    outs = []
    for seed in (None, 7):
        for pre in (False, True):
            cb = ConvolutionBuilder(KDEWindow=WINDOW, capNative=True, sampleSeed=seed)
            cb.load_state_dict(state)
            if pre:
                cb.prefetch_geometry(ph, 0, radius, outPointLevel=1, maxNeighbors=K)
                assert len(cb.prefetchedGeo_) == 1 and cb.prefetched_ is None
                cb.reset()
                kP = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True, K, seed)[2]
                assert list(cb.cacheGeo_) == [kP]
                parked = cb.cacheGeo_[kP]
            out = cb.create_convolution("c", ph, 0, F, fin, radius, outPointLevel=1, multiFeatureConv=True, outNumFeatures=fout,
                                        maxNeighbors=K)
            if pre:
                assert cb.cacheGeo_[kP] is parked and parked.cap[0] == K
            outs.append(out.detach().clone())
        assert torch.equal(outs[-1], outs[-2])
    assert not torch.equal(outs[0], outs[2])


def test_learned_prefetch_step_with_a_seed(mc, native):
    """prefetch_step(ph, sampleSeed=s) over a graph of seven capped layers (six lists): the next step, run with seed s, finds
    its geometries parked and gives the outputs of a builder with nothing running ahead, bit for bit; a prefetch_step with the
    wrong seed is never asked for its geometries and the outputs are still those."""
    import torch
    from mccnn_amd.MCConvBuilder import _GEO_PREFETCH_MIN
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    assert len(set((l[1], l[2], l[6]) for l in GRAPH)) >= _GEO_PREFETCH_MIN
    net = _Net(((2500, 5), (1800, 6)))
    run, quiet = _builders(100)
    for ci in (1, 0):           # (both shapes seen: no list outgrows a capacity guessed from the other batch and is built again inline)
        net.step(run, ci)
    _sync_state(run, quiet)
    order = [0, 1, 1, 0, 1, 0]
    wrong = {3}                                     # the step BEFORE which the prefetch gets another seed
    nxt = None
    for s, ci in enumerate(order):
        seed = 100 + s
        quiet.sampleSeed_ = seed
        want = net.step(quiet, ci)
        torch.cuda.synchronize()
        run.sampleSeed_ = seed
        state = {}

        def start_next():
            if s + 1 < len(order):
                state["ph"] = net.hierarchy(order[s + 1])
                state["n"] = run.prefetch_step(state["ph"], sampleSeed=(seed + 1 if s + 1 not in wrong else seed + 50))
        got = net.step(run, ci, ph=nxt, then=start_next)
        sides = [geo.core.side for geo in run.cacheGeo_.values()]
        assert len(run.cacheGeo_) >= 6 and all(geo.cap[0] == K_GRAPH for geo in run.cacheGeo_.values())
        if s >= 1 and s not in wrong:
            assert all(sd >= 0 for sd in sides), (s, sides)          # every geometry of the step was started a step ago
        assert sum(1 for key in run.cacheGeo_ if key.endswith("|%d|s%d" % (K_GRAPH, seed))) == 6   # the capped keys of this seed
        if s + 1 < len(order) and s >= 1:
            assert state["n"] == 6
        nxt = state.get("ph")
        for a, b in zip(got[0], want[0]):
            assert torch.equal(a, b), s
        for a, b in zip(got[1], want[1]):   # (feature gradients of one-feature layers are summed with float atomics)
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- soak
def test_soak_capped_pipelined_loop(mc, native):
    """The loop of tools/soak_network.py in short: batches of different sizes in random order, every layer capped, the seed
    another one every step, the next batch's geometries started by prefetch_step under the current step -- and no host
    synchronisation inside the loop. Outputs are compared on the GPU with references computed with nothing running ahead."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    net = _Net(((2500, 5), (1200, 6), (3200, 7), (700, 8)))
    run, quiet = _builders(0)
    net.step(run, 0)
    _sync_state(run, quiet)
    steps = 40
    order = np.random.default_rng(7).integers(0, len(net.clouds), steps)
    refs = []
    for s in range(steps):
        quiet.sampleSeed_ = s
        refs.append(net.step(quiet, int(order[s])))
    torch.cuda.synchronize()
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    worst = torch.zeros((), dtype=torch.float32, device="cuda")
    nxt = None
    for s in range(steps):
        run.sampleSeed_ = s
        state = {}

        def start_next():
            if s + 1 < steps:
                state["ph"] = net.hierarchy(int(order[s + 1]))
                run.prefetch_step(state["ph"], sampleSeed=s + 1)
        outs, grads = net.step(run, int(order[s]), ph=nxt, then=start_next)
        nxt = state.get("ph")
        for o, r in zip(outs, refs[s][0]):
            bad += (o != r).sum()
        for a, b in zip(grads, refs[s][1]):
            worst = torch.maximum(worst, (a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    torch.cuda.synchronize()
    print("soak: %d steps, forward mismatches %d, worst relative gradient deviation %.2e" % (steps, int(bad), float(worst)))
    assert int(bad) == 0 and float(worst) < 1e-4


# ------------------------------------------------------------------------------------------------- 8. ctypes binding
def test_ctypes_binding_inner(mc, oracle, native):
    """(run by test_ctypes_binding in a child process with MCCNN_TORCH_EXT=0; with the extension loaded it checks that one)"""
    for name, K, seed in (("mixed", 16, None), ("big_windows", 64, 13)):
        _check(mc, oracle, native, name, K, seed)


def test_ctypes_binding():
    """One capped and one sampled geometry through the ctypes binding of the C-ABI (mccnn_geometry_build_capped)."""
    env = dict(os.environ, MCCNN_TORCH_EXT="0")
    code = ("import sys, pytest; from mccnn_amd import native; assert native._EXT is None; "
            "sys.exit(pytest.main([%r, '-m', 'gpu', '-x', '-q', '-k', 'test_ctypes_binding_inner']))"
            % os.path.join(ROOT, "tests", "test_gpu_native_cap.py"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
