"""Per-point densities (pdfMode='point') through the native step executor: mccnn_geometry_build_point / _build_batch_point,
native.build_geometry(pointPDF=True), ConvolutionBuilder(pdfMode='point', pointNative=True).

Every array has two references: (a) tests/point_pdf_ref.py over the oracle's rows -- density_ref, then expand_ref -- at the
project's 1e-4 (norm-wise and per element), counts, startIndexs and packedNeighs exact; (b) the HIP op chain build_grid ->
find_neighbors -> compute_pdf_points -> expand_pdf, bit for bit.

Geometries: small_clouds() of tests/point_pdf_ref.py (a one-point cloud: R = 0 under the relative radius); `mixed` (<= 4096
centres: the two-launch search chain) and `many_centres` (5000: count, scan, fill) of tests/neighbor_cap_ref.py; `huge` below
(20 000 points: the single sweep runs four points per wave; 17 000 foreign centres: a visiting order of the geometry's own,
whose workspace shares the head of the chain with the sweep); one cloud of 9000 and one of 40 000 points, which cross the
thresholds of two and eight points per wave."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import neighbor_cap_ref as ref
from tests import neighbor_sample_ref as sref
from tests import point_pdf_ref as pref
from tests.helpers import make_mlp, conv_nb, assert_float_close, make_cloud

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's bar for float outputs (norm-wise and per element: tests/helpers.py)
WINDOW = 0.2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ORACLE = {}   # (geometry name, scaleInv, own centres) -> (geometry, the oracle's chain + reference (a)): computed once, never modified
_GPU = {}      # the same key -> device tensors of the inputs (points, boxes, cell count)
_OPS = {}      # (key, window) -> reference (b)


def geom_huge():
    """Two uniform clouds of 10 000 points each, absolute radius 0.12; centres = a shuffled subset of 17 000 points: more than
    the 16 384 from which a geometry over foreign centres builds a visiting order of its own. ~1.2 M uncapped edges."""
    rng = np.random.default_rng(105)
    pts, bids = ref._two_clouds(rng, (10000, 10000))
    sel = rng.permutation(len(pts))[:17000]
    return dict(pts=pts, bids=bids, centres=np.ascontiguousarray(pts[sel]), cbids=np.ascontiguousarray(bids[sel]), B=2,
                radius=0.12, scaleInv=False)


def geom_small_abs():
    pts, bids, B, _sizes = pref.small_clouds()
    return dict(pts=pts, bids=bids, centres=pts, cbids=bids, B=B, radius=0.1, scaleInv=False)


def geom_small_rel():
    return dict(geom_small_abs(), radius=2.0, scaleInv=True)


GEOMS = dict(ref.GEOMETRIES, huge=geom_huge, small_abs=geom_small_abs, small_rel=geom_small_rel)


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _case(oracle, name, scaleInv=None, own=False, window=WINDOW):
    """-> (key, geometry, r): r = the oracle's uncapped chain plus reference (a): density (float64), counts, pdfs."""
    key = (name, scaleInv, own)
    if key not in _ORACLE:
        g = GEOMS[name]()
        if scaleInv is not None:
            g = dict(g, scaleInv=scaleInv)
        if own:
            g = dict(g, centres=g["pts"], cbids=g["bids"])
        _ORACLE[key] = (g, ref.uncapped(oracle, g), {})
    g, r, dens = _ORACLE[key]
    if window not in dens:
        d, c = pref.density_ref(oracle, r["sortPts"], r["sortBatchs"], r["cellIndexs"], r["aabbMin"], r["aabbMax"], window,
                                g["radius"], g["B"], g["scaleInv"])
        dens[window] = (d, c, pref.expand_ref(d, r["startIndexs"], r["packedNeighs"]))
    return key, g, dict(r, density=dens[window][0], counts=dens[window][1], pdfs=dens[window][2])


def _inputs(mc, g, key):
    if key not in _GPU:
        P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
        mn, mx = mc.compute_aabb(P, Bi, g["B"], g["scaleInv"])
        nc = mc._num_cells(mn, mx, g["B"], g["radius"], g["scaleInv"])
        own = g["centres"] is g["pts"]     # (the points as their own centres: the SAME tensors, as a same-level layer passes them)
        _GPU[key] = dict(P=P, Bi=Bi, C=(P if own else _wrap(g["centres"])), Cb=(Bi if own else _wrap(g["cbids"])), mn=mn, mx=mx, nc=nc)
    return _GPU[key]


def _build(native, g, h, point=True, K=0, seed=None, grid_from=None, side=-1, fork=False, window=WINDOW, centres=None):
    C, Cb = (h["C"], h["Cb"]) if centres is None else centres
    return native.build_geometry(h["P"], h["Bi"], C, Cb, h["mn"], h["mx"], g["B"], h["nc"], g["radius"], g["scaleInv"],
                                 window, True, grid_from=grid_from, side=side, fork=fork, maxNeighbors=K, sampleSeed=seed,
                                 pointPDF=point)


def _op_chain(mc, g, h, key, window=WINDOW, centres=None):
    """Reference (b): the HIP ops one by one -> (startIndexs, packedNeighs, pdfs, density, counts)"""
    ck = (key, window, None if centres is None else centres[0].data_ptr())
    if ck not in _OPS:
        C, Cb = (h["C"], h["Cb"]) if centres is None else centres
        sP, sB, cells, _idx, _inv = mc.build_grid(h["P"], h["Bi"], h["mn"], h["mx"], g["B"], g["radius"], g["scaleInv"])
        st, pk = mc.find_neighbors(C, Cb, sP, cells, h["mn"], h["mx"], g["radius"], g["B"], g["scaleInv"])
        d, c = mc.compute_pdf_points(sP, sB, cells, h["mn"], h["mx"], window, g["radius"], g["B"], g["scaleInv"])
        _OPS[ck] = (st, pk, mc.expand_pdf(d, st, pk), d, c)
    return _OPS[ck]


def _arrays(geo):
    st, pk = geo.neighbors()
    d, c = geo.point_density()
    return st, pk, geo.pdfs(), d, c


def _against_a(arrays, r, what):
    """reference (a): lists and counts exact, density and PDFs at the project's bar"""
    st, pk, pdf, d, c = arrays
    assert np.array_equal(_unwrap(st), r["startIndexs"]) and np.array_equal(_unwrap(pk), r["packedNeighs"]), what
    assert np.array_equal(_unwrap(c), r["counts"]), what
    assert_float_close(_unwrap(d), r["density"], RTOL, what + ": density")
    assert_float_close(_unwrap(pdf), r["pdfs"], RTOL, what + ": pdfs")


def _equal(a, b, what=""):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, k)


def _check(mc, oracle, native, name, scaleInv=None, own=False):
    """One point geometry through the single chain against (a) and (b). -> (geometry, its arrays)"""
    key, g, r = _case(oracle, name, scaleInv, own)
    h = _inputs(mc, g, key)
    geo = _build(native, g, h)
    got = _arrays(geo)
    print(name, "scaleInv", g["scaleInv"], "own", own, "n", geo.n, "m", geo.m, "E", geo.edges(), "capacity", geo.e_cap)
    assert geo.point and geo.edges() == len(r["packedNeighs"]) and geo.edges() <= geo.e_cap
    _against_a(got, r, name)
    _equal(got, _op_chain(mc, g, h, key), name)
    return geo, got


@pytest.fixture(scope="module")
def native(mc):
    from mccnn_amd import native as nat
    return nat


def _launches():
    from mccnn_amd import _lib
    return int(_lib.load().mccnn_debug_launch_count())


# ------------------------------------------------------------------------------------------------- 1. single chain
@pytest.mark.parametrize("name", ["small_abs", "small_rel"])
def test_small_clouds(mc, oracle, native, name):
    """128 points in three clouds, one of a single point: under the relative radius its R is 0 -- an empty ball, counts 0,
    density 0. The other clouds lie inside all their balls: there the result is also the oracle's compute_pdf."""
    geo, (st, pk, pdf, d, c) = _check(mc, oracle, native, name)
    key, g, r = _case(oracle, name)
    sizes = np.asarray(pref.small_clouds()[3])
    b = r["sortBatchs"].reshape(-1)
    want = sizes[b]
    if g["scaleInv"]:
        want = np.where(want == 1, 0, want)
        assert float(_unwrap(d)[b == 1, 0][0]) == 0.0 and int(_unwrap(c)[b == 1, 0][0]) == 0
    assert np.array_equal(_unwrap(c).reshape(-1), want)
    edge = oracle.compute_pdf(r["sortPts"], r["sortBatchs"], r["aabbMin"], r["aabbMax"], r["startIndexs"], r["packedNeighs"],
                              WINDOW, g["radius"], g["B"], g["scaleInv"])
    assert_float_close(_unwrap(pdf), edge, RTOL, "against the oracle's compute_pdf")


@pytest.mark.parametrize("scaleInv,own", [(None, False), (False, False), (None, True), (False, True)],
                         ids=["rel", "abs", "rel-own", "abs-own"])
def test_mixed(mc, oracle, native, scaleInv, own):
    """<= 4096 centres: count, then the fill pass that scans the counts itself and publishes the total the expansion reads."""
    geo, (st, pk, pdf, d, c) = _check(mc, oracle, native, "mixed", scaleInv, own)
    if own:   # the same-level list: the row of centre i is the ball of point i
        k = np.diff(np.append(_unwrap(st).reshape(-1), geo.edges()))
        idx = _unwrap(geo.grid()[3]).reshape(-1).astype(np.int64)        # original index -> sorted position
        assert np.array_equal(np.sort(idx), np.arange(geo.n)) and np.array_equal(_unwrap(geo.grid()[0])[idx], _unwrap(geo.args[0]))
        assert np.array_equal(k, _unwrap(c).reshape(-1)[idx])


def test_many_centres(mc, oracle, native):
    """5000 centres: count, scan, fill"""
    _check(mc, oracle, native, "many_centres")


def test_huge_with_a_visiting_order(mc, oracle, native):
    """20 000 points: four points per wave in the single sweep; 17 000 foreign centres: the geometry sorts a visiting order of
    its own behind the sweep, from a workspace cleared at the head of the chain."""
    geo, _ = _check(mc, oracle, native, "huge")
    assert 16384 <= geo.n < 32768 and geo.m >= 16384


# ------------------------------------------------------------------------------------------------- 2. points per wave
def test_density_does_not_depend_on_the_points_per_wave(mc, native):
    """One cloud of 9000 points (two per wave alone) and one of 40 000 (eight): the single form, the batch form -- which takes
    ONE group size from all its points -- and the op give the same density and counts, bit for bit."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    clouds = []
    for n, seed, radius in ((9000, 41, 0.1), (40000, 42, 0.05)):
        pts, bids = make_cloud(n, 1, seed, "clustered")
        assert len(pts) == n
        sel = np.random.default_rng(seed).permutation(n)[:64]
        g = dict(pts=pts, bids=bids, centres=np.ascontiguousarray(pts[sel]), cbids=np.ascontiguousarray(bids[sel]), B=1,
                 radius=radius, scaleInv=True)
        h = _inputs(mc, g, ("cloud", n))
        sP, sB, cells, _i, _v = mc.build_grid(h["P"], h["Bi"], h["mn"], h["mx"], 1, radius, True)
        clouds.append((g, h, mc.compute_pdf_points(sP, sB, cells, h["mn"], h["mx"], WINDOW, radius, 1, True)))
    singles = []
    for g, h, op in clouds:
        geo = _build(native, g, h)
        _equal(geo.point_density(), op, "single")
        assert int(op[1].min()) >= 1 and int(op[1].max()) > 256      # (more candidates than one staged segment)
        singles.append(geo)
    for subset in ((0,), (1,), (0, 1)):
        native.begin_batch()
        try:
            geos = [_build(native, clouds[k][0], clouds[k][1], side=0, fork=(j == 0)) for j, k in enumerate(subset)]
        finally:
            native.end_batch()
        for k, geo in zip(subset, geos):
            _equal(geo.point_density(), clouds[k][2], "batch %s" % (subset,))
            _equal((geo.pdfs(),) + tuple(geo.neighbors()), (singles[k].pdfs(),) + tuple(singles[k].neighbors()))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 3. sharing
def test_sharing_one_density_per_grid_and_window(mc, oracle, native):
    import torch
    key, g, r = _case(oracle, "mixed")
    h = _inputs(mc, g, key)
    okey, og_, orr = _case(oracle, "mixed", None, True)            # the same points as their own centres: another list
    own = (h["P"], h["Bi"])
    # (capacity guesses of both shapes learned: no rebuild inside the counted spans)
    for cen in (None, own):
        _build(native, g, h, centres=cen).edges()
        _build(native, g, h, point=False, centres=cen).edges()
    torch.cuda.synchronize()
    deltas = {}
    for point in (True, False):
        owner = _build(native, g, h, point=point)
        torch.cuda.synchronize()
        l0 = _launches()
        sharer = _build(native, g, h, point=point, grid_from=owner, centres=own)
        torch.cuda.synchronize()
        deltas[point] = _launches() - l0
        assert sharer.grid_owner is owner
        if point:
            # no density sweep in the sharer's chain, and the pair is the owner's
            assert sharer.point_density()[0] is owner.point_density()[0] and sharer.point_density()[1] is owner.point_density()[1]
            _against_a(_arrays(owner), r, "owner")
            _against_a(_arrays(sharer), orr, "sharer")
            _equal(_arrays(sharer), _op_chain(mc, g, h, key, centres=own), "sharer")
            # another window: a second pair, computed by the sharer that asks for it first
            other = _build(native, g, h, grid_from=owner, centres=own, window=0.35)
            _k, _g, r35 = _case(oracle, "mixed", None, True, window=0.35)
            assert other.point_density()[0] is not owner.point_density()[0]
            assert other.point_density()[0] is owner.point_density(0.35)[0] and sorted(owner.pointPairs) == [WINDOW, 0.35]
            _against_a(_arrays(other), r35, "window 0.35")
            _equal(_arrays(other), _op_chain(mc, g, h, key, window=0.35, centres=own), "window 0.35")
    print("launches of a sharer's chain: point", deltas[True], "edge", deltas[False])
    assert deltas[True] == deltas[False] > 0
    # the modes of owner and sharer are independent: edge over a point owner, point over an edge owner
    for owner_point in (True, False):
        owner = _build(native, g, h, point=owner_point)
        sharer = _build(native, g, h, point=not owner_point, grid_from=owner, centres=own)
        for geo, cen, rr in ((owner, None, r), (sharer, own, orr)):
            if geo.point:
                _against_a(_arrays(geo), rr, "mixed modes")
                _equal(_arrays(geo), _op_chain(mc, g, h, key, centres=cen), "mixed modes")
            else:
                st, pk = geo.neighbors()
                C, Cb = (h["C"], h["Cb"]) if cen is None else cen
                sP, sB, cells, _i, _v = mc.build_grid(h["P"], h["Bi"], h["mn"], h["mx"], g["B"], g["radius"], g["scaleInv"])
                bst, bpk = mc.find_neighbors(C, Cb, sP, cells, h["mn"], h["mx"], g["radius"], g["B"], g["scaleInv"])
                bpdf = mc.compute_pdf(sP, sB, h["mn"], h["mx"], bst, bpk, WINDOW, g["radius"], g["B"], g["scaleInv"])
                _equal((st, pk, geo.pdfs()), (bst, bpk, bpdf), "edge mode beside a point geometry")
                assert np.array_equal(_unwrap(pk), rr["packedNeighs"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 4. batch form
def test_batch_form_mixes_edge_point_capped_and_sampled(mc, oracle, native):
    """One begin_batch() / end_batch() of 19 requests over three geometries -- edge, point, capped and sampled ones, two point
    requests in one chunk that share a density, and a point sharer behind the chunk flush at 16 whose density was computed
    before it: every array equals the single chain's byte for byte, and reference (a)."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    # (name, mode, K, seed, shares the grid of spec #)
    specs = [("mixed", "edge", 0, None, None), ("mixed", "edge", 16, None, None), ("mixed", "point", 0, None, None),
             ("mixed", "point", 0, None, 2), ("many_centres", "point", 0, None, None), ("many_centres", "edge", 0, None, None),
             ("many_centres", "edge", 16, 3, None), ("mid_windows", "point", 0, None, None), ("mid_windows", "edge", 5, 1, None),
             ("mid_windows", "edge", 0, None, 7), ("mixed", "edge", 0, None, 2), ("mixed", "point", 0, None, 0),
             ("many_centres", "point", 0, None, 5), ("mid_windows", "edge", 16, None, None), ("mixed", "edge", 16, 7, None),
             ("many_centres", "edge", 16, None, None),
             # ---- behind the flush at 16
             ("mixed", "point", 0, None, 2), ("many_centres", "point", 0, None, 4), ("mid_windows", "point", 0, None, None)]
    assert len(specs) >= 17
    singles = {}
    for name, mode, K, seed, _s in specs:
        if (name, mode, K, seed) not in singles:
            key, g, _r = _case(oracle, name)
            geo = _build(native, g, _inputs(mc, g, key), mode == "point", K, seed)
            singles[(name, mode, K, seed)] = _arrays(geo) if mode == "point" else (geo.neighbors() + (geo.pdfs(),))
    torch.cuda.synchronize()
    geos = []
    native.begin_batch()
    try:
        for k, (name, mode, K, seed, share) in enumerate(specs):
            key, g, _r = _case(oracle, name)
            geos.append(_build(native, g, _inputs(mc, g, key), mode == "point", K, seed,
                               grid_from=(geos[share] if share is not None else None), side=0, fork=(k == 0)))
    finally:
        native.end_batch()
    for (name, mode, K, seed, share), geo in zip(specs, geos):
        _key, g, r = _case(oracle, name)
        want = singles[(name, mode, K, seed)]
        if mode == "point":
            got = _arrays(geo)
            _against_a(got, r, "%s in the batch" % name)
        else:
            got = geo.neighbors() + (geo.pdfs(),)
            if K == 0:
                wst, wpk = r["startIndexs"], r["packedNeighs"]
            elif seed is None:
                wst, wpk = ref.cap_list(r["startIndexs"], r["packedNeighs"], K)
            else:
                wst, wpk = sref.sample_list(r["startIndexs"], r["packedNeighs"], K, seed)
            assert np.array_equal(_unwrap(got[0]), wst) and np.array_equal(_unwrap(got[1]), wpk), (name, mode, K, seed)
        _equal(got, want, (name, mode, K, seed, share))
    # the sharers hold their owners' pairs
    assert geos[3].point_density()[0] is geos[2].point_density()[0] and geos[16].point_density()[0] is geos[2].point_density()[0]
    assert geos[11].point_density()[0] is geos[0].point_density()[0] and geos[12].point_density()[0] is geos[5].point_density()[0]
    assert geos[17].point_density()[0] is geos[4].point_density()[0] and geos[18].point_density()[0] is not geos[7].point_density()[0]
    torch.cuda.synchronize()


def _capi_batch(g, h, modes, entry="point"):
    """The requests `modes` -- "edge", "point" (a density of its own, not ready), "ready" (a density of its own, said to be there)
    or ("share", k) (the density of request k, not ready) each, every geometry over the `mixed` inputs with a grid of its own --
    through one call of the C-ABI on the current stream: entry = "plain" (mccnn_geometry_build_batch), "null"
    (mccnn_geometry_build_batch_point, points == NULL) or "point". -> (launches issued, edge totals, densities)"""
    import ctypes as C
    import torch
    from mccnn_amd import _lib, native
    lib = _lib.load()

    class Request(C.Structure):   # mccnn_geometry_request (include/mccnn.h)
        _fields_ = [("geometry", C.c_void_p), ("pts", C.c_void_p), ("batch_ids", C.c_void_p), ("n", C.c_int),
                    ("centres", C.c_void_p), ("centre_batch_ids", C.c_void_p), ("m", C.c_int), ("aabb_min", C.c_void_p),
                    ("aabb_max", C.c_void_p), ("batch_size", C.c_int), ("num_cells", C.c_int), ("radius", C.c_float),
                    ("scale_inv", C.c_int), ("window", C.c_float), ("use_pdf", C.c_int), ("e_capacity", C.c_int),
                    ("grid_from", C.c_void_p), ("buffer", C.c_void_p), ("buffer_bytes", C.c_size_t), ("total_host", C.c_void_p)]

    n, m = h["P"].shape[0], h["C"].shape[0]
    reqs, ptv = (Request * len(modes))(), (native._PointPdf * len(modes))()
    keep, dens = [], []
    for k, mode in enumerate(modes):
        ecap = 64 * m          # (the longest row of `mixed` has 59 hits: nothing overflows)
        nbytes = lib.mccnn_geometry_bytes(n, m, g["B"], h["nc"], ecap, 1)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        slot = torch.empty(1, dtype=torch.int32).pin_memory()
        handle = lib.mccnn_geometry_create()
        keep.append((buf, slot, handle))
        reqs[k] = Request(handle, h["P"].data_ptr(), h["Bi"].data_ptr(), n, h["C"].data_ptr(), h["Cb"].data_ptr(), m,
                          h["mn"].data_ptr(), h["mx"].data_ptr(), g["B"], h["nc"], g["radius"], int(g["scaleInv"]), WINDOW, 1,
                          ecap, None, buf.data_ptr(), nbytes, slot.data_ptr())
        if mode == "edge":
            dens.append(None)
            ptv[k] = native._PointPdf(None, None, 0)
        elif isinstance(mode, tuple):
            dens.append(dens[mode[1]])
            ptv[k] = native._PointPdf(dens[k][0].data_ptr(), dens[k][1].data_ptr(), 0)
        else:
            dens.append((torch.zeros((n, 1), dtype=torch.float32, device="cuda"), torch.zeros((n, 1), dtype=torch.int32, device="cuda")))
            ptv[k] = native._PointPdf(dens[k][0].data_ptr(), dens[k][1].data_ptr(), 1 if mode == "ready" else 0)
    torch.cuda.synchronize()
    l0 = _launches()
    stream = _lib.stream_handle()
    if entry == "plain":
        assert all(md == "edge" for md in modes)
        rc = lib.mccnn_geometry_build_batch(C.addressof(reqs), len(modes), stream)
    else:
        rc = lib.mccnn_geometry_build_batch_point(C.addressof(reqs), None, C.addressof(ptv) if entry == "point" else None, len(modes), stream)
    assert rc == 0
    torch.cuda.synchronize()
    launches = _launches() - l0
    totals = [int(slot[0]) for _buf, slot, _h in keep]
    for _buf, _slot, handle in keep:
        lib.mccnn_geometry_destroy(handle)
    return launches, totals, dens


def test_launches_of_a_batch_with_point_requests(mc, oracle, native):
    """From the library's launch counter. The yardstick is what mccnn_geometry_build_batch issues for the same requests in edge
    mode; the point entry without records, or with records that are all null, issues exactly as many. A chunk of point requests
    alone: one more (the sweep and the expansion in the place of the KDE); with every density ready: as many; edge and point
    requests mixed: two more. A density named by several requests is swept once. The extension's queued batch: the same."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    key, g, r = _case(oracle, "mixed")
    h = _inputs(mc, g, key)
    E = len(r["packedNeighs"])
    base, totals, _d = _capi_batch(g, h, ["edge"] * 5, "plain")
    print("launches of mccnn_geometry_build_batch over 5 edge requests:", base)
    assert base > 0 and totals == [E] * 5
    assert _capi_batch(g, h, ["edge"] * 5, "null")[:2] == (base, totals)
    assert _capi_batch(g, h, ["edge"] * 5, "point")[:2] == (base, totals)
    got, tt, dens = _capi_batch(g, h, ["point"] * 5)
    assert (got, tt) == (base + 1, totals)
    for d, c in dens:      # every density was computed: reference (a)
        assert np.array_equal(_unwrap(c), r["counts"])
        assert_float_close(_unwrap(d), r["density"], RTOL, "density of a batch item")
    assert _capi_batch(g, h, ["ready"] * 5)[:2] == (base, totals)
    assert _capi_batch(g, h, ["edge", "point", "edge", "point", "edge"])[:2] == (base + 2, totals)
    # one density for three requests (the first computes it), beside one of its own: still one sweep launch, both computed
    got, tt, dens = _capi_batch(g, h, ["point", ("share", 0), "point", ("share", 0), "edge"])
    assert (got, tt) == (base + 2, totals)
    for k in (0, 2):
        assert np.array_equal(_unwrap(dens[k][1]), r["counts"])

    def queued(modes):   # the extension's begin_batch() / end_batch()
        for md in set(modes):      # (the shape's capacity guess is learned: no rebuild inside the counted span)
            _build(native, g, h, md == "point").edges()
        torch.cuda.synchronize()
        l0 = _launches()
        native.begin_batch()
        try:
            geos = [_build(native, g, h, md == "point", side=0, fork=(k == 0)) for k, md in enumerate(modes)]
        finally:
            native.end_batch()
        for geo in geos:
            assert geo.edges() <= geo.e_cap
        torch.cuda.synchronize()
        return _launches() - l0

    assert queued(["edge"] * 5) == base
    assert queued(["point"] * 5) == base + 1
    assert queued(["edge", "point", "edge", "point", "edge"]) == base + 2


# ------------------------------------------------------------------------------------------------- 5. overflow
def test_starved_guess_rebuilds_in_point_mode_without_a_second_sweep(mc, oracle, native, monkeypatch):
    """ecap_scale (the MCCNN_DEBUG switch of the capacity guesses) far below 1: the list overflows the buffer -- the expansion
    then stops at the capacity -- and is rebuilt once with the exact size: the same mode, the same pair, the same bytes, and
    the launches of an edge geometry's rebuild (an expansion in the place of the KDE, no sweep)."""
    import torch
    key, g, r = _case(oracle, "mixed")
    h = _inputs(mc, g, key)
    want = _arrays(_build(native, g, h))
    deltas = {}
    for point in (True, False):
        native._EDGE_GUESS.clear()
        native._EDGE_RATIO.clear()
        monkeypatch.setattr(native, "_ECAP_SCALE", 0.02)
        geo = _build(native, g, h, point=point)
        starved = geo.e_cap
        monkeypatch.setattr(native, "_ECAP_SCALE", 1.0)
        pair = geo.point_density() if point else None
        torch.cuda.synchronize()
        l0 = _launches()
        e = geo.edges()
        torch.cuda.synchronize()
        deltas[point] = _launches() - l0
        assert starved < e <= geo.e_cap and geo.point is point          # it did overflow, and was built again
        if point:
            assert geo.point_density()[0] is pair[0] and geo.point_density()[1] is pair[1]
            _equal(_arrays(geo), want, "rebuilt")
            _against_a(_arrays(geo), r, "rebuilt")
    print("launches of a rebuild: point", deltas[True], "edge", deltas[False])
    assert deltas[True] == deltas[False] > 0
    native._EDGE_GUESS.clear()
    native._EDGE_RATIO.clear()


# ------------------------------------------------------------------------------------------------- 6. builder
def _pool_layer(oracle):
    """The layer of tests/test_gpu_native_cap.py::_pool_layer"""
    from mccnn_amd.MCConvBuilder import PointHierarchy
    _key, g, _r = _case(oracle, "mixed")
    B, radius, fin, fout = g["B"], g["radius"], 3, 8
    rng = np.random.default_rng(55)
    fs = (2 * rng.random((len(g["pts"]), fin)) - 1).astype(np.float32)
    P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
    ph = PointHierarchy(P, _wrap(fs), Bi, [0.2], "PHpt", B, True)
    w = make_mlp(conv_nb(fin, fout, True), 33)
    nb = conv_nb(fin, fout, True)
    state = {"c_weights": _wrap(w["w1"]), "c_biases": _wrap(w["b1"]), "c_weights2": _wrap(w["w2"]).reshape(nb, 8, 8),
             "c_biases2": _wrap(w["b2"]).reshape(nb, 8), "c_weights3": _wrap(w["w3"]).reshape(nb, 8, 8),
             "c_biases3": _wrap(w["b3"]).reshape(nb, 8)}
    return g, ph, fs, w, state, (B, radius, fin, fout)


def test_builder_point_native(mc, oracle):
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    g, ph, fs, w, state, (B, radius, fin, fout) = _pool_layer(oracle)
    rng = np.random.default_rng(56)
    og_np = (2 * rng.random((ph.points_[1].shape[0], fout)) - 1).astype(np.float32)
    og = _wrap(og_np)
    res = {}
    for pn in (True, False):
        cb = ConvolutionBuilder(KDEWindow=WINDOW, pdfMode='point', pointNative=pn)
        assert cb.pointNative_ is pn
        cb.load_state_dict(state)
        cb.opTrace_ = []
        F = _wrap(fs).requires_grad_(True)
        out = cb.create_convolution("c", ph, 0, F, fin, radius, outPointLevel=1, multiFeatureConv=True, outNumFeatures=fout)
        kG, kN, kP = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True)
        kD = kG + '|' + str(WINDOW)
        pick = [t for t in cb.opTrace_ if t[0] in ("find_neighbors", "compute_pdf_points", "expand_pdf", "compute_pdf")]
        assert pick == [("find_neighbors", kN), ("compute_pdf_points", kD), ("expand_pdf", kP + "|pt")]
        assert list(cb.cachePDFs_) == [kP + "|pt"] and list(cb.cacheNeighs_) == [kN] and list(cb.cachePointPDFs_) == [kD]
        if pn:
            assert list(cb.cacheGeo_) == [kP + "|pt"] and cb.cacheGeo_[kP + "|pt"].point      # filed under the point key
        else:
            assert not cb.cacheGeo_ and isinstance(cb.cacheNeighs_[kN], tuple)                  # as today
        # a second layer over the same grid and window, another list: no second density
        torch.manual_seed(9)      # (the variables of "c2" are created here: the same ones in both builders)
        out2 = cb.create_convolution("c2", ph, 0, F, fin, radius, multiFeatureConv=True, outNumFeatures=fout)
        assert [t[0] for t in cb.opTrace_].count("compute_pdf_points") == 1 and [t[0] for t in cb.opTrace_].count("expand_pdf") == 2
        assert len(cb.cachePointPDFs_) == 1 and (not pn or len(cb.cacheGeo_) == 2)
        lists = tuple(_unwrap(t) for t in cb.cacheNeighs_[kN])
        pdfs = _unwrap(cb.cachePDFs_[kP + "|pt"].reshape(-1, 1))
        dens = tuple(_unwrap(t) for t in cb.cachePointPDFs_[kD])
        grads = torch.autograd.grad(out, [F] + [dict(cb.named_parameters())[n] for n in sorted(state)], og)
        res[pn] = (out.detach().clone(), [x.detach().clone() for x in grads], lists, pdfs, dens, out2.detach().clone())
    # both give the same lists, and the bytes of densities and PDFs
    for a, b in zip(res[True][2] + (res[True][3],) + res[True][4], res[False][2] + (res[False][3],) + res[False][4]):
        assert a.tobytes() == b.tobytes()
    assert_float_close(_unwrap(res[True][5]), _unwrap(res[False][5]), RTOL, "second layer over the shared density")
    # the oracle's chain over the same two levels, with reference (a) for the PDFs
    c1, cb1 = _unwrap(ph.points_[1]), _unwrap(ph.batchIds_[1])
    mn, mx = oracle.compute_aabb(g["pts"], g["bids"], B, True)
    keys, idx = oracle.sort_points_step1(g["pts"], g["bids"], mn, mx, B, radius, True)
    sp, sb, sf, cells = oracle.sort_points_step2(g["pts"], g["bids"], fs, keys, idx, mn, mx, B, radius, True)
    st, pk = oracle.find_neighbors(c1, cb1, sp, cells, mn, mx, radius, B, True)
    d, c = pref.density_ref(oracle, sp, sb, cells, mn, mx, WINDOW, radius, B, True)
    pdfs = pref.expand_ref(d, st, pk)
    for pn in (True, False):
        assert np.array_equal(res[pn][2][0], st) and np.array_equal(res[pn][2][1], pk) and np.array_equal(res[pn][4][1], c)
        assert_float_close(res[pn][3], pdfs, RTOL, "pdfs")
    args = (sp, sf, sb, pdfs, c1, st, pk, mn, mx, w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
    want = oracle.spatial_conv(*args, fout, True, B, radius, True, True)
    wg = oracle.spatial_conv_grad(*args, og_np, fout, True, B, radius, True, True)
    # the oracle's gradients in the order of `grads`: the feature rows unsorted, then the variables by name
    idx = np.asarray(idx).reshape(-1)      # original index -> sorted position
    assert np.array_equal(sf[idx], fs)
    fg = np.asarray(wg[0])[idx]
    wgrads = [fg, wg[2], wg[4], wg[6], wg[1], wg[3], wg[5]]      # c_biases, c_biases2, c_biases3, c_weights, c_weights2, c_weights3
    for pn in (True, False):
        assert_float_close(_unwrap(res[pn][0]), want, RTOL, "point layer (pointNative %s) against the oracle" % pn)
        for k, (a, b) in enumerate(zip(res[pn][1], wgrads)):
            assert_float_close(_unwrap(a).reshape(-1), np.asarray(b).reshape(-1), RTOL,
                               "gradient %d (0 = features, then the variables by name) against the oracle, pointNative %s" % (k, pn))
    assert_float_close(_unwrap(res[True][0]), _unwrap(res[False][0]), RTOL, "native against op by op")
    for k, (a, b) in enumerate(zip(res[True][1], res[False][1])):
        assert_float_close(_unwrap(a).reshape(-1), _unwrap(b).reshape(-1), RTOL, "gradient %d, native against op by op" % k)


# ------------------------------------------------------------------------------------------------- 7. prefetch
GRAPH = [  # name, lin, lout, fin, fout, combin, radius: six neighbour lists over four grids (tests/test_gpu_native_cap.py)
    ("Conv_f1", 0, 0, 1, 16, True, 0.12), ("Conv_dw", 0, 0, 16, 16, False, 0.12), ("Pool_dw", 0, 1, 16, 16, False, 0.2),
    ("Pool_f1", 0, 1, 1, 8, True, 0.12), ("Conv_l1", 1, 1, 32, 32, False, 0.3), ("Up_dw", 1, 0, 16, 16, False, 0.3),
    ("Conv_3to8", 0, 0, 3, 8, True, 0.16),
]


class _Net:
    """The graph above over batches of different sizes, every layer in point mode: feature rows and output gradients fixed
    per batch."""

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


def _builders():
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    torch.manual_seed(1)
    run = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, pdfMode='point', pointNative=True)
    quiet = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, pdfMode='point', pointNative=True)
    quiet.geoPrefetch_ = False     # the reference: nothing runs ahead
    return run, quiet


def _sync_state(src, dst):
    dst.load_state_dict({k: v.detach().clone() for k, v in src.state_dict().items()})


def test_prefetch_geometry_in_point_mode(mc, oracle, native):
    """prefetch_geometry(..., pdfMode='point') under pointNative: parked as a native point geometry, installed by reset() under
    keyPDF + '|pt', the layer's output the bytes of a builder that prefetched nothing. Without the flag it raises, as before."""
    import torch
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    from mccnn_amd.MCConvModule import InvalidArgumentError
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    g, ph, fs, w, state, (B, radius, fin, fout) = _pool_layer(oracle)
    F = _wrap(fs)
    outs = []
    for pre in (False, True):
        cb = ConvolutionBuilder(KDEWindow=WINDOW, pointNative=True)
        cb.load_state_dict(state)
        if pre:
            cb.prefetch_geometry(ph, 0, radius, outPointLevel=1, pdfMode='point')
            cb.prefetch_geometry(ph, 0, radius, pdfMode='point')                      # same grid and window: shares the pair
            assert len(cb.prefetchedGeo_) == 2 and cb.prefetched_ is None
            cb.reset()
            kG, kN, kP = cb.__compute_dic_keys__(ph, ph, 0, 1, radius, WINDOW, True, True)
            kP0 = cb.__compute_dic_keys__(ph, ph, 0, 0, radius, WINDOW, True, True)[2]
            assert sorted(cb.cacheGeo_) == sorted([kP + "|pt", kP0 + "|pt"]) and list(cb.cachePointPDFs_) == [kG + "|" + str(WINDOW)]
            parked = cb.cacheGeo_[kP + "|pt"]
            assert parked.point and cb.cacheGeo_[kP0 + "|pt"].point_density()[0] is parked.point_density()[0]
        out = cb.create_convolution("c", ph, 0, F, fin, radius, outPointLevel=1, multiFeatureConv=True, outNumFeatures=fout,
                                    pdfMode='point')
        out0 = cb.create_convolution("c", ph, 0, F, fin, radius, multiFeatureConv=True, outNumFeatures=fout, pdfMode='point')
        if pre:
            assert cb.cacheGeo_[kP + "|pt"] is parked and len(cb.cacheGeo_) == 2
        outs.append((out.detach().clone(), out0.detach().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for cb in (ConvolutionBuilder(KDEWindow=WINDOW), ConvolutionBuilder(KDEWindow=WINDOW, pdfMode='point')):
        with pytest.raises(InvalidArgumentError, match="prefetch_geometry"):
            cb.prefetch_geometry(ph, 0, radius, outPointLevel=1, pdfMode='point')
    torch.cuda.synchronize()


def test_learned_prefetch_in_point_mode(mc, native):
    """The seven-layer graph (six lists over four grids), uncapped and in point mode, over two batch sizes and six steps: from
    the second step on every geometry was started a step earlier, the forward outputs are those of a builder with nothing
    running ahead, bit for bit."""
    import torch
    from mccnn_amd.MCConvBuilder import _GEO_PREFETCH_MIN
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    assert len(set((l[1], l[2], l[6]) for l in GRAPH)) >= _GEO_PREFETCH_MIN
    net = _Net(((2500, 5), (1800, 6)))
    run, quiet = _builders()
    for ci in (1, 0):           # (both shapes seen: no list outgrows a capacity guessed from the other batch and is built again inline)
        net.step(run, ci)
    _sync_state(run, quiet)
    order = [0, 1, 1, 0, 1, 0]
    nxt = None
    for s, ci in enumerate(order):
        want = net.step(quiet, ci)
        assert all(geo.core.side < 0 for geo in quiet.cacheGeo_.values())
        torch.cuda.synchronize()
        state = {}

        def start_next():
            if s + 1 < len(order):
                state["ph"] = net.hierarchy(order[s + 1])
                state["n"] = run.prefetch_step(state["ph"])
        got = net.step(run, ci, ph=nxt, then=start_next)
        sides = [geo.core.side for geo in run.cacheGeo_.values()]
        assert len(run.cacheGeo_) == 6 and all(key.endswith("|pt") and geo.point for key, geo in run.cacheGeo_.items())
        assert len(run.cachePointPDFs_) == 4                         # one density per grid
        if s >= 1:
            assert all(sd >= 0 for sd in sides), (s, sides)          # every geometry of the step was started a step ago
        if s + 1 < len(order) and s >= 1:
            assert state["n"] == 6
        nxt = state.get("ph")
        for a, b in zip(got[0], want[0]):
            assert torch.equal(a, b), s
        for a, b in zip(got[1], want[1]):   # (feature gradients of one-feature layers are summed with float atomics)
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    # the learned prefetch WITHOUT prefetch_step: the step's first layer starts every geometry of the plan
    for s, ci in enumerate((0, 1, 0)):
        want = net.step(quiet, ci)
        got = net.step(run, ci)
        assert len(run.cacheGeo_) == 6 and all(geo.core.side >= 0 for geo in run.cacheGeo_.values())
        for a, b in zip(got[0], want[0]):
            assert torch.equal(a, b), s
    torch.cuda.synchronize()


def test_soak_point_pipelined_loop(mc, native):
    """The loop of tools/soak_network.py in short: batches of four sizes in random order, every layer in point mode, the next
    batch's geometries started by prefetch_step under the current step -- and no host synchronisation inside the loop.
    Outputs are compared on the GPU with references computed with nothing running ahead."""
    import torch
    assert native._EXT is not None, "the torch extension (lib/_mccnn_torch.so) did not load"
    net = _Net(((2500, 5), (1200, 6), (3200, 7), (700, 8)))
    run, quiet = _builders()
    net.step(run, 0)
    _sync_state(run, quiet)
    steps = 40
    order = np.random.default_rng(7).integers(0, len(net.clouds), steps)
    refs = [net.step(quiet, int(order[s])) for s in range(steps)]
    torch.cuda.synchronize()
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    worst = torch.zeros((), dtype=torch.float32, device="cuda")
    nxt = None
    for s in range(steps):
        state = {}

        def start_next():
            if s + 1 < steps:
                state["ph"] = net.hierarchy(int(order[s + 1]))
                run.prefetch_step(state["ph"])
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
    geo, _ = _check(mc, oracle, native, "mixed")
    key, g, r = _case(oracle, "mixed")
    _k, _g, orr = _case(oracle, "mixed", None, True)
    h = _inputs(mc, g, key)
    own = (h["P"], h["Bi"])
    sharer = _build(native, g, h, grid_from=geo, centres=own)
    assert sharer.point_density()[0] is geo.point_density()[0] and sharer.point_density()[1] is geo.point_density()[1]
    _against_a(_arrays(sharer), orr, "sharer")
    _equal(_arrays(sharer), _op_chain(mc, g, h, key, centres=own), "sharer")


def test_ctypes_binding():
    """One point geometry and one shared pair through the ctypes binding of the C-ABI (mccnn_geometry_build_point)."""
    env = dict(os.environ, MCCNN_TORCH_EXT="0")
    code = ("import sys, pytest; from mccnn_amd import native; assert native._EXT is None; "
            "sys.exit(pytest.main([%r, '-m', 'gpu', '-x', '-q', '-k', 'test_ctypes_binding_inner']))"
            % os.path.join(ROOT, "tests", "test_gpu_native_point.py"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
