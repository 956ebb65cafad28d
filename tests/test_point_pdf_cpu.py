"""pdfMode='point' without a GPU: the NumPy reference of tests/point_pdf_ref.py against the oracle's own compute_pdf on
clouds that lie inside every one of their balls (there the two definitions coincide), the builder's caches, keys, trace
and errors through the oracle-backed op surface, and the C-ABI surface of the two entry points."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import point_pdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WINDOW = 0.25


# ------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("radius,scaleInv", [(0.1, False), (2.0, True)])
def test_reference_equals_the_oracles_compute_pdf_inside_the_ball(oracle, radius, scaleInv):
    """Every row is the whole cloud, so the centre's row and the neighbour's own ball are the same set: density[j] / len_i
    is the oracle's per-edge value. Bar 1e-5 relative per value: the oracle rounds to f32 per statement (measured 4.1e-7)."""
    pts, bids, B, sizes = ref.small_clouds()
    mn, mx, sP, sB, cells, _ = ref.sorted_grid(oracle, pts, bids, B, radius, scaleInv)
    start, packed = ref.point_rows(oracle, sP, sB, cells, mn, mx, radius, B, scaleInv)
    density, counts = ref.density_ref(oracle, sP, sB, cells, mn, mx, WINDOW, radius, B, scaleInv)
    b = np.asarray(sB).reshape(-1)
    want = np.asarray(sizes)[b]
    if scaleInv:
        want = np.where(want == 1, 0, want)          # the one-point cloud: zero extent, R = 0, an empty ball
        assert float(density[b == 1, 0][0]) == 0.0
    assert np.array_equal(counts.reshape(-1), want)
    assert np.array_equal(ref.row_lengths(start, len(packed)), want)
    self_term = (0.39894228 / WINDOW) ** 3
    assert np.all(density[counts > 0] >= self_term * (1 - 1e-12))
    got = ref.expand_ref(density, start, packed)
    exp = oracle.compute_pdf(sP, sB, mn, mx, start, packed, WINDOW, radius, B, scaleInv)
    assert got.shape == exp.shape == (int(want.sum()), 1) and got.dtype == np.float32
    rel = float((np.abs(got.astype(np.float64) - exp) / np.abs(exp)).max())
    print("reference vs oracle compute_pdf (radius %s, scaleInv %s): max rel %.2e" % (radius, scaleInv, rel))
    assert rel <= 1e-5, rel


def test_expand_reference_is_one_f32_divide():
    density = np.asarray([[3.0], [0.1], [7.5]], np.float64)
    start = np.asarray([[0], [3], [3]], np.int32)                     # rows of 3, 0 and 2 edges
    packed = np.asarray([[0, 0], [1, 0], [2, 0], [1, 2], [2, 2]], np.int32)
    got = ref.expand_ref(density, start, packed)
    exp = [np.float32(3.0) / np.float32(3), np.float32(0.1) / np.float32(3), np.float32(7.5) / np.float32(3),
           np.float32(0.1) / np.float32(2), np.float32(7.5) / np.float32(2)]
    assert got.dtype == np.float32 and np.array_equal(got.reshape(-1), np.asarray(exp, np.float32))
    assert ref.expand_ref(density, start[:0], packed[:0]).shape == (0, 1)


# ------------------------------------------------------------------------------------------------- 2. the builder
def _inputs(B=2, n=96, seed=5):
    rng = np.random.default_rng(seed)
    pts = torch.from_numpy(rng.random((B * n, 3), dtype=np.float32))
    bids = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), n).reshape(-1, 1))
    feats = torch.from_numpy(rng.random((B * n, 8), dtype=np.float32))
    return pts, bids, feats, B


def test_builder_shares_the_density_per_grid_and_window(oracle):
    import mccnn_amd.MCConvBuilder as MB
    pts, bids, feats, B = _inputs()
    ops = ref.PointPdfOracleOps(oracle)
    ph = MB.PointHierarchy(pts, feats, bids, [0.2], "PH", B, ops=ops)
    cb = MB.ConvolutionBuilder(KDEWindow=WINDOW, ops=ops, pdfMode='point')
    cb.opTrace_ = []
    a = cb.create_convolution("A", ph, 0, feats, 8, 0.3)                              # same level
    cb.create_convolution("B", ph, 0, a, 8, 0.3, outPointLevel=1)                     # pooling: same grid, another list
    cb.create_convolution("C", ph, 0, a, 8, 0.3)                                      # everything cached
    cb.create_convolution("D", ph, 0, a, 8, 0.3, KDEWindow=0.5)                       # another window: another density
    cb.create_convolution("E", ph, 0, a, 8, 0.3, usePDF=False)                        # no PDF: the mode has no effect
    keyGrid = "PH|0|0.3|True"
    tr = [r for r in cb.opTrace_ if r[0] in ("compute_pdf_points", "expand_pdf", "compute_pdf", "find_neighbors")]
    assert tr == [("find_neighbors", keyGrid + "|PH|0"), ("compute_pdf_points", keyGrid + "|0.25"),
                  ("expand_pdf", keyGrid + "|PH|0|0.25|True|pt"),
                  ("find_neighbors", keyGrid + "|PH|1"), ("expand_pdf", keyGrid + "|PH|1|0.25|True|pt"),
                  ("compute_pdf_points", keyGrid + "|0.5"), ("expand_pdf", keyGrid + "|PH|0|0.5|True|pt")]
    assert list(cb.cachePointPDFs_) == [keyGrid + "|0.25", keyGrid + "|0.5"]
    assert list(cb.cachePDFs_) == [keyGrid + "|PH|0|0.25|True|pt", keyGrid + "|PH|1|0.25|True|pt",
                                   keyGrid + "|PH|0|0.5|True|pt", keyGrid + "|PH|0|0.25|False"]
    # what was filed is the reference's expansion of the reference's density over the oracle's lists
    g = cb.cacheGrids_[keyGrid]
    dens, cnt = ref.density_ref(oracle, g[0].numpy(), g[1].numpy(), g[2].numpy(), ph.aabbMin_.numpy(), ph.aabbMax_.numpy(),
                                WINDOW, 0.3, B, True)
    assert np.array_equal(cb.cachePointPDFs_[keyGrid + "|0.25"][1].numpy(), cnt)
    for lvl in (0, 1):
        st, pk = cb.cacheNeighs_[keyGrid + "|PH|%d" % lvl]
        assert np.array_equal(cb.cachePDFs_[keyGrid + "|PH|%d|0.25|True|pt" % lvl].numpy(),
                              ref.expand_ref(dens.astype(np.float32), st.numpy(), pk.numpy()))
    # the same-level list of the points themselves: the row lengths are the counts
    st, pk = cb.cacheNeighs_[keyGrid + "|PH|0"]
    assert np.array_equal(np.sort(ref.row_lengths(st.numpy(), len(pk))), np.sort(cnt.reshape(-1)))
    cb.reset()
    assert not cb.cachePointPDFs_ and not cb.cachePDFs_
    # a layer may choose its mode: 'edge' inside a 'point' builder runs compute_pdf under the reference's key
    cb.opTrace_ = []
    cb.create_convolution("A", ph, 0, feats, 8, 0.3, pdfMode='edge')
    assert ("compute_pdf", keyGrid + "|PH|0|0.25|True") in cb.opTrace_ and not cb.cachePointPDFs_
    assert list(cb.cachePDFs_) == [keyGrid + "|PH|0|0.25|True"]


def _mcclass_s_trace(MB, cb, ops):
    B, k = 4, 16
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.random((B * 64, 3), dtype=np.float32))
    bids = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), 64).reshape(-1, 1))
    feats = torch.ones((B * 64, 1), dtype=torch.float32)
    ph = MB.PointHierarchy(pts, feats, bids, [0.1, 0.4, math.sqrt(3.0) + 0.1], "MCClassS_PH", B, ops=ops)
    cb.opTrace_ = []
    f1 = cb.create_convolution(convName="Conv_1", inPointHierarchy=ph, inPointLevel=0, outPointLevel=1, inFeatures=feats,
                               inNumFeatures=1, outNumFeatures=k, convRadius=0.2, multiFeatureConv=True)
    f1 = torch.cat([f1, f1], 1)
    f2 = cb.create_convolution(convName="Conv_2", inPointHierarchy=ph, inPointLevel=1, outPointLevel=2, inFeatures=f1,
                               inNumFeatures=k * 2, convRadius=0.8)
    f2 = torch.cat([f2, f2], 1)
    cb.create_convolution(convName="Conv_3", inPointHierarchy=ph, inPointLevel=2, outPointLevel=3, inFeatures=f2,
                          inNumFeatures=k * 4, convRadius=math.sqrt(3.0) + 0.1)


def test_edge_mode_keeps_keys_and_trace(oracle):
    """pdfMode='edge', spelled out or by default: the reference's trace (tests/golden/builder_trace.json) and cache keys."""
    import mccnn_amd.MCConvBuilder as MB
    ops = ref.PointPdfOracleOps(oracle)
    gold = json.load(open(os.path.join(GOLD, "builder_trace.json")))
    gold_ops = [c[0] for c in gold["calls"] if c[0] in ("sort_points_step1", "sort_points_step2", "sort_features", "find_neighbors",
                                                        "compute_pdf", "spatial_conv")]
    res = []
    for kw in ({}, {"pdfMode": "edge"}):
        cb = MB.ConvolutionBuilder(KDEWindow=0.2, ops=ops, **kw)
        assert cb.pdfMode_ == 'edge'
        _mcclass_s_trace(MB, cb, ops)
        res.append((list(cb.opTrace_), list(cb.cacheGrids_), list(cb.cacheNeighs_), list(cb.cachePDFs_), dict(cb.cachePointPDFs_)))
    assert res[0] == res[1]
    trace, grids, neighs, pdfs, pointPdfs = res[0]
    assert [r[0] for r in trace] == gold_ops[-len(trace):] and len(trace) == 15
    assert grids == ["MCClassS_PH|0|0.2|True", "MCClassS_PH|1|0.8|True", "MCClassS_PH|2|%s|True" % (math.sqrt(3.0) + 0.1)]
    assert neighs == [g + "|MCClassS_PH|%d" % (i + 1) for i, g in enumerate(grids)]
    assert pdfs == [n + "|0.2|True" for n in neighs] and pointPdfs == {}


def test_point_mode_errors(oracle):
    import mccnn_amd.MCConvBuilder as MB
    from mccnn_amd.MCConvModule import InvalidArgumentError
    pts, bids, feats, B = _inputs()
    ops = ref.PointPdfOracleOps(oracle)
    ph = MB.PointHierarchy(pts, feats, bids, [], "PH", B, ops=ops)
    for bad in ('row', 'POINT', None, 1, True):
        with pytest.raises(InvalidArgumentError, match="pdfMode"):
            MB.ConvolutionBuilder(ops=ops, pdfMode=bad)
    cb = MB.ConvolutionBuilder(KDEWindow=WINDOW, ops=ops)
    with pytest.raises(InvalidArgumentError, match="pdfMode"):
        cb.create_convolution("A", ph, 0, feats, 8, 0.3, pdfMode='row')
    with pytest.raises(InvalidArgumentError, match="uncapped"):
        cb.create_convolution("A", ph, 0, feats, 8, 0.3, pdfMode='point', maxNeighbors=16)
    with pytest.raises(InvalidArgumentError, match="uncapped"):
        MB.ConvolutionBuilder(ops=ops, pdfMode='point', maxNeighbors=16).create_convolution("A", ph, 0, feats, 8, 0.3)
    with pytest.raises(InvalidArgumentError, match="prefetch_geometry"):
        cb.prefetch_geometry(ph, 0, 0.3, pdfMode='point')
    with pytest.raises(InvalidArgumentError, match="prefetch_geometry"):
        MB.ConvolutionBuilder(ops=ops, pdfMode='point').prefetch_geometry(ph, 0, 0.3)
    gpts = pts.clone().requires_grad_(True)
    phg = MB.PointHierarchy(gpts, feats, bids, [], "PHG", B, ops=ops)
    with pytest.raises(InvalidArgumentError, match="gradient"):
        cb.create_convolution("A", phg, 0, feats, 8, 0.3, pdfMode='point')
    assert not cb.cacheGrids_ and not cb.cachePDFs_ and not cb.cachePointPDFs_      # nothing ran before the errors
    # without a PDF the mode has no effect: a cap, a prefetch and points with a gradient are all allowed
    cb.prefetch_geometry(ph, 0, 0.3, pdfMode='point', usePDF=False)               # (host tensors: a no-op)
    out = cb.create_convolution("A", ph, 0, feats, 8, 0.3, pdfMode='point', usePDF=False)
    assert out.shape == (feats.shape[0], 8) and not cb.cachePointPDFs_


# ------------------------------------------------------------------------------------------------- 3. the C-ABI
def test_entry_points_are_declared_bound_and_documented():
    from mccnn_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mccnn_compute_pdf_points", "mccnn_expand_pdf"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and name in integ
    assert len(_lib.SIGNATURES["mccnn_compute_pdf_points"][1]) == 14 and len(_lib.SIGNATURES["mccnn_expand_pdf"][1]) == 7
    lib = _lib.load() if os.path.exists(build.LIB) and not build.needs_build() else None
    if lib is None:
        build.build()
        lib = _lib.load()
    # argument errors and empty inputs are decided on the host, before any launch
    one = lambda **kw: lib.mccnn_compute_pdf_points(None, None, kw.get("n", 0), None, None, None, kw.get("B", 1), kw.get("nc", 1),
                                                    kw.get("window", 0.25), kw.get("radius", 0.1), 0, None, None, None)
    assert one() == 0                                   # n == 0: nothing to do
    for kw in (dict(n=-1), dict(B=0), dict(nc=0), dict(radius=0.0), dict(radius=-1.0), dict(window=0.0), dict(n=5)):
        assert one(**kw) == -1, kw                      # (n = 5 with null pointers)
    assert lib.mccnn_expand_pdf(None, None, 0, None, 0, None, None) == 0
    assert lib.mccnn_expand_pdf(None, None, 4, None, 0, None, None) == 0
    for m, e in ((-1, 0), (0, -1), (0, 3), (4, 3)):
        assert lib.mccnn_expand_pdf(None, None, m, None, e, None, None) == -1, (m, e)
