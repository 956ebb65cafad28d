"""Position gradients of pdfMode='point' without a GPU: the C-ABI surface of the two backward entries (declared, exported,
bound, argument errors before any launch), the builder's pointGrad argument, and the kernels' closed form (NumPy float64)
against torch float64 autograd of the definition over the oracle's rows (tests/point_pdf_grad_ref.py) -- which also shows
that the oracle's rows are symmetric on the test inputs, the fact the closed form rests on."""
import os
import re

import numpy as np
import pytest

from tests import neighbor_cap_ref as geo
from tests import point_pdf_grad_ref as gref
from tests import point_pdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = 0.25


def _lib_loaded():
    from mccnn_amd import _lib, build
    if not os.path.exists(build.LIB) or build.needs_build():
        build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------- 1. the C-ABI
def test_entry_points_are_declared_bound_and_exported():
    from mccnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    for decl in (
            "size_t mccnn_compute_pdf_points_bwd_workspace_bytes(int n, int batch_size);",
            "int mccnn_compute_pdf_points_bwd(const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs, "
            "const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window, float radius, "
            "int scale_inv, const float* density_grad, float* dpts, float* dradius, void* ws, size_t ws_bytes, "
            "mccnn_stream_t stream);",
            "int mccnn_expand_pdf_bwd(float* density_grad, const float* pdfs_grad, const int* start_idx, int m, const int* packed, "
            "int e, const int* start_t, const int* perm_t, int n, mccnn_stream_t stream);"):
        assert decl in flat, decl
    sig = _lib.SIGNATURES
    assert len(sig["mccnn_compute_pdf_points_bwd"][1]) == 17 and len(sig["mccnn_expand_pdf_bwd"][1]) == 10
    assert len(sig["mccnn_compute_pdf_points_bwd_workspace_bytes"][1]) == 2
    # the forward's inputs lead the backward's, type for type
    assert sig["mccnn_compute_pdf_points_bwd"][1][:11] == sig["mccnn_compute_pdf_points"][1][:11]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib_loaded()
    for name in ("mccnn_compute_pdf_points_bwd", "mccnn_compute_pdf_points_bwd_workspace_bytes", "mccnn_expand_pdf_bwd"):
        assert getattr(lib, name) is not None and name in integ
    assert lib.mccnn_abi_version() >= 14
    assert lib.mccnn_compute_pdf_points_bwd_workspace_bytes(100000, 4) >= 100000 * 4
    assert lib.mccnn_compute_pdf_points_bwd_workspace_bytes(0, 1) > 0


def test_argument_errors_come_before_any_launch():
    lib = _lib_loaded()
    nan = float("nan")

    def sweep(n=0, B=1, nc=1, window=0.25, radius=0.1, si=0, dR=None, ws=None, wsb=0):
        return lib.mccnn_compute_pdf_points_bwd(None, None, n, None, None, None, B, nc, window, radius, si, None, None, dR, ws,
                                                wsb, None)
    before = lib.mccnn_debug_launch_count()
    assert sweep() == 0 and sweep(si=1) == 0                        # n == 0: nothing to do
    for kw in (dict(n=-1), dict(B=0), dict(B=-2), dict(nc=0), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan),
               dict(window=0.0), dict(window=-0.5), dict(window=nan), dict(n=5), dict(n=5, si=1)):
        assert sweep(**kw) == -1, kw                                # (n = 5: null pointers)
    assert sweep(dR=1024, si=0) == -1                               # a radius gradient needs the relative radius
    assert lib.mccnn_expand_pdf_bwd(None, None, None, 0, None, 0, None, None, 0, None) == 0
    assert lib.mccnn_expand_pdf_bwd(None, None, None, 4, None, 0, None, None, 7, None) == 0      # e == 0
    assert lib.mccnn_expand_pdf_bwd(None, None, None, 4, None, 9, None, None, 0, None) == 0      # n == 0
    for m, e, n in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 3, 5), (4, 3, 5)):
        assert lib.mccnn_expand_pdf_bwd(None, None, None, m, None, e, None, None, n, None) == -1, (m, e, n)
    assert lib.mccnn_debug_launch_count() == before


# ------------------------------------------------------------------------------------------------- 2. the builder
def test_point_grad_argument():
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    from mccnn_amd.MCConvModule import InvalidArgumentError
    assert ConvolutionBuilder().pointGrad_ is False and ConvolutionBuilder(pdfMode='point').pointGrad_ is False
    cb = ConvolutionBuilder(pdfMode='point', pointGrad=True)
    assert cb.pointGrad_ is True and cb.pointNative_ is False
    assert ConvolutionBuilder(pdfMode='point', pointGrad=True, pointNative=True).pointGrad_ is True
    cb.pointGrad_ = False      # reassigned between steps, like pointNative_
    cb.reset()
    assert cb.pointGrad_ is False
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(InvalidArgumentError, match="pointGrad"):
            ConvolutionBuilder(pdfMode='point', pointGrad=bad)


def test_ops_surface_keeps_the_gradient_error(oracle):
    """Behind `ops=` (not the HIP surface) nothing differentiates the density: the error stays whatever the flag."""
    import torch
    import mccnn_amd.MCConvBuilder as MB
    from mccnn_amd.MCConvModule import InvalidArgumentError
    rng = np.random.default_rng(5)
    B = 2
    pts = torch.from_numpy(rng.random((120, 3), dtype=np.float32)).requires_grad_(True)
    bids = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), 60).reshape(-1, 1))
    feats = torch.ones((120, 8), dtype=torch.float32)
    ops = ref.PointPdfOracleOps(oracle)
    ph = MB.PointHierarchy(pts, feats, bids, [], "PHG", B, ops=ops)
    for flag in (False, True):
        cb = MB.ConvolutionBuilder(KDEWindow=WINDOW, ops=ops, pdfMode='point', pointGrad=flag)
        with pytest.raises(InvalidArgumentError, match="gradient"):
            cb.create_convolution("A", ph, 0, feats, 8, 0.3)
        assert not cb.cacheGrids_ and not cb.cachePDFs_ and not cb.cachePointPDFs_
        with pytest.raises(InvalidArgumentError, match="uncapped"):
            cb.create_convolution("A", ph, 0, feats, 8, 0.3, maxNeighbors=16)


# ------------------------------------------------------------------------------------------------- 3. the closed form
def _inputs(name):
    if name == "mixed":
        g = geo.geom_mixed()
        return g["pts"], g["bids"], g["B"]
    pts, bids, B, _ = ref.small_clouds()
    return pts, bids, B


@pytest.mark.parametrize("name,radius,scaleInv", [("small", 0.1, False), ("small", 2.0, True), ("mixed", 0.25, True),
                                                  ("mixed", 0.25, False)])
def test_closed_form_equals_autograd_of_the_definition(oracle, name, radius, scaleInv):
    pts, bids, B = _inputs(name)
    mn, mx, sP, sB, cells, idx = ref.sorted_grid(oracle, pts, bids, B, radius, scaleInv)
    start, packed = ref.point_rows(oracle, sP, sB, cells, mn, mx, radius, B, scaleInv)
    packed = np.asarray(packed).reshape(-1, 2)
    # the rows are symmetric: (l, j) is an edge exactly when (j, l) is
    fwd = set(map(tuple, packed.tolist()))
    assert fwd == {(j, l) for l, j in fwd} and len(fwd) == len(packed)
    n = len(sP)
    gd = np.random.default_rng(17).random(n)
    dp, box = gref.sweep_grads(sP, sB, mn, mx, packed, WINDOW, radius, scaleInv, gd)
    cdp, cdR = gref.closed_form(sP, sB, mn, mx, packed, WINDOW, radius, scaleInv, gd)
    assert np.isfinite(dp).all() and np.abs(dp).max() > 0
    assert np.allclose(cdp, dp, rtol=1e-9, atol=1e-9 * np.abs(dp).max())
    if scaleInv:
        cbox = gref.box_from_dR(mn, mx, cdR, radius)
        assert np.abs(box).max() > 0 and np.allclose(cbox, box, rtol=1e-9, atol=1e-9 * np.abs(box).max())
    if name == "small" and scaleInv:      # the one-point cloud: R = 0, an empty row, no gradient at all
        one = np.asarray(sB).reshape(-1) == 1
        assert one.sum() == 1 and not dp[one].any() and not cdp[one].any() and cdR[1] == 0.0
        assert not box[[1, B + 1]].any()


def test_expand_reference_matches_expand_ref(oracle):
    """The float64 restatement of the expansion is tests/point_pdf_ref.expand_ref up to its f32 rounding."""
    import torch
    g = geo.geom_many_centres()
    mn, mx, sP, sB, cells, idx = ref.sorted_grid(oracle, g["pts"], g["bids"], g["B"], g["radius"], g["scaleInv"])
    start, packed = oracle.find_neighbors(g["centres"], g["cbids"], sP, cells, mn, mx, g["radius"], g["B"], g["scaleInv"])
    d = np.random.default_rng(3).random(len(sP)).astype(np.float32)
    got = gref.expand(torch.as_tensor(d.astype(np.float64)), start, packed).numpy()
    want = ref.expand_ref(d, start, packed).reshape(-1).astype(np.float64)
    assert np.allclose(got, want, rtol=2e-7, atol=0)
