"""The point entries of the native step executor without a GPU: the header, the binding table and the struct layout, the
builder's pointNative argument and its cache keys, a CPU-tensor builder that still runs op by op, and the bad-argument
returns of the new entries (decided on the host, before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mccnn_geometry_build_point", "mccnn_geometry_build_batch_point")


def _header_code():
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_and_binding_table_have_the_point_entries():
    from mccnn_amd import _lib, native
    code = _header_code()
    assert re.search(r"typedef\s+struct\s+mccnn_point_pdf\s*\{\s*float\s*\*\s*density;\s*int\s*\*\s*counts;\s*int\s+ready;\s*\}\s*mccnn_point_pdf;", code)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    # argument counts: the capped entry plus the point record
    assert len(_lib.SIGNATURES["mccnn_geometry_build_point"][1]) == len(_lib.SIGNATURES["mccnn_geometry_build_capped"][1]) + 1
    assert len(_lib.SIGNATURES["mccnn_geometry_build_batch_point"][1]) == len(_lib.SIGNATURES["mccnn_geometry_build_batch_capped"][1]) + 1
    assert _lib.SIGNATURES["mccnn_geometry_build_point"][1][:-1] == _lib.SIGNATURES["mccnn_geometry_build_capped"][1]
    # the declaration of the single entry: the capped one's parameters, then the record
    flat = re.sub(r"\s+", " ", code)
    capped = re.search(r"int mccnn_geometry_build_capped\((.*?)\);", flat).group(1)
    point = re.search(r"int mccnn_geometry_build_point\((.*?)\);", flat).group(1)
    assert point == capped + ", const mccnn_point_pdf* point"
    assert ("int mccnn_geometry_build_batch_point(const mccnn_geometry_request* requests, const mccnn_neighbor_cap* caps, "
            "const mccnn_point_pdf* points, int count, mccnn_stream_t stream);") in flat
    # the binding's struct: two pointers and an int, as the C compiler lays them out
    P = native._PointPdf
    assert [f[0] for f in P._fields_] == ["density", "counts", "ready"]
    assert (P.density.offset, P.counts.offset, P.ready.offset) == (0, C.sizeof(C.c_void_p), 2 * C.sizeof(C.c_void_p))
    assert C.sizeof(P) == 3 * C.sizeof(C.c_void_p)       # (the int is padded to the pointers' alignment)


def test_old_declarations_are_verbatim():
    flat = re.sub(r"\s+", " ", _header_code())
    for decl in (
            "size_t mccnn_geometry_bytes(int n, int m, int batch_size, int num_cells, int e_capacity, int with_grid);",
            "int mccnn_geometry_build(mccnn_geometry_t* g, const float* pts, const int* batch_ids, int n, const float* centres, "
            "const int* centre_batch_ids, int m, const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, "
            "float radius, int scale_inv, float window, int use_pdf, int e_capacity, const mccnn_geometry_t* grid_from, "
            "void* buffer, size_t buffer_bytes, int* total_host, mccnn_stream_t stream);",
            "int mccnn_geometry_build_batch(const mccnn_geometry_request* requests, int count, mccnn_stream_t stream);",
            "typedef struct mccnn_neighbor_cap { int max_neighbors; int sampled; unsigned seed; } mccnn_neighbor_cap;",
            "size_t mccnn_geometry_bytes_capped(int n, int m, int batch_size, int num_cells, int e_capacity, int with_grid, "
            "int max_neighbors);",
            "int mccnn_geometry_build_capped(mccnn_geometry_t* g, const float* pts, const int* batch_ids, int n, const float* centres, "
            "const int* centre_batch_ids, int m, const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, "
            "float radius, int scale_inv, float window, int use_pdf, int e_capacity, const mccnn_geometry_t* grid_from, "
            "void* buffer, size_t buffer_bytes, int* total_host, mccnn_stream_t stream, const mccnn_neighbor_cap* cap);",
            "int mccnn_geometry_build_batch_capped(const mccnn_geometry_request* requests, const mccnn_neighbor_cap* caps, int count, "
            "mccnn_stream_t stream);",
            "int mccnn_compute_pdf_points(const float* sorted_pts, const int* sorted_batch_ids, int n, const int* cell_indexs, "
            "const float* aabb_min, const float* aabb_max, int batch_size, int num_cells, float window, float radius, "
            "int scale_inv, float* density, int* counts, mccnn_stream_t stream);",
            "int mccnn_expand_pdf(const float* density, const int* start_idx, int m, const int* packed, int e, float* pdfs, "
            "mccnn_stream_t stream);"):
        assert decl in flat, decl


def test_point_native_argument():
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    from mccnn_amd.MCConvModule import InvalidArgumentError
    assert ConvolutionBuilder().pointNative_ is False                                  # the default: point layers run op by op
    assert ConvolutionBuilder(pdfMode='point').pointNative_ is False
    assert ConvolutionBuilder(pdfMode='point', pointNative=True).pointNative_ is True
    assert ConvolutionBuilder(pointNative=True).pointNative_ is True                    # (in edge mode: nothing to send anywhere)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(InvalidArgumentError, match="pointNative"):
            ConvolutionBuilder(pdfMode='point', pointNative=bad)


class _Hier:
    def __init__(self, name):
        self.hierarchyName_ = name


def test_cache_keys_do_not_depend_on_point_native():
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    ph = _Hier("PH")
    keys = [ConvolutionBuilder(pdfMode='point', pointNative=pn).__compute_dic_keys__(ph, ph, 0, 1, 0.25, 0.2, True, True)
            for pn in (False, True)]
    assert keys[0] == keys[1] == ("PH|0|0.25|True", "PH|0|0.25|True|PH|1", "PH|0|0.25|True|PH|1|0.2|True")


def test_cpu_tensor_builder_with_point_native_runs_op_by_op(oracle):
    """Host tensors behind `ops=`: pointNative changes nothing -- the density and its expansion go through the checker's
    compute_pdf_points / expand_pdf, with the trace and the cache keys of tests/test_point_pdf_cpu.py."""
    import torch
    import mccnn_amd.MCConvBuilder as MB
    from mccnn_amd.MCConvModule import InvalidArgumentError
    from tests import point_pdf_ref as ref
    rng = np.random.default_rng(5)
    B, n = 2, 96
    pts = torch.from_numpy(rng.random((B * n, 3), dtype=np.float32))
    bids = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), n).reshape(-1, 1))
    feats = torch.from_numpy(rng.random((B * n, 8), dtype=np.float32))
    ops = ref.PointPdfOracleOps(oracle)
    keyGrid = "PH|0|0.3|True"
    res = []
    for pn in (False, True):
        torch.manual_seed(4)
        ph = MB.PointHierarchy(pts, feats, bids, [0.2], "PH", B, ops=ops)
        cb = MB.ConvolutionBuilder(KDEWindow=0.25, ops=ops, pdfMode='point', pointNative=pn)
        cb.opTrace_ = []
        a = cb.create_convolution("A", ph, 0, feats, 8, 0.3)                              # same level
        b = cb.create_convolution("B", ph, 0, a, 8, 0.3, outPointLevel=1)                 # pooling: same grid, another list
        cb.create_convolution("D", ph, 0, a, 8, 0.3, KDEWindow=0.5)                       # another window: another density
        tr = [r for r in cb.opTrace_ if r[0] in ("compute_pdf_points", "expand_pdf", "compute_pdf", "find_neighbors")]
        assert tr == [("find_neighbors", keyGrid + "|PH|0"), ("compute_pdf_points", keyGrid + "|0.25"),
                      ("expand_pdf", keyGrid + "|PH|0|0.25|True|pt"),
                      ("find_neighbors", keyGrid + "|PH|1"), ("expand_pdf", keyGrid + "|PH|1|0.25|True|pt"),
                      ("compute_pdf_points", keyGrid + "|0.5"), ("expand_pdf", keyGrid + "|PH|0|0.5|True|pt")]
        assert not cb.cacheGeo_ and isinstance(cb.cacheNeighs_[keyGrid + "|PH|0"], tuple)
        assert list(cb.cachePointPDFs_) == [keyGrid + "|0.25", keyGrid + "|0.5"]
        assert list(cb.cachePDFs_) == [keyGrid + "|PH|0|0.25|True|pt", keyGrid + "|PH|1|0.25|True|pt", keyGrid + "|PH|0|0.5|True|pt"]
        cb.prefetch_geometry(ph, 0, 0.3, pdfMode='point', usePDF=False)                   # (host tensors: a no-op)
        if pn:
            cb.prefetch_geometry(ph, 0, 0.3)                                              # allowed under the flag; host tensors: a no-op
            assert not cb.prefetchedGeo_ and cb.prefetched_ is None
        else:
            with pytest.raises(InvalidArgumentError, match="prefetch_geometry"):
                cb.prefetch_geometry(ph, 0, 0.3)
        # the errors of the mode stay whatever the flag
        with pytest.raises(InvalidArgumentError, match="uncapped"):
            cb.create_convolution("A", ph, 0, feats, 8, 0.3, maxNeighbors=16)
        gpts = pts.clone().requires_grad_(True)
        phg = MB.PointHierarchy(gpts, feats, bids, [], "PHG", B, ops=ops)
        with pytest.raises(InvalidArgumentError, match="gradient"):
            cb.create_convolution("A", phg, 0, feats, 8, 0.3)
        res.append((a, b))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_bad_arguments_of_the_point_entries():
    """Everything below is refused by the argument checks: nothing is launched and no pointer is followed."""
    from mccnn_amd import build, _lib, native
    build.build()
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 13
    BADARG = -1
    g = lib.mccnn_geometry_create()
    try:
        # fake, never dereferenced addresses (256-byte aligned where the library asks for it)
        a = lambda k: C.c_void_p(0x10000 * (k + 1))
        slot = (C.c_int * 1)(0)
        nbytes = lib.mccnn_geometry_bytes(100, 50, 1, 4, 1000, 1)
        assert nbytes > 0

        def single(use_pdf=1, cap=None, point=None, buffer=a(7), centres=a(3)):
            return lib.mccnn_geometry_build_point(g, a(1), a(2), 100, centres, a(4), 50, a(5), a(6), 1, 4, 0.1, 0, 0.25, use_pdf, 1000,
                                                  None, buffer, nbytes, C.cast(slot, C.c_void_p), None,
                                                  C.addressof(cap) if cap is not None else None,
                                                  C.addressof(point) if point is not None else None)
        P, K = native._PointPdf, native._NeighborCap
        assert single(point=P(0x1000, 0x2000, 0), use_pdf=0) == BADARG                    # a density without PDFs
        assert single(point=P(0x1000, 0x2000, 1), cap=K(16, 0, 0)) == BADARG              # a density over a capped list
        assert single(point=P(0x1000, None, 0)) == BADARG                                 # one buffer without the other
        assert single(point=P(None, 0x2000, 1)) == BADARG
        assert single(point=P(0x1000, 0x2000, 0), centres=None) == BADARG                 # (the checks of the other entries hold)
        assert single(point=None, buffer=None) == BADARG
        assert single(point=P(None, None, 0), buffer=None) == BADARG                      # both null: edge mode, its own checks

        class Req(C.Structure):   # mccnn_geometry_request
            _fields_ = [("geometry", C.c_void_p), ("pts", C.c_void_p), ("batch_ids", C.c_void_p), ("n", C.c_int),
                        ("centres", C.c_void_p), ("centre_batch_ids", C.c_void_p), ("m", C.c_int),
                        ("aabb_min", C.c_void_p), ("aabb_max", C.c_void_p), ("batch_size", C.c_int), ("num_cells", C.c_int),
                        ("radius", C.c_float), ("scale_inv", C.c_int), ("window", C.c_float), ("use_pdf", C.c_int),
                        ("e_capacity", C.c_int), ("grid_from", C.c_void_p), ("buffer", C.c_void_p), ("buffer_bytes", C.c_size_t),
                        ("total_host", C.c_void_p)]

        def batch(use_pdf=1, cap=None, point=None, count=1):
            r = (Req * 1)(Req(g, 0x10000, 0x20000, 100, 0x30000, 0x40000, 50, 0x50000, 0x60000, 1, 4, 0.1, 0, 0.25, use_pdf, 1000,
                              None, 0x70000, nbytes, C.cast(slot, C.c_void_p).value))
            caps = (K * 1)(cap) if cap is not None else None
            pts = (P * 1)(point) if point is not None else None
            return lib.mccnn_geometry_build_batch_point(r, caps, pts, count, None)
        assert lib.mccnn_geometry_build_batch_point(None, None, None, 1, None) == BADARG
        assert batch(count=-1) == BADARG
        assert batch(count=0) == 0 and batch(point=P(0x1000, 0x2000, 0), count=0) == 0     # nothing to do
        assert batch(point=P(0x1000, 0x2000, 0), use_pdf=0) == BADARG
        assert batch(point=P(0x1000, 0x2000, 1), cap=K(16, 0, 0)) == BADARG
        assert batch(point=P(0x1000, None, 0)) == BADARG
        assert batch(point=P(None, 0x2000, 0)) == BADARG
    finally:
        lib.mccnn_geometry_destroy(g)
