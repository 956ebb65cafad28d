"""The budget entries of the native step executor without a GPU: the header and the binding table, the size query, the
builder's budgetNative argument and its cache keys, a CPU-tensor builder that still runs op by op, and the argument errors
of native.build_geometry, which are raised before any device call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mccnn_geometry_bytes_budget", "mccnn_geometry_build_budget", "mccnn_geometry_build_batch_budget", "mccnn_geometry_cap")


def test_header_and_binding_table_have_the_budget_entries():
    import ctypes as C
    from mccnn_amd import build, _lib
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef\s+struct\s+mccnn_neighbor_budget\s*\{\s*int\s+max_edges;\s*\}\s*mccnn_neighbor_budget;", code)
    # the layout of the cap record is the one it had
    assert re.search(r"typedef\s+struct\s+mccnn_neighbor_cap\s*\{\s*int\s+max_neighbors;\s*int\s+sampled;\s*unsigned\s+seed;\s*\}\s*mccnn_neighbor_cap;", code)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    S = _lib.SIGNATURES
    assert len(S["mccnn_geometry_bytes_budget"][1]) == len(S["mccnn_geometry_bytes_capped"][1]) + 1
    assert len(S["mccnn_geometry_build_budget"][1]) == len(S["mccnn_geometry_build_point"][1]) + 1
    assert len(S["mccnn_geometry_build_batch_budget"][1]) == len(S["mccnn_geometry_build_batch_point"][1]) + 1
    assert S["mccnn_geometry_cap"] == (C.c_void_p, [C.c_void_p])
    # the old entries keep their declarations
    assert "size_t mccnn_geometry_bytes_capped(int n, int m, int batch_size, int num_cells, int e_capacity, int with_grid, int max_neighbors);" in code
    build.build()
    lib = C.CDLL(build.LIB)
    for name in NEW:
        assert hasattr(lib, name), name     # exported by the library


def test_abi_version():
    from mccnn_amd import build, _lib
    build.build()
    assert _lib.load().mccnn_abi_version() >= 17


def test_geometry_bytes_budget():
    from mccnn_amd import build, _lib
    build.build()
    lib = _lib.load()
    tile = 2048                      # centres per tile of the clamped prefix sum: one status word each, and the ticket
    hist = 2048 + 1024 + 1024        # buckets of the three selection levels: a row count (4 bytes) and a sum (8 bytes) each
    for n, m, B, nc, e, grid in ((1000, 1020, 2, 4, 16320, 1), (3000, 3000, 1, 10, 50000, 0), (20000, 17000, 2, 8, 272000, 1),
                                 (5, 1, 1, 1, 1, 1)):
        for K in (0, 16):
            capped = lib.mccnn_geometry_bytes_capped(n, m, B, nc, e, grid, K)
            assert capped > 0 and lib.mccnn_geometry_bytes_budget(n, m, B, nc, e, grid, K, 0) == capped
            base = lib.mccnn_geometry_bytes_capped(n, m, B, nc, e, grid, max(K, 1))   # (a budgeted search keeps the row lengths too)
            region = 8 * ((m + tile - 1) // tile + 1) + 12 * hist
            for budget in (1, 5000, 2 ** 31 - 1):
                got = lib.mccnn_geometry_bytes_budget(n, m, B, nc, e, grid, K, budget)
                assert base + region <= got <= base + region + 1024, (n, m, K, budget, got - base, region)
    # monotone in m
    sizes = [lib.mccnn_geometry_bytes_budget(5000, m, 2, 8, 60000, 1, 0, 30000) for m in (1, 100, 2048, 2049, 4096, 4097, 50000, 2 ** 21)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert lib.mccnn_geometry_bytes_budget(10, 10, 1, 4, 10, 1, 0, -1) == 0
    assert lib.mccnn_geometry_bytes_budget(10, 10, 1, 4, 10, 1, -1, 5) == 0


def test_budget_native_argument():
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    from mccnn_amd.MCConvModule import InvalidArgumentError
    assert ConvolutionBuilder().budgetNative_ is False                                # the default: budgeted layers run op by op
    assert ConvolutionBuilder(maxEdges=1000).budgetNative_ is False
    assert ConvolutionBuilder(maxEdges=1000, capNative=True).budgetNative_ is False   # (capNative_ does not decide for a budget)
    cb = ConvolutionBuilder(maxEdges=1000, budgetNative=True)
    assert cb.budgetNative_ is True and cb.capNative_ is False
    assert ConvolutionBuilder(budgetNative=True).budgetNative_ is True                 # (without a budget: nothing to send anywhere)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(InvalidArgumentError):
            ConvolutionBuilder(maxEdges=1000, budgetNative=bad)
    # which layers may take the native executor
    for bn, cn in ((False, False), (True, False), (False, True), (True, True)):
        cb = ConvolutionBuilder(budgetNative=bn, capNative=cn)
        assert cb.__native_thinning__(0, 0) is True
        assert cb.__native_thinning__(16, 0) is cn
        assert cb.__native_thinning__(0, 500) is bn and cb.__native_thinning__(16, 500) is bn   # the budget flag decides


class _Hier:
    def __init__(self, name):
        self.hierarchyName_ = name


def test_cache_keys_do_not_depend_on_budget_native():
    import zlib
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    ph = _Hier("PH")
    for cap, seed, budget in ((0, None, 0), (0, None, 500), (16, None, 500), (0, 7, 500), (16, 7, 500)):
        keys = [ConvolutionBuilder(maxNeighbors=cap, sampleSeed=seed, maxEdges=budget, budgetNative=bn).__compute_dic_keys__(
            ph, ph, 0, 1, 0.25, 0.2, True, True, cap, seed, budget) for bn in (False, True)]
        assert keys[0] == keys[1]
    kG, kN, kP = keys[1]
    assert kG == "PH|0|0.25|True" and kN == "PH|0|0.25|True|PH|1|16|e500|s7" and kP == "PH|0|0.25|True|PH|1|0.2|True|16|e500|s7"
    # the search of a native geometry gets the op-by-op path's arguments, without the request for the cap tensor
    want_seed = (7 + zlib.crc32(b"PH|0|0.25|True|PH|1|16|e500")) & 0xFFFFFFFF
    assert ConvolutionBuilder.__search_args__(16, 7, kN, 500) == {"maxNeighbors": 16, "maxEdges": 500, "returnCap": True, "sampleSeed": want_seed}
    assert ConvolutionBuilder.__native_search_args__(16, 7, kN, 500) == {"maxNeighbors": 16, "maxEdges": 500, "sampleSeed": want_seed}
    assert ConvolutionBuilder.__native_search_args__(0, None, "x", 500) == {"maxEdges": 500}
    assert ConvolutionBuilder.__native_search_args__(16, None, "x") == {"maxNeighbors": 16}
    assert ConvolutionBuilder.__native_search_args__(0, None, "x") == {}


def test_cpu_tensor_builder_with_budget_native_runs_op_by_op(oracle):
    """Host tensors behind `ops=`: budgetNative changes nothing -- the budgeted search goes through the checker's find_neighbors."""
    import torch
    from tests import neighbor_cap_ref as cref
    from tests import neighbor_budget_ref as bref
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder, PointHierarchy

    class Ops:
        """The oracle behind torch tensors, with the budget applied by tests/neighbor_budget_ref.py."""
        calls = []

        def __getattr__(self, name):
            fn = getattr(oracle, name)

            def call(*a, **kw):
                budget, want_cap = kw.pop("maxEdges", 0), kw.pop("returnCap", False)
                Ops.calls.append((name, budget))
                out = fn(*[x.detach().numpy() if isinstance(x, torch.Tensor) else x for x in a], **kw)
                if name == "find_neighbors" and budget > 0:
                    K = bref.budget_cap(cref.row_lengths(out[0], len(out[1])), budget)
                    out = cref.cap_list(out[0], out[1], K)
                    if want_cap:
                        out = tuple(out) + (np.asarray([K], np.int32),)
                wrap = lambda o: torch.from_numpy(np.ascontiguousarray(o)) if isinstance(o, np.ndarray) else o
                return tuple(wrap(o) for o in out) if isinstance(out, tuple) else wrap(out)
            return call

    g = cref.geom_mixed()
    P, Bi = torch.from_numpy(g["pts"]), torch.from_numpy(g["bids"])
    F = torch.from_numpy((2 * np.random.default_rng(1).random((len(g["pts"]), 3)) - 1).astype(np.float32))
    outs = []
    for bn in (False, True):
        torch.manual_seed(4)
        Ops.calls = []
        ops = Ops()
        ph = PointHierarchy(P, F, Bi, [0.2], "PHb", g["B"], True, ops=ops)
        cb = ConvolutionBuilder(KDEWindow=0.2, maxEdges=3000, budgetNative=bn, ops=ops)
        cb.opTrace_ = []
        outs.append(cb.create_convolution("c", ph, 0, F, 3, g["radius"], outPointLevel=1, multiFeatureConv=True, outNumFeatures=8))
        kN = cb.__compute_dic_keys__(ph, ph, 0, 1, g["radius"], 0.2, True, True, 0, None, 3000)[1]
        assert kN.endswith("|e3000")
        assert not cb.cacheGeo_ and ("find_neighbors", kN) in cb.opTrace_ and isinstance(cb.cacheNeighs_[kN], tuple)
        assert ("find_neighbors", 3000) in Ops.calls
        assert isinstance(cb.chosenCaps_[kN], torch.Tensor) and int(cb.chosenCaps_[kN][0]) >= 1
        assert len(cb.cacheNeighs_[kN][1]) <= 3000
        cb.reset()
        assert kN in cb.chosenCaps_          # (a tensor of the op path outlives reset(), as before)
    assert torch.equal(outs[0], outs[1])


def test_build_geometry_argument_errors_come_before_any_device_call():
    """Host tensors: every check below fires before the first library call, which would fail on them in another way."""
    import torch
    from mccnn_amd import native
    P = torch.zeros((8, 3))
    Bi = torch.zeros((8, 1), dtype=torch.int32)
    mn, mx = torch.zeros((1, 3)), torch.ones((1, 3))
    args = (P, Bi, P, Bi, mn, mx, 1, 4, 0.25, True, 0.2, True)
    for kw, word in ((dict(maxEdges=-1), "maxEdges"), (dict(maxEdges=2 ** 31), "maxEdges"), (dict(maxEdges=1.5), "maxEdges"),
                     (dict(maxEdges=True), "maxEdges"), (dict(sampleSeed=3), "sampleSeed"),
                     (dict(maxEdges=100, sampleSeed=2 ** 32), "sampleSeed"), (dict(maxEdges=100, sampleSeed=-1), "sampleSeed"),
                     (dict(maxEdges=100, pointPDF=True), "pointPDF"), (dict(maxNeighbors=-2, maxEdges=100), "maxNeighbors")):
        with pytest.raises(ValueError, match=word):
            native.build_geometry(*args, **kw)
