"""The capped entries of the native step executor without a GPU: the header and the binding table, the size query, the
builder's capNative argument and its cache keys, and a CPU-tensor builder that still runs op by op."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mccnn_geometry_bytes_capped", "mccnn_geometry_build_capped", "mccnn_geometry_build_batch_capped")


def test_header_and_binding_table_have_the_capped_entries():
    from mccnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef\s+struct\s+mccnn_neighbor_cap\s*\{\s*int\s+max_neighbors;\s*int\s+sampled;\s*unsigned\s+seed;\s*\}\s*mccnn_neighbor_cap;", code)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    # argument counts: the uncapped entry plus the cap
    assert len(_lib.SIGNATURES["mccnn_geometry_bytes_capped"][1]) == len(_lib.SIGNATURES["mccnn_geometry_bytes"][1]) + 1
    assert len(_lib.SIGNATURES["mccnn_geometry_build_capped"][1]) == len(_lib.SIGNATURES["mccnn_geometry_build"][1]) + 1
    assert len(_lib.SIGNATURES["mccnn_geometry_build_batch_capped"][1]) == len(_lib.SIGNATURES["mccnn_geometry_build_batch"][1]) + 1
    # the old entries keep their declarations
    assert "size_t mccnn_geometry_bytes(int n, int m, int batch_size, int num_cells, int e_capacity, int with_grid);" in code
    assert "int mccnn_geometry_build_batch(const mccnn_geometry_request* requests, int count, mccnn_stream_t stream);" in code


def test_geometry_bytes_capped():
    from mccnn_amd import build, _lib
    build.build()
    lib = _lib.load()
    for n, m, B, nc, e, grid in ((1000, 1020, 2, 4, 16320, 1), (3000, 3000, 1, 10, 50000, 0), (20000, 17000, 2, 8, 272000, 1),
                                 (5, 1, 1, 1, 1, 1)):
        plain = lib.mccnn_geometry_bytes(n, m, B, nc, e, grid)
        assert plain > 0 and lib.mccnn_geometry_bytes_capped(n, m, B, nc, e, grid, 0) == plain
        for K in (1, 16, 300):
            capped = lib.mccnn_geometry_bytes_capped(n, m, B, nc, e, grid, K)
            # (the capped search keeps the true row lengths: m more words, whichever stage of the chain sets the workspace)
            assert plain + 4 * m <= capped <= plain + 4 * m + 512
    assert lib.mccnn_geometry_bytes_capped(10, 10, 1, 4, 10, 1, -1) == 0


def test_cap_native_argument():
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    from mccnn_amd.MCConvModule import InvalidArgumentError
    assert ConvolutionBuilder().capNative_ is False                                   # the default: capped layers run op by op
    assert ConvolutionBuilder(maxNeighbors=16).capNative_ is False
    assert ConvolutionBuilder(maxNeighbors=16, capNative=True).capNative_ is True
    assert ConvolutionBuilder(capNative=True).capNative_ is True                       # (without a cap: nothing to send anywhere)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(InvalidArgumentError):
            ConvolutionBuilder(maxNeighbors=16, capNative=bad)


class _Hier:
    def __init__(self, name):
        self.hierarchyName_ = name


def test_cache_keys_do_not_depend_on_cap_native():
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder
    ph = _Hier("PH")
    for cap, seed in ((0, None), (16, None), (16, 7)):
        keys = [ConvolutionBuilder(maxNeighbors=cap, sampleSeed=seed, capNative=cn).__compute_dic_keys__(
            ph, ph, 0, 1, 0.25, 0.2, True, True, cap, seed) for cn in (False, True)]
        assert keys[0] == keys[1]
    kG, kN, kP = keys[1]
    assert kG == "PH|0|0.25|True" and kN == "PH|0|0.25|True|PH|1|16|s7" and kP == "PH|0|0.25|True|PH|1|0.2|True|16|s7"
    # the seed the search of a geometry gets is the op-by-op path's
    import zlib
    args = ConvolutionBuilder.__search_args__(16, 7, kN)
    assert args == {"maxNeighbors": 16, "sampleSeed": (7 + zlib.crc32(b"PH|0|0.25|True|PH|1|16")) & 0xFFFFFFFF}
    assert ConvolutionBuilder.__search_args__(16, None, kN[:-3]) == {"maxNeighbors": 16}
    assert ConvolutionBuilder.__search_args__(0, None, "x") == {}


def test_cpu_tensor_builder_with_cap_native_runs_op_by_op(oracle):
    """Host tensors behind `ops=`: capNative changes nothing -- the capped search goes through the checker's find_neighbors."""
    import torch
    from tests import neighbor_cap_ref as ref
    from mccnn_amd.MCConvBuilder import ConvolutionBuilder, PointHierarchy

    class Ops:
        """The oracle behind torch tensors, with the cap applied by tests/neighbor_cap_ref.py."""
        calls = []

        def __getattr__(self, name):
            fn = getattr(oracle, name)

            def call(*a, **kw):
                cap = kw.pop("maxNeighbors", 0)
                Ops.calls.append((name, cap))
                out = fn(*[x.detach().numpy() if isinstance(x, torch.Tensor) else x for x in a], **kw)
                if name == "find_neighbors":
                    out = ref.cap_list(out[0], out[1], cap)
                wrap = lambda o: torch.from_numpy(np.ascontiguousarray(o)) if isinstance(o, np.ndarray) else o
                return tuple(wrap(o) for o in out) if isinstance(out, tuple) else wrap(out)
            return call

    g = ref.geom_mixed()
    P, Bi = torch.from_numpy(g["pts"]), torch.from_numpy(g["bids"])
    F = torch.from_numpy((2 * np.random.default_rng(1).random((len(g["pts"]), 3)) - 1).astype(np.float32))
    outs = []
    for cn in (False, True):
        torch.manual_seed(4)
        Ops.calls = []
        ops = Ops()
        ph = PointHierarchy(P, F, Bi, [0.2], "PHc", g["B"], True, ops=ops)
        cb = ConvolutionBuilder(KDEWindow=0.2, maxNeighbors=16, capNative=cn, ops=ops)
        cb.opTrace_ = []
        outs.append(cb.create_convolution("c", ph, 0, F, 3, g["radius"], outPointLevel=1, multiFeatureConv=True, outNumFeatures=8))
        kN = cb.__compute_dic_keys__(ph, ph, 0, 1, g["radius"], 0.2, True, True, 16)[1]
        assert not cb.cacheGeo_ and ("find_neighbors", kN) in cb.opTrace_ and isinstance(cb.cacheNeighs_[kN], tuple)
        assert ("find_neighbors", 16) in Ops.calls
    assert torch.equal(outs[0], outs[1])
