"""find_neighbors(maxEdges=B) without a GPU: the rule that picks the cap (tests/neighbor_budget_ref.py), the figures the GPU
tests expect (from the oracle's lists), the builder's cache keys and op trace with a budget, the op's argument errors, the
C-ABI surface, and the host build of the selection's scalar half (mccnn_amd/csrc/neigh_budget.h)."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import neighbor_budget_ref as bref
from tests import neighbor_cap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------- 1. the rule
def _vectors():
    rng = np.random.default_rng(7)
    yield np.zeros(0, np.int64)
    yield np.zeros(5, np.int64)
    yield np.asarray([3], np.int64)
    for top in (1, 5, 60, 1100, 70000, 2 ** 31 - 1):
        for m in (1, 2, 17, 300):
            k = rng.integers(0, top + 1, m)
            k[rng.random(m) < 0.2] = 0
            yield k.astype(np.int64)


def test_budget_rule():
    """S(K*) <= B < S(K* + 1) unless K* is saturated (at kmax or at the user's cap) or sits on the floor."""
    rng = np.random.default_rng(8)
    for k in _vectors():
        kmax = max(int(k.max()) if len(k) else 0, 1)
        E = bref.edges_under(k, kmax)
        for Ku in (0, 1, max(kmax // 3, 1), kmax, kmax + 5):
            top = min(kmax, Ku) if Ku else kmax
            budgets = {1, max(len(k), 1), E + 1, max(E, 1), max(E - 1, 1), 2 ** 31 - 1} | {int(b) for b in rng.integers(1, max(E, 2) + 1, 6)}
            for B in sorted(budgets):
                K = bref.budget_cap(k, B, Ku)
                assert 1 <= K <= top
                if bref.edges_under(k, 1) > B:
                    assert K == 1                                             # the floor
                    continue
                assert bref.edges_under(k, K) <= B
                assert K == top or bref.edges_under(k, K + 1) > B             # the largest such cap
                assert bref.edges_under(k, K) <= max(B, int((np.asarray(k) > 0).sum()))


def test_budget_is_monotone():
    for k in _vectors():
        E = bref.edges_under(k, 2 ** 31)
        last = 0
        for B in sorted({1, 2, 3, max(E // 7, 1), max(E // 2, 1), max(E - 1, 1), max(E, 1), E + 1}):
            K = bref.budget_cap(k, B)
            assert K >= last
            last = K
            assert bref.budget_cap(k, B, 4) == min(K, 4)                      # a user cap only clips


# ------------------------------------------------------------------------------------------------- 2. the expected figures
_LISTS = {}


def _oracle_rows(oracle, name):
    if name not in _LISTS:
        g = bref.BUDGET_GEOMETRIES[name]()
        r = ref.uncapped(oracle, g)
        _LISTS[name] = (g, r, ref.row_lengths(r["startIndexs"], len(r["packedNeighs"])))
    return _LISTS[name]


@pytest.mark.parametrize("name", sorted(bref.TABLE))
def test_table_from_the_oracle(oracle, name):
    g, r, k = _oracle_rows(oracle, name)
    m, E, kmax, rows = bref.TABLE[name]
    assert (len(k), int(k.sum()), int(k.max())) == (m, E, kmax)
    if name == "tall_rows":
        assert tuple(int(x) for x in k) == bref.TALL_ROW_LENGTHS
    nonempty = int((k > 0).sum())
    for B, K, EK in rows:
        got = bref.budget_cap(k, B)
        st, pk = ref.cap_list(r["startIndexs"], r["packedNeighs"], got)
        print(name, "B", B, "K*", got, "E(K*)", len(pk))
        assert got == K, (name, B)
        assert EK is None or len(pk) == EK
        assert len(pk) == bref.edges_under(k, got) and len(pk) <= max(B, nonempty)
    if name == "mixed":   # with a user cap at B = 14 434 (the GPU test's cases)
        assert bref.budget_cap(k, 14434, 10) == 10 and bref.budget_cap(k, 14434, 40) == 15
        assert nonempty == 1000


def test_mixed_under_the_absolute_radius(oracle):
    """The GPU test's two budgets on `mixed` with scaleInv off (E 29 008, max k 60: tests/test_neighbor_cap_cpu.py)."""
    g = dict(ref.geom_mixed(), scaleInv=False)
    k = ref.row_lengths(*(lambda r: (r["startIndexs"], len(r["packedNeighs"])))(ref.uncapped(oracle, g)))
    assert int(k.sum()) == 29008
    assert [bref.budget_cap(k, B) for B in (7252, 14504)] == [7, 15]


# ------------------------------------------------------------------------------------------------- 3. the builder
@pytest.fixture()
def shimmed_builder(oracle, monkeypatch):
    """The builder's ops replaced by oracle-backed CPU shims (tests/test_neighbor_cap_cpu.py); find_neighbors takes the cap
    and the budget through NumPy stand-ins (cap_list at budget_cap) and records what it chose."""
    import mccnn_amd.MCConvBuilder as MB
    calls, chosen = [], []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else x

    def shim(name):
        fn = getattr(oracle, name)

        def f(*args, **kwargs):
            calls.append((name, dict(kwargs)))
            cap, budget = kwargs.pop("maxNeighbors", 0), kwargs.pop("maxEdges", 0)
            ret = kwargs.pop("returnCap", False)
            kwargs.pop("sampleSeed", None)   # (the stand-in keeps the canonical ranks)
            assert not kwargs
            out = fn(*[n(a) for a in args])
            if name == "find_neighbors":
                if budget:
                    cap = bref.budget_cap(ref.row_lengths(out[0], len(out[1])), budget, cap)
                    chosen.append(cap)
                if cap:
                    out = ref.cap_list(out[0], out[1], cap)
                if ret:
                    out = tuple(out) + (np.asarray([cap], np.int32),)
            return tuple(t(o) for o in out) if isinstance(out, tuple) else t(out)
        return f

    for nm in ("compute_aabb", "sort_points_step1", "sort_points_step2", "sort_features", "sort_features_back",
               "compute_pdf", "poisson_sampling", "get_sampled_features", "spatial_conv", "transform_indexs",
               "find_neighbors"):
        monkeypatch.setattr(MB, nm, shim(nm))
    monkeypatch.setattr(MB, "get_block_size", lambda: 8)
    return MB, calls, chosen


def _mcclass_s(MB, cb, **conv_kwargs):
    B, k = 4, 16
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.random((B * 64, 3), dtype=np.float32))
    bids = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), 64).reshape(-1, 1))
    feats = torch.ones((B * 64, 1), dtype=torch.float32)
    ph = MB.PointHierarchy(pts, feats, bids, [0.1, 0.4, math.sqrt(3.0) + 0.1], "MCClassS_PH", B)
    f1 = cb.create_convolution(convName="Conv_1", inPointHierarchy=ph, inPointLevel=0, outPointLevel=1, inFeatures=feats,
                               inNumFeatures=1, outNumFeatures=k, convRadius=0.2, multiFeatureConv=True, **conv_kwargs)
    f1 = torch.cat([f1, f1], 1)
    f2 = cb.create_convolution(convName="Conv_2", inPointHierarchy=ph, inPointLevel=1, outPointLevel=2, inFeatures=f1,
                               inNumFeatures=k * 2, convRadius=0.8, **conv_kwargs)
    f2 = torch.cat([f2, f2], 1)
    f3 = cb.create_convolution(convName="Conv_3", inPointHierarchy=ph, inPointLevel=2, outPointLevel=3, inFeatures=f2,
                               inNumFeatures=k * 4, convRadius=math.sqrt(3.0) + 0.1, **conv_kwargs)
    return ph, feats, f3


def test_builder_without_a_budget_is_the_reference_builder(shimmed_builder):
    MB, calls, chosen = shimmed_builder
    gold = json.load(open(os.path.join(GOLD, "builder_trace.json")))
    gold_ops = [c[0] for c in gold["calls"] if c[0] not in ("get_variable", "add_to_collection")]
    cb = MB.ConvolutionBuilder(KDEWindow=0.2, maxEdges=0)
    cb.opTrace_ = []
    ph, feats, f3 = _mcclass_s(MB, cb, maxEdges=0)
    assert [c[0] for c in calls] == gold_ops
    assert all(not kw for _, kw in calls) and not chosen and not cb.chosenCaps_
    cb_default = MB.ConvolutionBuilder(KDEWindow=0.2)
    cb_default.opTrace_ = []
    _mcclass_s(MB, cb_default)
    assert cb.opTrace_ == cb_default.opTrace_
    kG = "MCClassS_PH|0|0.2|True"
    assert cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 0, None, 0) == (kG, kG + "|MCClassS_PH|1",
                                                                                      kG + "|MCClassS_PH|1|0.2|True")


def test_builder_keys_and_ops_with_a_budget(shimmed_builder):
    MB, calls, chosen = shimmed_builder
    cb = MB.ConvolutionBuilder(KDEWindow=0.2, maxEdges=300)
    assert cb.maxEdges_ == 300
    cb.opTrace_ = []
    ph, feats, f3 = _mcclass_s(MB, cb)
    keys = lambda *a: cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, *a)
    k0, kb, kcb, kcbs, kbs = keys(0), keys(0, None, 300), keys(7, None, 300), keys(7, 5, 300), keys(0, 5, 300)
    assert k0[0] == kb[0] == kcb[0] == kcbs[0]                          # the grid is shared
    assert kb[1] == k0[1] + "|e300" and kb[2] == k0[2] + "|e300"
    assert kcb[1] == k0[1] + "|7|e300" and kcbs[1] == k0[1] + "|7|e300|s5" and kcbs[2] == k0[2] + "|7|e300|s5"
    assert kbs[1] == k0[1] + "|e300|s5"
    assert keys(7) == (k0[0], k0[1] + "|7", k0[2] + "|7") and keys(7, 5) == (k0[0], k0[1] + "|7|s5", k0[2] + "|7|s5")
    # the default reaches every search; every list is within its budget (or on the floor) and its cap is kept
    searches = [kw for name, kw in calls if name == "find_neighbors"]
    assert searches == [{"maxEdges": 300, "returnCap": True}] * 3 and len(chosen) == 3
    assert kb[1] in cb.cacheNeighs_ and kb[2] in cb.cachePDFs_ and k0[1] not in cb.cacheNeighs_
    st, pk = cb.cacheNeighs_[kb[1]]
    klen = ref.row_lengths(st.numpy(), len(pk))
    assert len(pk) <= max(300, int((klen > 0).sum())) and int(klen.max()) == chosen[0]
    assert int(cb.chosenCaps_[kb[1]][0]) == chosen[0] and len(cb.chosenCaps_) == 3
    assert [r[0] for r in cb.opTrace_ if r[0] != "spatial_conv"] == ["sort_points_step1", "sort_points_step2",
                                                                    "find_neighbors", "compute_pdf"] * 3
    assert not cb.cacheGeo_                                             # op by op, whatever capNative_ says
    # per call: a budget of the layer's own with a cap and a seed; 0 switches the default off
    n = len(calls)
    conv = lambda **kw: cb.create_convolution("Conv_1", ph, 0, feats, 1, 0.2, outPointLevel=1, multiFeatureConv=True,
                                              outNumFeatures=16, **kw)
    conv(maxEdges=0)
    assert [c for c in calls[n:] if c[0] == "find_neighbors"] == [("find_neighbors", {})] and k0[1] in cb.cacheNeighs_
    n = len(calls)
    conv(maxEdges=500, maxNeighbors=3, sampleSeed=9)
    (name, kw), = [c for c in calls[n:] if c[0] == "find_neighbors"]
    assert kw["maxEdges"] == 500 and kw["maxNeighbors"] == 3 and kw["returnCap"] is True and 0 <= kw["sampleSeed"] < 2 ** 32
    import zlib
    assert kw["sampleSeed"] == (9 + zlib.crc32((k0[1] + "|3|e500").encode())) & 0xffffffff
    assert chosen[-1] <= 3 and (k0[1] + "|3|e500|s9") in cb.cacheNeighs_
    # the attribute may be reassigned between steps
    cb.maxEdges_ = 0
    cb.reset()
    n = len(calls)
    conv()
    assert [c for c in calls[n:] if c[0] == "find_neighbors"] == [("find_neighbors", {})]


def test_builder_budget_errors(shimmed_builder):
    MB, calls, chosen = shimmed_builder
    import mccnn_amd.MCConvModule as M
    for bad in (-1, 1.5, True, "3", 2 ** 31):
        with pytest.raises(M.InvalidArgumentError, match="maxEdges"):
            MB.ConvolutionBuilder(maxEdges=bad)
    cb = MB.ConvolutionBuilder(KDEWindow=0.2)
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.random((64, 3), dtype=np.float32))
    bids = torch.zeros((64, 1), dtype=torch.int32)
    feats = torch.ones((64, 1), dtype=torch.float32)
    ph = MB.PointHierarchy(pts, feats, bids, [0.4], "PHb", 1)
    conv = lambda **kw: cb.create_convolution("c", ph, 0, feats, 1, 0.2, outPointLevel=1, multiFeatureConv=True,
                                              outNumFeatures=8, **kw)
    for bad in (-2, 2.0, False):
        with pytest.raises(M.InvalidArgumentError, match="maxEdges"):
            conv(maxEdges=bad)
        with pytest.raises(M.InvalidArgumentError, match="maxEdges"):
            cb.prefetch_geometry(ph, 0, 0.2, outPointLevel=1, maxEdges=bad)
    with pytest.raises(M.InvalidArgumentError, match="uncapped neighbour list"):
        conv(maxEdges=100, pdfMode='point')
    with pytest.raises(M.InvalidArgumentError, match="sampleSeed needs a cap"):
        conv(sampleSeed=3)
    conv(maxEdges=100, sampleSeed=3)                                    # a seed is allowed with a budget alone
    assert calls[-1][0] == "spatial_conv" and any(kw.get("maxEdges") == 100 and "sampleSeed" in kw for nm, kw in calls)


# ------------------------------------------------------------------------------------------------- 4. the op, header and binding
def test_op_rejects_bad_budgets_without_the_library(monkeypatch):
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib

    def no_library():
        raise AssertionError("the library is loaded before the arguments are checked")
    monkeypatch.setattr(_lib, "load", no_library)
    z = torch.zeros((4, 3))
    for bad in (-1, 2.0, True, 2 ** 31, "5"):
        with pytest.raises(M.InvalidArgumentError, match="maxEdges"):
            M.find_neighbors(z, z, z, z, z, z, 0.1, 1, True, maxEdges=bad)
    with pytest.raises(M.InvalidArgumentError, match="sampleSeed"):
        M.find_neighbors(z, z, z, z, z, z, 0.1, 1, True, sampleSeed=1)
    with pytest.raises(M.InvalidArgumentError, match="maxNeighbors"):
        M.find_neighbors(z, z, z, z, z, z, 0.1, 1, True, maxNeighbors=-1, maxEdges=5)


BUDGET = ("mccnn_find_neighbors_count_budget", "mccnn_find_neighbors_fill_budget")


def test_header_declares_the_budget_passes():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mccnn.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % BUDGET[0], code)
    assert m and re.search(r"int\s+max_neighbors\s*,\s*int\s+max_edges\s*,\s*int\s*\*\s*cap_dev\s*$", m.group(1).strip())
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % BUDGET[1], code)
    assert m and re.search(r"const\s+int\s*\*\s*cap_dev\s*,\s*int\s+sampled\s*,\s*unsigned\s+seed\s*$", m.group(1).strip())
    assert re.search(r"size_t\s+mccnn_find_neighbors_budget_workspace_bytes\s*\(\s*int\s+m\s*,\s*int\s+n\s*\)\s*;", code)


def test_binding_and_library_have_the_budget_passes():
    from mccnn_amd import _lib, build
    lib_path = build.build()
    i, vp, u = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint
    assert _lib.SIGNATURES[BUDGET[0]] == (i, _lib.SIGNATURES["mccnn_find_neighbors_count"][1] + [i, i, vp])
    assert _lib.SIGNATURES[BUDGET[1]] == (i, _lib.SIGNATURES["mccnn_find_neighbors_fill"][1] + [vp, i, u])
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    assert set(BUDGET) | {"mccnn_find_neighbors_budget_workspace_bytes"} <= exported
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 16
    for m in (0, 1, 1000, 100000):   # host-only: the capped workspace and the selection's histograms (4096 buckets of 4 + 8 bytes)
        assert lib.mccnn_find_neighbors_budget_workspace_bytes(m, m) >= lib.mccnn_find_neighbors_capped_workspace_bytes(m, m) + 4096 * 12
    # argument errors are decided on the host, before any launch
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)   # (never dereferenced: the calls below fail first)
    common = [one, one, 4, one, 4, one, one, one, 1, 2, 0.1, 1, null]
    count = lambda K, B, cap: lib.mccnn_find_neighbors_count_budget(*common, one, one, one, 1 << 20, null, K, B, cap)
    assert count(0, 0, one) == -1 and count(0, -5, one) == -1 and count(-1, 10, one) == -1 and count(0, 10, null) == -1
    assert lib.mccnn_find_neighbors_fill_budget(*common, one, 4, one, one, 1 << 20, null, null, 0, 0) == -1
    assert lib.mccnn_find_neighbors_count_budget(*common, one, one, one, 16, null, 0, 10, one) == -4   # workspace too small


# ------------------------------------------------------------------------------------------------- 5. the selection on the host
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_selection_header_on_the_host(tmp_path, flags):
    """mccnn_amd/csrc/neigh_budget.h compiled for the host as a stand-alone program (tools/budget_select_check.cpp): the
    three-level descent agrees with brute force on random row lengths, totals beyond 2^32 and budgets with S(K*) = B."""
    exe = str(tmp_path / "budget_select_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1"] + flags + ["-I", os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "budget_select_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.startswith("ok ")
    m = re.match(r"ok (\d+) \(uncapped totals beyond 2\^32: (\d+), S\(K\*\) = B: (\d+)\)", out.stdout)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) > 0 and int(m.group(3)) > 0
