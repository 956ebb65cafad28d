"""find_neighbors(maxNeighbors=K) without a GPU: the NumPy thinning rule the GPU tests compare against, the builder's cache
keys and op trace with and without a cap, the C-ABI surface of the capped passes, and the regimes the seeded test geometries
of tests/neighbor_cap_ref.py reach (row lengths and window sizes, from the oracle's lists)."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import neighbor_cap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------- 1. the rule
def _brute_force(start, packed, K):
    st = np.asarray(start).reshape(-1)
    rows, new_start, run = [], [], 0
    for i in range(len(st)):
        a = int(st[i])
        b = int(st[i + 1]) if i + 1 < len(st) else len(packed)
        k = b - a
        new_start.append(run)
        keep = list(range(k)) if k <= K else [(t * k) // K for t in range(K)]
        rows.extend(packed[a + r] for r in keep)
        run += len(keep)
    return np.asarray(new_start, np.int32).reshape(-1, 1), np.asarray(rows, np.int32).reshape(-1, 2)


@pytest.mark.parametrize("K", [1, 2, 7, 16, 100])
def test_thinning_rule(K):
    prime = next(p for p in range(K + 1, 4 * K + 20) if all(p % d for d in range(2, int(p ** 0.5) + 1)))
    special = [0, 1, K, K + 1, 2 * K, prime, 0, 3 * K + 1, 1]
    rng = np.random.default_rng(K)
    lengths = np.asarray(special + list(rng.integers(0, 4 * K + 3, 40)), np.int64)
    rng.shuffle(lengths)
    for k in lengths:
        ranks = ref.cap_ranks(k, K)
        assert len(ranks) == min(k, K)
        assert np.all(np.diff(ranks) > 0)                 # strictly increasing: a subsequence, no hit twice
        if k > 0:
            assert ranks[0] == 0 and ranks[-1] < k
        # the per-hit (compaction) form agrees with the forward rule for every rank
        slots = [ref.cap_slot(r, k, K) for r in range(int(k))]
        kept = [r for r in range(int(k)) if slots[r] >= 0]
        assert kept == list(ranks)
        assert [slots[r] for r in kept] == list(range(len(ranks)))
    start = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int32).reshape(-1, 1)
    e = int(lengths.sum())
    packed = np.stack([rng.integers(0, 1 << 20, e), np.repeat(np.arange(len(lengths)), lengths)], 1).astype(np.int32)
    st, pk = ref.cap_list(start, packed, K)
    bst, bpk = _brute_force(start, packed, K)
    assert st.dtype == np.int32 and pk.dtype == np.int32
    assert np.array_equal(st, bst) and np.array_equal(pk, bpk)
    assert np.array_equal(np.diff(np.append(st[:, 0], len(pk))), np.minimum(lengths, K))
    st0, pk0 = ref.cap_list(start, packed, 0)             # 0 = no cap
    assert np.array_equal(st0, start) and np.array_equal(pk0, packed)


def test_thinning_rule_in_64_bit():
    """k * K beyond 2^32: the slot arithmetic needs 64-bit integers (the kernel switches on k * (K + 1))."""
    k, K = 3000017, 2000003
    ranks = ref.cap_ranks(k, K)
    assert len(ranks) == K and ranks[0] == 0 and np.all(np.diff(ranks) > 0) and ranks[-1] < k
    for r in (0, 1, 2, int(ranks[12345]), int(ranks[12345]) + 1, int(ranks[-1]), k - 1):
        t = ref.cap_slot(r, k, K)
        assert (t >= 0) == bool(np.any(ranks == r)) and (t < 0 or ranks[t] == r)


# ------------------------------------------------------------------------------------------------- 2. the builder
@pytest.fixture()
def shimmed_builder(oracle, monkeypatch):
    """The op names of the builder's module replaced by oracle-backed CPU shims, as tests/test_builder_cpu.py does."""
    import mccnn_amd.MCConvBuilder as MB
    calls = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else x

    def shim(name):
        fn = getattr(oracle, name)

        def f(*args, **kwargs):
            calls.append((name, dict(kwargs)))
            cap = kwargs.pop("maxNeighbors", 0)
            assert not kwargs
            out = fn(*[n(a) for a in args])
            if name == "find_neighbors" and cap:
                out = ref.cap_list(out[0], out[1], cap)
            return tuple(t(o) for o in out) if isinstance(out, tuple) else t(out)
        return f

    for nm in ("compute_aabb", "sort_points_step1", "sort_points_step2", "sort_features", "sort_features_back",
               "compute_pdf", "poisson_sampling", "get_sampled_features", "spatial_conv", "transform_indexs",
               "find_neighbors"):
        monkeypatch.setattr(MB, nm, shim(nm))
    monkeypatch.setattr(MB, "get_block_size", lambda: 8)
    return MB, calls


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
    return ph, f3


def test_builder_without_a_cap_is_the_reference_builder(shimmed_builder):
    """maxNeighbors=0, given explicitly to the constructor and to every call: the golden op sequence of the reference's
    builder, no keyword reaches the ops, and the cache keys are the reference's strings."""
    MB, calls = shimmed_builder
    gold = json.load(open(os.path.join(GOLD, "builder_trace.json")))
    gold_ops = [c[0] for c in gold["calls"] if c[0] not in ("get_variable", "add_to_collection")]
    cb = MB.ConvolutionBuilder(KDEWindow=0.2, maxNeighbors=0)
    cb.opTrace_ = []
    ph, f3 = _mcclass_s(MB, cb, maxNeighbors=0)
    assert [c[0] for c in calls] == gold_ops
    assert all(not kw for _, kw in calls)
    cb_default = MB.ConvolutionBuilder(KDEWindow=0.2)
    cb_default.opTrace_ = []
    _mcclass_s(MB, cb_default)
    assert cb.opTrace_ == cb_default.opTrace_
    kG = "MCClassS_PH|0|0.2|True"
    assert cb.opTrace_[:4] == [("sort_points_step1", kG), ("sort_points_step2", kG), ("find_neighbors", kG + "|MCClassS_PH|1"),
                               ("compute_pdf", kG + "|MCClassS_PH|1|0.2|True")]
    assert cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True) == (kG, kG + "|MCClassS_PH|1",
                                                                           kG + "|MCClassS_PH|1|0.2|True")
    assert cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 0) == cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2,
                                                                                                    True, True)


def test_builder_keys_and_ops_with_a_cap(shimmed_builder):
    MB, calls = shimmed_builder
    cb = MB.ConvolutionBuilder(KDEWindow=0.2, maxNeighbors=7)
    cb.opTrace_ = []
    ph, f3 = _mcclass_s(MB, cb)
    k0 = cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 0)
    k7 = cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 7)
    k8 = cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 8)
    assert k0[0] == k7[0] == k8[0]                                     # the grid does not depend on the cap
    assert len({k0[1], k7[1], k8[1]}) == 3 and len({k0[2], k7[2], k8[2]}) == 3
    assert k7[1] == k0[1] + "|7" and k7[2] == k0[2] + "|7"
    # the builder's default reaches every search, the caches are filed under the capped keys, rows are capped
    searches = [kw for name, kw in calls if name == "find_neighbors" and kw]
    assert searches == [{"maxNeighbors": 7}] * 3
    assert k7[1] in cb.cacheNeighs_ and k7[2] in cb.cachePDFs_ and k0[1] not in cb.cacheNeighs_
    st, pk = cb.cacheNeighs_[k7[1]]
    assert ref.row_lengths(st.numpy(), len(pk)).max() <= 7
    assert [r[0] for r in cb.opTrace_ if r[0] != "spatial_conv"] == ["sort_points_step1", "sort_points_step2",
                                                                    "find_neighbors", "compute_pdf"] * 3
    # a per-call cap overrides the default, 0 switches it off for that call: other cache entries over the same grid
    n = len(calls)
    feats = torch.ones((ph.points_[0].shape[0], 1), dtype=torch.float32)
    cb.create_convolution("Conv_1", ph, 0, feats, 1, 0.2, outPointLevel=1, multiFeatureConv=True, outNumFeatures=16,
                          maxNeighbors=0)
    assert [c for c in calls[n:] if c[0] == "find_neighbors"] == [("find_neighbors", {})]
    assert k0[1] in cb.cacheNeighs_ and [c[0] for c in calls[n:]].count("sort_points_step1") == 0
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError):
            MB.ConvolutionBuilder(maxNeighbors=bad)
    with pytest.raises(ValueError):
        cb.create_convolution("Conv_1", ph, 0, feats, 1, 0.2, outPointLevel=1, multiFeatureConv=True, outNumFeatures=16,
                              maxNeighbors=-2)


# ------------------------------------------------------------------------------------------------- 3. header and binding
CAPPED = ("mccnn_find_neighbors_count_capped", "mccnn_find_neighbors_fill_capped")


def test_header_declares_the_capped_passes():
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in CAPPED:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name
        assert re.search(r"int\s+max_neighbors\s*$", m.group(1).strip()), name    # the trailing argument
    # the uncapped entries keep their argument lists
    assert re.search(r"int\s+mccnn_find_neighbors_fill\s*\([^;]*mccnn_stream_t\s+stream\s*\)\s*;", code)
    assert re.search(r"int\s+mccnn_find_neighbors_count\s*\([^;]*mccnn_stream_t\s+stream\s*\)\s*;", code)


def test_binding_and_library_have_the_capped_passes():
    import ctypes
    from mccnn_amd import _lib, build
    lib_path = build.build()
    for name, base in zip(CAPPED, ("mccnn_find_neighbors_count", "mccnn_find_neighbors_fill")):
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == (ctypes.c_int, _lib.SIGNATURES[base][1] + [ctypes.c_int])
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    assert set(CAPPED) <= exported
    lib = _lib.load()
    for m in (0, 1, 1000, 100000):   # host-only: the capped workspace also holds one int per centre
        assert lib.mccnn_find_neighbors_capped_workspace_bytes(m, m) >= lib.mccnn_find_neighbors_workspace_bytes(m, m) + 4 * m


def test_op_rejects_a_negative_cap():
    import mccnn_amd.MCConvModule as M
    z = torch.zeros((4, 3))
    for bad in (-1, 2.0, True):
        with pytest.raises(M.InvalidArgumentError, match="maxNeighbors"):
            M.find_neighbors(z, z, z, z, z, z, 0.1, 1, True, maxNeighbors=bad)


# ------------------------------------------------------------------------------------------------- 4. the GPU tests' geometries
#: name -> what the oracle's list of the geometry must show, measured here (M, E, max k, empty rows, max window):
#:   mixed         1020   28868    59   20   315   (70 windows of 257..315 points, the rest up to 256)
#:   mid_windows   1500   99172   240    0   498
#:   big_windows   3000 1032324  1015    0  1056
#:   many_centres  5000   97982    40    0   191
MEASURED = dict(mixed=(1020, 28868, 59, 20, 315), mid_windows=(1500, 99172, 240, 0, 498),
                big_windows=(3000, 1032324, 1015, 0, 1056), many_centres=(5000, 97982, 40, 0, 191))


def test_mixed_geometry_under_the_absolute_radius(oracle):
    """scaleInv off: one box of extent 1.25 for both clouds, 4 cells per axis -- windows of all three regimes."""
    g = dict(ref.geom_mixed(), scaleInv=False)
    r = ref.uncapped(oracle, g)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    w = ref.window_sizes(g, r)
    assert (len(k), int(k.sum()), int(k.max()), int((k == 0).sum()), int(w.max())) == (1020, 29008, 60, 20, 586)
    assert ((w > 512) & (k > 16)).sum() > 0 and ((w > 256) & (w <= 512) & (k > 16)).sum() > 0 and ((w <= 256) & (k > 16)).sum() > 0


@pytest.mark.parametrize("name", sorted(ref.GEOMETRIES))
def test_geometries_reach_their_regimes(oracle, name):
    g = ref.GEOMETRIES[name]()
    r = ref.uncapped(oracle, g)
    k = ref.row_lengths(r["startIndexs"], len(r["packedNeighs"]))
    w = ref.window_sizes(g, r)
    print(name, "M", len(k), "E", int(k.sum()), "max k", int(k.max()), "empty rows", int((k == 0).sum()), "max window", int(w.max()))
    assert (len(k), int(k.sum()), int(k.max()), int((k == 0).sum()), int(w.max())) == MEASURED[name]
    assert np.all(w >= k)
    if name == "mixed":          # K = 16: rows under the cap, over it, and empty; a list of at most 4096 centres
        assert len(k) <= 4096 and (k > 16).mean() >= 0.1 and (k <= 16).mean() >= 0.1 and (k == 0).sum() >= 20
        assert (w <= 256).sum() > 0
    elif name == "mid_windows":  # K = 32, 100: windows of 257..512 points whose rows exceed both caps
        assert w.max() <= 512 and ((w > 256) & (k > 100)).sum() > 0
    elif name == "big_windows":  # K = 64, 1: windows the fill pass searches again, rows of more than 600 hits
        assert ((w > 512) & (k > 600)).sum() > 0
    else:                        # K = 24: count, scan, fill
        assert len(k) > 4096 and (k > 24).mean() >= 0.1 and (k <= 24).mean() >= 0.1
