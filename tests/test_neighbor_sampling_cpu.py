"""find_neighbors(maxNeighbors=K, sampleSeed=s) without a GPU: the NumPy rule the GPU tests compare against
(tests/neighbor_sample_ref.py), the host build of the fill pass's predicate against it, the C-ABI surface of the sampled fill
pass, the op's argument checks, and the builder's keys, seeds and op trace with and without a seed."""
import ctypes
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

from tests import neighbor_cap_ref as cap
from tests import neighbor_sample_ref as ref
from tests.test_neighbor_cap_cpu import _mcclass_s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (1, 16, 64)


def _lengths(K):
    return sorted({k for k in (K + 1, 2 * K - 1, 2 * K, 59, 1015) if k > K})


def _csr(lengths, rng):
    lengths = np.asarray(lengths, np.int64)
    start = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int32).reshape(-1, 1)
    e = int(lengths.sum())
    packed = np.stack([rng.integers(0, 1 << 20, e), np.repeat(np.arange(len(lengths)), lengths)], 1).astype(np.int32)
    return start, packed


# ------------------------------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("K", CAPS)
def test_strata_and_one_hit_per_stratum(K):
    for k in _lengths(K):
        lo = ref.strata(k, K)
        assert len(lo) == K + 1 and lo[0] == 0 and lo[-1] == k and np.all(np.diff(lo) >= 1)     # a partition of [0, k)
        assert np.array_equal(lo[:-1], cap.cap_ranks(k, K))                                    # the canonical cap's strata
        for seed in (0, 1, 12345, 2 ** 32 - 1):
            for i in (0, 1, 1019):
                ranks = ref.sample_ranks(i, k, K, seed)
                assert len(ranks) == K and np.all(np.diff(ranks) > 0)                          # K distinct ascending ranks
                assert np.all(ranks >= lo[:-1]) and np.all(ranks < lo[1:])                     # one per stratum
                slots = [ref.sample_slot(r, i, k, K, seed) for r in range(k)]                  # the per-hit form agrees
                assert [r for r in range(k) if slots[r] >= 0] == list(ranks)
                assert [slots[r] for r in ranks] == list(range(K))
    assert np.array_equal(ref.sample_ranks(3, K, K, 5), np.arange(K))                          # k <= K: untouched


@pytest.mark.parametrize("K", CAPS)
def test_offset_zero_is_the_canonical_cap(K):
    rng = np.random.default_rng(K)
    lengths = _lengths(K) + [0, 1, K] + list(rng.integers(0, 4 * K + 3, 20))
    start, packed = _csr(lengths, rng)
    st0, pk0 = ref.sample_list(start, packed, K, 9, zero=True)
    stc, pkc = cap.cap_list(start, packed, K)
    assert st0.dtype == np.int32 and pk0.dtype == np.int32
    assert np.array_equal(st0, stc) and np.array_equal(pk0, pkc)
    st, pk = ref.sample_list(start, packed, K, 9)
    assert np.array_equal(st, stc) and pk.shape == pkc.shape                                   # startIndexs: no seed in it
    # a subsequence of the uncapped rows, in canonical order: the positions of the kept hits ascend row by row
    pos = {tuple(p): n for n, p in enumerate(packed.tolist())}
    if len(pos) == len(packed):
        idx = np.asarray([pos[tuple(p)] for p in pk.tolist()])
        assert np.all(np.diff(idx) > 0)


def test_rule_in_64_bit():
    """k * K beyond 2^32: the slot arithmetic needs 64-bit integers (the kernel switches on k * (K + 1))."""
    k, K, i, seed = 3000017, 2000003, 5, 7
    ranks = ref.sample_ranks(i, k, K, seed)
    lo = ref.strata(k, K)
    assert len(ranks) == K and np.all(np.diff(ranks) > 0) and np.all(ranks >= lo[:-1]) and np.all(ranks < lo[1:])
    for r in (0, 1, 2, int(ranks[12345]), int(ranks[12345]) + 1, int(lo[12345]), int(ranks[-1]), k - 1):
        t = ref.sample_slot(r, i, k, K, seed)
        assert (t >= 0) == bool(np.any(ranks == r)) and (t < 0 or ranks[t] == r)


def test_hash_vectors():
    """mix is the murmur3 finaliser: its published vectors (0 -> 0; 1 -> 0x514E28B7) and 2^32 wrap-around."""
    assert int(ref.mix(0)) == 0 and int(ref.mix(1)) == 0x514E28B7
    assert int(ref.mix(2 ** 32 + 1)) == int(ref.mix(1))
    x = 0xDEADBEEF
    for sh, mul in ((16, 0x85EBCA6B), (13, 0xC2B2AE35)):
        x ^= x >> sh
        x = (x * mul) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(ref.mix(0xDEADBEEF)) == x


@pytest.fixture(scope="module")
def mixed_list(oracle):
    g = ref.GEOMETRIES["mixed"]()
    r = ref.uncapped(oracle, g)
    return r["startIndexs"], r["packedNeighs"]


def test_every_hit_is_reached_by_some_seed(mixed_list):
    """Seeds 0..255 on `mixed` with K = 16 (strata of at most 4 hits: a miss has probability below 1e-30): every hit of every
    over-full row is kept by at least one seed. The canonical cap alone fails this by construction."""
    start, packed = mixed_list
    K = 16
    st = start.reshape(-1).astype(np.int64)
    k = ref.row_lengths(st, len(packed))
    assert k.max() == 59 and np.diff(ref.strata(59, K)).max() <= 4
    seen = np.zeros(len(packed), bool)
    for seed in range(256):
        for i in np.nonzero(k > K)[0]:
            seen[st[i] + ref.sample_ranks(i, k[i], K, seed)] = True
    over = np.repeat(k > K, k)
    assert seen[over].all(), "%d hits never drawn" % int((~seen[over]).sum())
    canon = np.zeros(len(packed), bool)
    for i in np.nonzero(k > K)[0]:
        canon[st[i] + cap.cap_ranks(k[i], K)] = True
    assert not canon[over].all()


def test_seeds_differ_and_repeat(mixed_list):
    start, packed = mixed_list
    a, b, a2 = (ref.sample_list(start, packed, 16, s) for s in (1, 2, 1))
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1])
    # rows are not drawn alike: the offsets of two rows of the same length differ under one seed
    assert not np.array_equal(ref.offsets(0, 59, 16, 1), ref.offsets(1, 59, 16, 1))


def test_host_build_of_the_kernel_predicate(tmp_path):
    """mccnn_amd/csrc/neigh_sample.h compiled for the host (tools/sample_slot_check.cpp): its own forward-rule check passes,
    and the ranks it keeps on the (k, K) grid above are sample_ranks' for every row it prints."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sample_slot_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "sample_slot_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 disagreements" in out.stdout, out.stdout + out.stderr
    rows = subprocess.check_output([exe, "--dump"], text=True).splitlines()
    seen = set()
    for line in rows:
        head, tail = line.split(":")
        K, k, seed, i = (int(v) for v in head.split())
        assert np.array_equal(np.asarray(tail.split(), np.int64), ref.sample_ranks(i, k, K, seed)), head
        seen.add((K, k))
    assert seen == {(K, k) for K in CAPS for k in _lengths(K)}


# ------------------------------------------------------------------------------------------------- 2. header, library, binding
SAMPLED = "mccnn_find_neighbors_fill_sampled"


def test_header_declares_the_sampled_fill():
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % SAMPLED, code)
    assert m
    assert re.search(r"int\s+max_neighbors\s*,\s*unsigned\s+seed\s*$", m.group(1).strip())
    capped = re.search(r"\bint\s+mccnn_find_neighbors_fill_capped\s*\(([^;]*)\)\s*;", code).group(1)
    norm = lambda a: re.sub(r"\s+", " ", a).strip()
    assert norm(m.group(1)) == norm(capped) + ", unsigned seed"
    assert re.search(r"int\s+mccnn_find_neighbors_fill_capped\s*\([^;]*int\s+max_neighbors\s*\)\s*;", code)


def test_binding_and_library_have_the_sampled_fill():
    from mccnn_amd import _lib, build
    lib_path = build.build()
    base = _lib.SIGNATURES["mccnn_find_neighbors_fill_capped"]
    assert _lib.SIGNATURES[SAMPLED] == (ctypes.c_int, base[1] + [ctypes.c_uint])
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    assert SAMPLED in set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    lib = _lib.load()
    assert hasattr(lib, SAMPLED)
    # host-only argument check: a cap of 0 (or less) is no sampled search
    args = [None, None, 4, None, 4, None, None, None, 1, 2, 0.1, 1, None, None, 0, None, None, 0, None]
    for K in (0, -1):
        assert getattr(lib, SAMPLED)(*args, K, 7) == lib.mccnn_find_neighbors_fill_capped(*args, -1) != 0   # MCCNN_E_BADARG
    # the torch extension binds the native executor's calls, which take no cap: it keeps clear of the capped and sampled passes
    src = open(os.path.join(ROOT, "mccnn_amd", "csrc", "torch_ext.cpp")).read()
    assert "fill_capped" not in src and SAMPLED not in src


def test_op_rejects_bad_seeds():
    import mccnn_amd.MCConvModule as M
    z = torch.zeros((4, 3))
    for bad in (-1, 2 ** 32, True, 1.0, "3"):
        with pytest.raises(M.InvalidArgumentError, match="sampleSeed"):
            M.find_neighbors(z, z, z, z, z, z, 0.1, 1, True, maxNeighbors=4, sampleSeed=bad)
    for cap0 in ({}, {"maxNeighbors": 0}):
        with pytest.raises(M.InvalidArgumentError, match="sampleSeed"):
            M.find_neighbors(z, z, z, z, z, z, 0.1, 1, True, sampleSeed=3, **cap0)


# ------------------------------------------------------------------------------------------------- 3. the builder
@pytest.fixture()
def shimmed_builder(oracle, monkeypatch):
    """tests/test_neighbor_cap_cpu.py's shims, with a find_neighbors that also takes the seed."""
    import mccnn_amd.MCConvBuilder as MB
    calls = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n = lambda x: x.detach().numpy() if isinstance(x, torch.Tensor) else x

    def shim(name):
        fn = getattr(oracle, name)

        def f(*args, **kwargs):
            calls.append((name, dict(kwargs)))
            K = kwargs.pop("maxNeighbors", 0)
            seed = kwargs.pop("sampleSeed", None)
            assert not kwargs and (seed is None or name == "find_neighbors")
            out = fn(*[n(a) for a in args])
            if name == "find_neighbors" and K:
                out = cap.cap_list(out[0], out[1], K) if seed is None else ref.sample_list(out[0], out[1], K, seed)
            return tuple(t(o) for o in out) if isinstance(out, tuple) else t(out)
        return f

    for nm in ("compute_aabb", "sort_points_step1", "sort_points_step2", "sort_features", "sort_features_back",
               "compute_pdf", "poisson_sampling", "get_sampled_features", "spatial_conv", "transform_indexs",
               "find_neighbors"):
        monkeypatch.setattr(MB, nm, shim(nm))
    monkeypatch.setattr(MB, "get_block_size", lambda: 8)
    return MB, calls


def test_builder_without_a_seed_is_todays(shimmed_builder):
    """sampleSeed=None, given explicitly everywhere: the keys, the op calls and the trace of a builder that was never told
    of seeds, with and without a cap."""
    MB, calls = shimmed_builder
    for K in (0, 7):
        del calls[:]
        cb = MB.ConvolutionBuilder(KDEWindow=0.2, maxNeighbors=K, sampleSeed=None)
        cb.opTrace_ = []
        ph, f3 = _mcclass_s(MB, cb, sampleSeed=None)
        got = list(calls)
        del calls[:]
        cb0 = MB.ConvolutionBuilder(KDEWindow=0.2, maxNeighbors=K)
        cb0.opTrace_ = []
        ph0, f30 = _mcclass_s(MB, cb0)
        assert got == calls and cb.opTrace_ == cb0.opTrace_   # (the outputs are not compared: each builder draws its own weights)
        assert all("sampleSeed" not in kw for _, kw in got)
        assert [kw for name, kw in got if name == "find_neighbors"] == [{"maxNeighbors": 7}] * 3 if K else all(not kw for _, kw in got)
        keys = cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, K)
        assert keys == cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, K, None)
        kG = "MCClassS_PH|0|0.2|True"
        tail = "|7" if K else ""
        assert keys == (kG, kG + "|MCClassS_PH|1" + tail, kG + "|MCClassS_PH|1|0.2|True" + tail)


def test_builder_keys_seeds_and_ops_with_a_seed(shimmed_builder):
    MB, calls = shimmed_builder
    cb = MB.ConvolutionBuilder(KDEWindow=0.2, maxNeighbors=7, sampleSeed=5)
    assert cb.sampleSeed_ == 5
    cb.opTrace_ = []
    ph, f3 = _mcclass_s(MB, cb)
    k7 = cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 7)
    k75 = cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 7, 5)
    k76 = cb.__compute_dic_keys__(ph, ph, 0, 1, 0.2, 0.2, True, True, 7, 6)
    assert k7[0] == k75[0] == k76[0]                                                  # the grid is shared
    assert k75[1] == k7[1] + "|s5" and k75[2] == k7[2] + "|s5" and k76[1] == k7[1] + "|s6"
    assert k75[1].endswith("|7|s5")                                                  # after the cap
    # the op's seed: the builder's plus the CRC-32 of the layer's neighbour key without the seed part
    searches = [kw for name, kw in calls if name == "find_neighbors"]
    layer_keys = [r[1] for r in cb.opTrace_ if r[0] == "find_neighbors"]
    assert len(searches) == 3 and len(set(layer_keys)) == 3 and layer_keys[0] == k75[1]
    for kw, key in zip(searches, layer_keys):
        assert key.endswith("|s5")
        assert kw == {"maxNeighbors": 7, "sampleSeed": (5 + zlib.crc32(key[:-3].encode())) & 0xFFFFFFFF}
    assert len({kw["sampleSeed"] for kw in searches}) == 3
    assert k75[1] in cb.cacheNeighs_ and k75[2] in cb.cachePDFs_ and k7[1] not in cb.cacheNeighs_
    st, pk = cb.cacheNeighs_[k75[1]]
    assert ref.row_lengths(st.numpy(), len(pk)).max() <= 7
    assert [r[0] for r in cb.opTrace_ if r[0] != "spatial_conv"] == ["sort_points_step1", "sort_points_step2",
                                                                    "find_neighbors", "compute_pdf"] * 3
    # the attribute is reassigned between steps: other keys, another draw, the same grid; wrap-around of the sum
    n = len(calls)
    cb.sampleSeed_ = 2 ** 32 - 1
    feats = torch.ones((ph.points_[0].shape[0], 1), dtype=torch.float32)
    conv1 = lambda **kw: cb.create_convolution("Conv_1", ph, 0, feats, 1, 0.2, outPointLevel=1, multiFeatureConv=True,
                                               outNumFeatures=16, **kw)
    out_a = conv1()
    new = [c for c in calls[n:] if c[0] == "find_neighbors"]
    assert new == [("find_neighbors", {"maxNeighbors": 7, "sampleSeed": (2 ** 32 - 1 + zlib.crc32(k7[1].encode())) & 0xFFFFFFFF})]
    assert [c[0] for c in calls[n:]].count("sort_points_step1") == 0 and k7[1] + "|s4294967295" in cb.cacheNeighs_
    # a seed of the layer's own overrides the builder's; the same seed again is a cache hit
    n = len(calls)
    out_b = conv1(sampleSeed=6)
    assert [c for c in calls[n:] if c[0] == "find_neighbors"] == [
        ("find_neighbors", {"maxNeighbors": 7, "sampleSeed": (6 + zlib.crc32(k7[1].encode())) & 0xFFFFFFFF})]
    n = len(calls)
    out_b2 = conv1(sampleSeed=6)
    assert not [c for c in calls[n:] if c[0] == "find_neighbors"] and torch.equal(out_b, out_b2)
    assert torch.equal(out_a, out_b)     # (no row of this level exceeds the cap: the draw changes nothing)
    # the next step: another seed and reset() -- a level whose rows exceed the cap gets another list of the same shape
    key2 = layer_keys[1]
    st5, pk5 = cb.cacheNeighs_[key2]
    assert ref.row_lengths(st5.numpy(), len(pk5)).max() == 7
    cb.sampleSeed_ = 6
    cb.reset()
    assert not cb.cacheNeighs_
    _mcclass_s(MB, cb)
    st6, pk6 = cb.cacheNeighs_[key2[:-1] + "6"]
    assert key2 not in cb.cacheNeighs_ and torch.equal(st5, st6) and pk5.shape == pk6.shape and not torch.equal(pk5, pk6)
    # a layer without a cap ignores the builder's seed, but refuses one of its own; bad seeds
    n = len(calls)
    conv1(maxNeighbors=0)
    assert [c for c in calls[n:] if c[0] == "find_neighbors"] == [("find_neighbors", {})]
    with pytest.raises(ValueError, match="sampleSeed"):
        conv1(maxNeighbors=0, sampleSeed=3)
    with pytest.raises(ValueError, match="sampleSeed"):
        MB.ConvolutionBuilder().create_convolution("Conv_1", ph, 0, feats, 1, 0.2, outPointLevel=1, multiFeatureConv=True,
                                                   outNumFeatures=16, sampleSeed=3)
    for bad in (-1, 2 ** 32, 1.5, True, "3"):
        with pytest.raises(ValueError, match="sampleSeed"):
            MB.ConvolutionBuilder(maxNeighbors=7, sampleSeed=bad)
        with pytest.raises(ValueError, match="sampleSeed"):
            conv1(sampleSeed=bad)
    cb.sampleSeed_ = -4
    with pytest.raises(ValueError, match="sampleSeed"):
        conv1()
