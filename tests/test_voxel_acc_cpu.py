"""Voxel accuracy without a GPU: the NumPy model of tests/voxel_acc_ref.py against the restated loop of the reference where
that loop is exact, the torch code of MCNetworkUtils.voxel_counts / voxel_scores on CPU tensors against the model -- counts
exactly, as integers -- the ABI, the workspace formula and the argument errors of mccnn_voxel_acc_add, and the checks of the
Python op."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_acc_ref as ref  # noqa: E402

BADARG, TOOLARGE, WORKSPACE = -1, -3, -4
LOOP_CASES = [name for name in ref.SMALL if ref.CASES[name]()["loop"]]


# ------------------------------------------------------------------------------------------------- the model
def test_the_case_table_covers_the_loop():
    assert {"one-row", "planted", "grid-0625", "grid-005", "room", "random-300"} <= set(LOOP_CASES)


@pytest.mark.parametrize("name", LOOP_CASES)
def test_model_equals_the_restated_reference_loop(name):
    """One cloud, the box from the points, label 0 ignored, share 0.3, predictions in range: where the loop's float32 flat id
    separates the occupied triples and stays below 2^24 -- asserted -- the model gives the loop's figures."""
    d, want, dropped = ref.case(name)
    assert d["B"] == 1 and d["bid"] is None and d["ignore"] == 0 and d["share"] == 0.3 and dropped == 0
    assert np.array_equal(d["mn"][0], d["points"].min(0))
    V, G, flat, coords = ref.reference_loop(d["points"], d["pred"], d["labels"], d["C"], d["res"])
    assert ref.loop_is_exact(flat, coords)
    zero = (coords == 0).any(1)
    print("%s: %d rows, %d voxels, %d rows with a coordinate 0" % (name, d["n"], len(np.unique(flat)), int(zero.sum())))
    if name in ("planted", "room"):
        assert zero.sum() == 1                                   # the planted corner and nothing else
    assert np.array_equal(want[0, :, 0], V.astype(np.int64)) and np.array_equal(want[0, :, 1], G.astype(np.int64))
    assert want[0, :, 1].sum() > 0


def test_model_on_the_planted_voxels():
    """The designed multisets, by hand: (V, G) per class."""
    d, want, _ = ref.case("planted")
    #            corner (1,1)   tie->1     tie->2,2   4 vs 1     1,1       2/10       29/100     [4],[4]   [4],[0]   [2,2,1],[1,1,2]
    G = {1: 1 + 1 + 1, 2: 1 + 1 + 1, 3: 1, 4: 1 + 1 + 1}
    V = {1: 1 + 1, 2: 1 + 1, 3: 1, 4: 1}
    assert want[0, :, 1].tolist() == [0] + [G[c] for c in (1, 2, 3, 4)]
    assert want[0, :, 0].tolist() == [0] + [V[c] for c in (1, 2, 3, 4)]
    d2, want2, _ = ref.case("planted-oob")                       # no ignore label: every voxel is valid
    assert d2["ignore"] == -1 and want2[0, :, 1].sum() == len(ref.PLANTED_OOB) + 1
    assert want2[0, 0, 0] >= 1 and want2[0, 0, 1] >= 2           # ([0, 0], [9, -3]): up = 0 = ul


def test_model_on_dead_rows():
    d, want, dropped = ref.case("dead-rows")
    assert dropped == 6            # NaN, +inf, -inf, 4096.0, one ulp above the edge, a whole voxel below the minimum
    pts = np.array(d["points"])
    keep = np.isfinite(pts).all(1)
    assert (pts[keep].max(0) >= 4095.9375).all()                 # the v = 65535 rows are there, and are kept:
    alone = ref.model(pts[keep], d["pred"][keep], d["labels"][keep], 4, d["mn"], d["bid"][keep], 2, d["res"], -1)
    assert np.array_equal(alone[0], want) and alone[1] == 3


def test_the_double_quotient_is_the_integer_rule():
    """(double) g / (double) s < 0.3 agrees with 10 g < 3 s for every 0 <= g <= s < 400."""
    for s in range(1, 400):
        for g in range(s + 1):
            assert (float(g) / float(s) < 0.3) == (10 * g < 3 * s), (g, s)


def test_a_random_cloud_without_the_corner_point_aliases_the_loop():
    """Why the room plants its corner: in a random 4000-point cloud many rows have a coordinate 0 and the loop's flat id
    merges voxels -- the model's tuples do not."""
    rng = np.random.default_rng(41)
    pts = rng.uniform(0.0, 1.0, (4000, 3)).astype(np.float32)
    lab = rng.integers(0, 5, 4000).astype(np.int32)
    _, _, flat, coords = ref.reference_loop(pts, lab, lab, 5)
    print("unique flat ids %d, unique triples %d" % (len(np.unique(flat)), len(np.unique(coords.astype(np.int64), axis=0))))
    assert not ref.loop_is_exact(flat, coords)


# ------------------------------------------------------------------------------------------------- ABI, argument errors
def test_abi_version():
    from mccnn_amd import _lib
    assert _lib.load().mccnn_abi_version() >= 26


def test_header_binding_and_library_agree():
    import re
    import subprocess
    import mccnn_amd.MCConvModule as M
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib, build, dense_glue, native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_voxel_acc_add", "mccnn_voxel_acc_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    assert len(_lib.SIGNATURES["mccnn_voxel_acc_add"][1]) == 17 and len(_lib.SIGNATURES["mccnn_voxel_acc_workspace_bytes"][1]) == 2
    assert "voxel_acc.hip" in build.SOURCES and "voxel_key.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "voxel_acc.hip")) and os.path.exists(os.path.join(build.CSRC, "voxel_key.h"))
    assert M.voxel_counts is dense_glue.voxel_counts and M._voxel_counts_args is dense_glue._voxel_counts_args
    assert callable(native.voxel_counts) and callable(U.voxel_counts) and callable(U.voxel_scores)
    assert U.VoxelScores._fields == ("acc", "meanAcc")
    doc = U.voxel_counts.__doc__
    assert "CLAMPS" in doc and "synchronises" in doc and "2^24" in doc


def test_workspace_bytes_is_the_formula():
    from mccnn_amd import _lib, dense_glue
    q = _lib.load().mccnn_voxel_acc_workspace_bytes
    for n, cap in ((0, 64), (1, 64), (32, 64), (33, 128), (4095, 8192), (4096, 8192), (4097, 16384), (100000, 262144),
                   (600000, 2097152), ((1 << 30) - 1, 1 << 31)):
        assert dense_glue.voxel_cap_rec(n) == cap
        for C in (1, 4, 21):
            assert q(n, C) == cap * (8 + 8 * C), (n, C)
    assert q(600000, 21) == 369098752                            # the 369 MB of six rooms
    assert q(-1, 4) == 0 and q(1 << 30, 4) == 0 and q(10, 0) == 0


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 0x7f0000000000   # a made-up, 16-byte aligned address: never dereferenced, every call below returns before a launch
    names = (("pts", p), ("pred", p), ("labels", p), ("bid", p), ("mn", p), ("n", 300), ("B", 3), ("C", 5), ("ignore", -1),
             ("res", 0.05), ("share", 0.3), ("counts", p), ("dropped", p), ("ws", p), ("ws_bytes", 1 << 20), ("clean", 0),
             ("stream", None))
    add = lambda **k: lib.mccnn_voxel_acc_add(*[k.get(a, d) for a, d in names])  # noqa: E731
    assert add(B=0) == BADARG and add(C=0) == BADARG and add(B=-2) == BADARG and add(C=-1) == BADARG and add(n=-1) == BADARG
    for name in ("pts", "pred", "labels", "mn", "counts", "ws"):
        assert add(**{name: None}) == BADARG, name
        assert add(**{name: None, "n": 0}) == BADARG, name
    for res in (0.0, -0.05, float("inf"), float("nan"), -float("inf")):
        assert add(res=res) == BADARG, res
    assert add(ws=p + 8) == BADARG
    assert add(B=32769) == TOOLARGE and add(B=32768, C=32768) == TOOLARGE and add(n=1 << 30) == TOOLARGE
    assert add(B=32769, n=0) == TOOLARGE and add(B=0, n=1 << 30) == BADARG          # (the argument error comes first)
    # the workspace: cap_min = 512 slots of 48 bytes for n = 300
    assert add(ws_bytes=512 * 48 - 1) == WORKSPACE and add(ws_bytes=0) == WORKSPACE and add(ws_bytes=511 * 48, clean=1) == WORKSPACE
    assert add(n=4095, C=3, ws_bytes=4096 * 32 - 8) == WORKSPACE
    # n == 0: success, nothing launched -- also with the optional inputs absent and no room in the workspace
    assert add(n=0) == 0 and add(n=0, bid=None, dropped=None, ws_bytes=0) == 0
    assert lib.mccnn_debug_launch_count() == before


# ------------------------------------------------------------------------------------------------- the Python op
def test_op_argument_errors_launch_nothing():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    good = dict(points=torch.zeros(6, 3), pred=i32(6), labels=i32(6, 1), numClasses=4, aabbMin=torch.zeros(1, 3))
    bad = [(dict(points=torch.zeros(6, 3, dtype=torch.float64)), "points must be a float32"), (dict(points=[0.0] * 6), "points must be a float32"),
           (dict(points=torch.zeros(6, 2)), r"points must have shape \(n, 3\)"), (dict(points=torch.zeros(12, 3)[::2]), "points must be contiguous"),
           (dict(pred=torch.zeros(6)), "pred must be an int32"), (dict(pred=i32(6, 2)), r"pred must have shape \(n,\) or \(n, 1\)"),
           (dict(pred=i32(12)[::2]), "pred must be contiguous"),
           (dict(labels=torch.zeros(6)), "labels must be an int32"), (dict(labels=i32(5)), "labels must have shape"),
           (dict(labels=i32(12)[::2]), "labels must be contiguous"),
           (dict(numClasses=0), "numClasses >= 1"), (dict(numClasses=4.0), "numClasses >= 1"), (dict(numClouds=0), "numClouds >= 1"),
           (dict(numClouds=True), "numClouds >= 1"), (dict(numClouds=32769, aabbMin=torch.zeros(32769, 3)), "too large"),
           (dict(ignoreLabel=1.5), "integer ignoreLabel"), (dict(ignoreLabel=1 << 31), "integer ignoreLabel"),
           (dict(resolution=0.0), "finite resolution > 0"), (dict(resolution=-1.0), "finite resolution > 0"),
           (dict(resolution=float("nan")), "finite resolution > 0"), (dict(resolution=1e39), "finite resolution > 0"),
           (dict(resolution="5cm"), "number as resolution"), (dict(maxIgnoreShare=None), "number as maxIgnoreShare"),
           (dict(batchIds=torch.zeros(6, dtype=torch.int64)), "batchIds must be an int32"), (dict(batchIds=i32(7)), "batchIds must have shape"),
           (dict(batchIds=i32(12)[::2]), "batchIds must be contiguous"),
           (dict(aabbMin=None), "aabbMin must be a float32"), (dict(aabbMin=torch.zeros(2, 3)), r"aabbMin must have shape \(numClouds, 3\)"),
           (dict(aabbMin=torch.zeros(1, 3, dtype=torch.float64)), "aabbMin must be a float32"),
           (dict(out=torch.zeros(1, 4, 2)), "out must be an int64"), (dict(out=torch.zeros(1, 4, 3, dtype=torch.int64)), "out must have shape"),
           (dict(out=torch.zeros(1, 4, 4, dtype=torch.int64)[:, :, ::2]), "out must be contiguous"),
           (dict(dropped=torch.zeros(1, dtype=torch.int64)), "dropped must be an int32"), (dict(dropped=i32(2)), "dropped must have one element"),
           (dict(), "points must be a CUDA tensor"),
           (dict(pred=torch.zeros(6, 1, dtype=torch.int64), batchIds=i32(6, 1), numClouds=2, aabbMin=torch.zeros(2, 3),
                 out=torch.zeros(2, 4, 2, dtype=torch.int64), dropped=i32(1), resolution=np.float32(0.05)), "points must be a CUDA tensor")]
    for op in (M.voxel_counts, native.voxel_counts):
        for kw, text in bad:   # (the last two: everything in order but on the CPU)
            args = dict(good)
            args.update(kw)
            with pytest.raises(M.InvalidArgumentError, match="voxel_counts.*" + text):
                op(**args)
    assert lib.mccnn_debug_launch_count() == before
    doc = M.voxel_counts.__doc__
    assert "ADDED" in doc and "dead" in doc and "never" in doc


# ------------------------------------------------------------------------------------------------- the helpers on the CPU
def _t(a):
    return None if a is None else torch.from_numpy(np.array(a))


@pytest.mark.parametrize("fusedLoss", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("name", ref.SMALL)
def test_helper_on_cpu_tensors(name, fusedLoss):
    """MCNetworkUtils.voxel_counts on CPU tensors equals the model exactly, counts and dropped, with the switch off AND on (on
    the CPU, on falls back to the torch code); int64 and (n, 1) inputs, a LossHead for pred, and a second call into `out`
    doubles."""
    import mccnn_amd.MCNetworkUtils as U
    d, want, wdrop = ref.case(name)
    st = U.VariableStore(fusedLoss=fusedLoss)
    pts, pred, labels, bid, mn = _t(d["points"]), _t(d["pred"]), _t(d["labels"]), _t(d["bid"]), _t(d["mn"])
    kw = dict(resolution=d["res"], ignoreLabel=d["ignore"], maxIgnoreShare=d["share"])
    assert U._fused_voxel_counts(st, pts, pred, labels, d["C"], bid, d["B"], mn, d["res"], d["ignore"], d["share"], None, None) is None
    dropped = torch.zeros(1, dtype=torch.int32)
    got = U.voxel_counts(pts, pred, labels, d["C"], bid, d["B"], mn, dropped=dropped, store=st, **kw)
    assert got.dtype == torch.int64 and tuple(got.shape) == (d["B"], d["C"], 2)
    assert np.array_equal(got.numpy(), want) and int(dropped) == wdrop
    head = U.LossHead(None, pred.reshape(-1, 1).to(torch.int64), None, None, None)
    again = U.voxel_counts(pts, head, labels.to(torch.int64).reshape(-1, 1), d["C"], None if bid is None else bid.reshape(-1, 1),
                           d["B"], mn, out=got, dropped=dropped, store=st, **kw)
    assert again is got and np.array_equal(got.numpy(), 2 * want) and int(dropped) == 2 * wdrop


@pytest.mark.parametrize("name", ["room", "planted", "two-clouds"])
def test_the_default_box_is_the_per_cloud_minimum(name):
    """aabbMin=None on CPU tensors: the per-cloud minimum of the points, which is these cases' box."""
    import mccnn_amd.MCNetworkUtils as U
    d, want, _ = ref.case(name)
    bid = d["bid"]
    mins = np.stack([d["points"][(bid == b) if bid is not None else slice(None)].min(0) for b in range(d["B"])])
    wmin, _ = ref.model(d["points"], d["pred"], d["labels"], d["C"], mins, bid, d["B"], d["res"], d["ignore"], d["share"])
    got = U.voxel_counts(_t(d["points"]), _t(d["pred"]), _t(d["labels"]), d["C"], _t(bid), d["B"], None, d["res"], d["ignore"], d["share"])
    assert np.array_equal(got.numpy(), wmin)
    if name != "two-clouds":
        assert np.array_equal(wmin, want)
    assert np.array_equal(U._box_min(_t(d["points"]), _t(bid), d["B"]).numpy(), mins)


def test_defaults_are_the_reference():
    import inspect
    import mccnn_amd.MCNetworkUtils as U
    sig = inspect.signature(U.voxel_counts).parameters
    assert list(sig) == ["points", "pred", "labels", "numClasses", "batchIds", "numClouds", "aabbMin", "resolution", "ignoreLabel",
                         "maxIgnoreShare", "out", "dropped", "store"]
    assert sig["resolution"].default == 0.05 and sig["maxIgnoreShare"].default == 0.3 and sig["ignoreLabel"].default == -1
    assert U._voxel_res(0.05) == float(np.float32(0.05)) == float(ref.RES)
    with pytest.raises(ValueError, match="resolution"):
        U.voxel_counts(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 3, resolution=0.0)
    empty = U.voxel_counts(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 3,
                           aabbMin=torch.zeros(1, 3))
    assert tuple(empty.shape) == (1, 3, 2) and int(empty.sum()) == 0


def test_scores_on_hand_computed_counts():
    """Two clouds, C = 4: class 0 ignored; class 1: V 3 of G 4 over both clouds; class 2: G == 0 -> 1.0; class 3: 0 of 2."""
    import mccnn_amd.MCNetworkUtils as U
    cnt = np.array([[[5, 9], [1, 2], [0, 0], [0, 1]], [[0, 0], [2, 2], [0, 0], [0, 1]]], np.int64)
    s = U.voxel_scores(torch.from_numpy(cnt), 0)
    assert isinstance(s, U.VoxelScores) and s.acc.dtype == torch.float64 and s.meanAcc.dim() == 0
    assert s.acc.tolist() == [5.0 / 9.0, 0.75, 1.0, 0.0] and float(s.meanAcc) == (0.75 + 1.0 + 0.0) / 3.0
    assert float(U.voxel_scores(torch.from_numpy(cnt)).meanAcc) == (5.0 / 9.0 + 0.75 + 1.0 + 0.0) / 4.0
    assert float(U.voxel_scores(torch.zeros(1, 3, 2, dtype=torch.int64), 0).meanAcc) == 1.0
    assert float(U.voxel_scores(torch.zeros(1, 1, 2, dtype=torch.int64), 0).meanAcc) == 1.0      # (no class left)
    acc, mean = ref.scores(cnt, 0)
    assert np.abs(s.acc.numpy() - acc).max() <= 1e-15 and abs(float(s.meanAcc) - mean) <= 1e-15
    d, want, _ = ref.case("room")
    acc, mean = ref.scores(want, 0)
    s = U.voxel_scores(torch.from_numpy(want.copy()), 0)
    assert np.abs(s.acc.numpy() - acc).max() <= 1e-12 and abs(float(s.meanAcc) - mean) <= 1e-12 and 0.3 < mean < 1.0


def test_the_example_reports_the_voxel_accuracy():
    import inspect
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import mcclass_s
    src = inspect.getsource(mcclass_s.train_parts)
    assert "voxel_counts" in src and "voxel_scores" in src
