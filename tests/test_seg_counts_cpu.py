"""Segmentation counts and scores without a GPU: the ABI and the argument errors of mccnn_seg_counts_add, which route a shape
takes (mccnn_seg_counts_lds_bytes), the checks of the Python op, and the torch code of MCNetworkUtils.segmentation_counts /
segmentation_scores / part_iou on CPU tensors against the NumPy model of tests/seg_counts_ref.py -- counts exactly, scores
within 1e-12 (float64 divisions of integers below 2^53 and a mean over at most C values)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_counts_ref as ref  # noqa: E402

BADARG, TOOLARGE = -1, -3


# ------------------------------------------------------------------------------------------------- ABI, argument errors
def test_abi_version():
    from mccnn_amd import _lib
    assert _lib.load().mccnn_abi_version() >= 25


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
    for name in ("mccnn_seg_counts_add", "mccnn_seg_counts_lds_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    assert len(_lib.SIGNATURES["mccnn_seg_counts_add"][1]) == 10 and len(_lib.SIGNATURES["mccnn_seg_counts_lds_bytes"][1]) == 2
    assert "seg_counts.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "seg_counts.hip"))
    assert M.segmentation_counts is dense_glue.segmentation_counts and M._seg_counts_args is dense_glue._seg_counts_args
    assert callable(native.segmentation_counts)
    assert U.SegScores._fields == ("iou", "acc", "meanIoU", "meanAcc", "totalAcc")
    assert U.LossHead._fields == ("loss", "pred", "correct", "denom", "logits")     # (keeps its five fields)
    for f in (U.segmentation_counts, U.segmentation_scores, U.part_iou):
        assert callable(f)
    assert "mean" in U.part_iou.__doc__ and "all models" in U.part_iou.__doc__


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 0x7f0000000000   # a made-up address: never dereferenced, every call below returns before a launch
    add = lambda **k: lib.mccnn_seg_counts_add(*[k.get(a, d) for a, d in (  # noqa: E731
        ("pred", p), ("labels", p), ("rw", p), ("bid", p), ("n", 300), ("B", 3), ("C", 5), ("ignore", -1), ("counts", p),
        ("stream", None))])
    assert add(B=0) == BADARG and add(C=0) == BADARG and add(B=-2) == BADARG and add(C=-1) == BADARG and add(n=-1) == BADARG
    for name in ("pred", "labels", "counts"):
        assert add(**{name: None}) == BADARG, name
        assert add(**{name: None, "n": 0}) == BADARG, name
    assert add(B=1 << 20, C=1 << 10) == TOOLARGE and add(B=715827883, C=1) == TOOLARGE and add(B=(1 << 31) - 1, C=(1 << 31) - 1) == TOOLARGE
    assert add(B=1 << 20, C=1 << 10, n=0) == TOOLARGE
    assert add(B=0, C=1 << 30) == BADARG                       # (the argument error comes first)
    # n == 0: success, nothing launched -- also with the optional inputs absent
    assert add(n=0) == 0 and add(n=0, rw=None, bid=None) == 0 and add(n=0, B=715827882, C=1) == 0
    assert lib.mccnn_debug_launch_count() == before


def test_which_route_a_shape_takes():
    """The LDS table for (1, 2) and (32, 50); none for (64, 400): 76 800 words are 307 KB as uint32, more than the 160 KiB of
    LDS a CU has, so any budget sends it to the global-atomic route."""
    from mccnn_amd import _lib
    q = _lib.load().mccnn_seg_counts_lds_bytes
    assert q(1, 2) == 24 and q(32, 50) == 32 * 50 * 3 * 4 and q(3, 5) > 0 and q(7, 6) > 0 and q(1, 21) > 0
    assert q(64, 400) == 0
    assert max(q(B, C) for B in (1, 7, 32, 64, 1000) for C in (1, 21, 50, 400)) <= 80 * 1024   # (two workgroups share a CU)
    assert q(0, 5) == 0 and q(5, 0) == 0 and q(-1, 5) == 0 and q(1 << 20, 1 << 10) == 0


# ------------------------------------------------------------------------------------------------- the Python op
def test_op_argument_errors_launch_nothing():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    good = dict(pred=i32(6), labels=i32(6, 1), numClasses=4)
    bad = [(dict(pred=torch.zeros(6)), "pred must be an int32"), (dict(pred=[0] * 6), "pred must be an int32"),
           (dict(pred=i32(6, 2)), r"pred must have shape \(n,\) or \(n, 1\)"), (dict(pred=i32(2, 3, 1)), "pred must have shape"),
           (dict(pred=i32(12)[::2]), "pred must be contiguous"),
           (dict(labels=torch.zeros(6)), "labels must be an int32"), (dict(labels=i32(5)), "labels must have shape"),
           (dict(labels=i32(12)[::2]), "labels must be contiguous"),
           (dict(numClasses=0), "numClasses >= 1"), (dict(numClasses=4.0), "numClasses >= 1"), (dict(numClouds=0), "numClouds >= 1"),
           (dict(numClouds=True), "numClouds >= 1"), (dict(numClouds=1 << 20, numClasses=1 << 10), "too large"),
           (dict(ignoreLabel=1.5), "integer ignoreLabel"), (dict(ignoreLabel=1 << 31), "integer ignoreLabel"),
           (dict(batchIds=torch.zeros(6, dtype=torch.int64)), "batchIds must be an int32"), (dict(batchIds=i32(7)), "batchIds must have shape"),
           (dict(batchIds=i32(12)[::2]), "batchIds must be contiguous"),
           (dict(weights=torch.ones(6, dtype=torch.float64)), "weights must be a float32"), (dict(weights=torch.ones(1, 6)), "weights must have shape"),
           (dict(weights=torch.ones(12)[::2]), "weights must be contiguous"),
           (dict(weights=torch.ones(6, requires_grad=True)), "no gradient with respect to weights"),
           (dict(out=torch.zeros(1, 4, 3)), "out must be an int64"), (dict(out=torch.zeros(1, 4, 2, dtype=torch.int64)), "out must have shape"),
           (dict(out=torch.zeros(1, 4, 6, dtype=torch.int64)[:, :, ::2]), "out must be contiguous"),
           (dict(numClouds=2, out=torch.zeros(1, 4, 3, dtype=torch.int64)), "out must have shape"),
           (dict(), "pred must be a CUDA tensor"),
           (dict(pred=torch.zeros(6, 1, dtype=torch.int64), batchIds=i32(6, 1), weights=torch.ones(6, 1), numClouds=2,
                 out=torch.zeros(2, 4, 3, dtype=torch.int64)), "pred must be a CUDA tensor")]
    for op in (M.segmentation_counts, native.segmentation_counts):
        for kw, text in bad:   # (the last two: everything in order but on the CPU)
            args = dict(good)
            args.update(kw)
            with pytest.raises(M.InvalidArgumentError, match="segmentation_counts.*" + text):
                op(**args)
    assert lib.mccnn_debug_launch_count() == before
    doc = M.segmentation_counts.__doc__
    assert "ADDED" in doc and "dead row" in doc and "never" in doc


# ------------------------------------------------------------------------------------------------- the helpers on the CPU
def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a)).to(dtype) if dtype else torch.from_numpy(np.array(a))


@pytest.mark.parametrize("fusedLoss", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("name", ref.SMALL)
def test_helper_on_cpu_tensors(name, fusedLoss):
    """MCNetworkUtils.segmentation_counts on CPU tensors equals the model exactly, with the switch off AND on (on the CPU, on
    falls back to the torch code); int64 and (n, 1) inputs, a LossHead for pred, and a second call into `out` doubles."""
    import mccnn_amd.MCNetworkUtils as U
    d, want = ref.case(name)
    st = U.VariableStore(fusedLoss=fusedLoss)
    pred, labels, bid, rw = _t(d["pred"]), _t(d["labels"]), _t(d["bid"]), _t(d["rw"])
    assert U._fused_seg_counts(st, pred, labels, d["C"], bid, d["B"], rw, d["ignore"], None) is None
    got = U.segmentation_counts(pred, labels, d["C"], bid, d["B"], rw, d["ignore"], store=st)
    assert got.dtype == torch.int64 and tuple(got.shape) == (d["B"], d["C"], 3)
    assert np.array_equal(got.numpy(), want)
    head = U.LossHead(None, pred.reshape(-1, 1).to(torch.int64), None, None, None)
    again = U.segmentation_counts(head, labels.to(torch.int64).reshape(-1, 1), d["C"], None if bid is None else bid.reshape(-1, 1),
                                  d["B"], None if rw is None else rw.reshape(-1, 1), d["ignore"], out=got, store=st)
    assert again is got and np.array_equal(got.numpy(), 2 * want)


def test_every_label_ignored_leaves_the_counts_as_they_are():
    import mccnn_amd.MCNetworkUtils as U
    d, _ = ref.case("tail-257")
    labels = np.full(257, 2, np.int32)
    start = np.arange(3 * 5 * 3, dtype=np.int64).reshape(3, 5, 3) + 1
    out = torch.from_numpy(start.copy())
    U.segmentation_counts(_t(d["pred"]), _t(labels), 5, _t(d["bid"]), 3, None, 2, out=out)
    assert np.array_equal(out.numpy(), start)
    assert np.array_equal(ref.counts(d["pred"], labels, 5, d["bid"], 3, None, 2, start=start), start)


def test_model_on_a_hand_computed_case():
    """Five rows, C = 3: a hit of class 1, a miss 1 -> 2, a miss with the prediction out of range, an ignored label, a row of
    another cloud with a bad batch id."""
    got = ref.counts([1, 2, 7, 1, 0], [1, 1, 2, 0, 0], 3, [0, 0, 0, 0, 5], 1, None, 0)
    assert got.tolist() == [[[0, 0, 0], [1, 2, 2], [0, 2, 1]]]
    s = ref.scores(got, 0)
    assert s["iou"].tolist() == [1.0, 0.5, 0.0] and s["acc"].tolist() == [1.0, 0.5, 0.0]
    assert s["meanIoU"] == 0.25 and s["meanAcc"] == 0.25 and s["totalAcc"] == 1.0 / 3.0
    assert ref.part_iou(got, [[False, True, True]]).tolist() == [0.25] and ref.part_iou(got, [[False, False, False]]).tolist() == [1.0]


def _score_cases():
    """Counts with classes nobody has and nobody predicts (U == 0), classes predicted but never there (G == 0), no live row at
    all, and large counts (an epoch's)."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 50, (4, 6)).astype(np.int64)
    cnt = np.stack([a, a + rng.integers(0, 30, (4, 6)), a + rng.integers(0, 20, (4, 6))], 2)
    cnt[:, 1] = 0                       # U == 0 (and G == 0) in every cloud
    cnt[:, 2, 0] = cnt[:, 2, 2] = 0     # G == 0, U > 0: predicted, never there
    cnt[2] = 0                          # a cloud without a live row
    big = cnt * ((1 << 40) + 12345)
    d, want = ref.case("interleaved")
    return [("mixed", cnt, 0), ("mixed-all-classes", cnt, -1), ("ignore-out-of-range", cnt, 9), ("empty", np.zeros((2, 5, 3), np.int64), 0),
            ("one-class-ignored", np.array([[[3, 4, 5]]], np.int64), 0), ("epoch", big, 3), ("drawn", want.copy(), -1)]


@pytest.mark.parametrize("name,cnt,ignore", _score_cases(), ids=[c[0] for c in _score_cases()])
def test_scores_equal_the_model(name, cnt, ignore):
    import mccnn_amd.MCNetworkUtils as U
    got = U.segmentation_scores(torch.from_numpy(cnt), ignore)
    want = ref.scores(cnt, ignore)
    assert isinstance(got, U.SegScores)
    for f in ("iou", "acc"):
        v = getattr(got, f)
        assert v.dtype == torch.float64 and tuple(v.shape) == (cnt.shape[1],)
        assert np.abs(v.numpy() - want[f]).max() <= 1e-12, f
    for f in ("meanIoU", "meanAcc", "totalAcc"):
        v = getattr(got, f)
        assert v.dtype == torch.float64 and v.dim() == 0 and abs(float(v) - want[f]) <= 1e-12, f
    rng = np.random.default_rng(11)
    mask = rng.random(cnt.shape[:2]) < 0.5
    mask[0] = False                                  # an empty mask row: 1.0
    if cnt.shape[0] > 1:
        mask[1] = True
    p = U.part_iou(torch.from_numpy(cnt), torch.from_numpy(mask))
    assert p.dtype == torch.float64 and tuple(p.shape) == (cnt.shape[0],)
    assert np.abs(p.numpy() - ref.part_iou(cnt, mask)).max() <= 1e-12 and float(p[0]) == 1.0
    if name == "empty":
        assert float(got.meanIoU) == 1.0 and float(got.totalAcc) == 1.0 and np.all(p.numpy() == 1.0)
    with pytest.raises(ValueError, match="classMask"):
        U.part_iou(torch.from_numpy(cnt), torch.from_numpy(mask[:, :-1]))


def test_the_parts_network_on_the_cpu(oracle):
    """MCNormS widened to per-point features with the part head, on the CPU path (oracle ops): the default width keeps the
    prediction [N, 3]; with part labels the result is a LossHead whose counts add up to its own correct / denom."""
    import inspect
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import mcclass_s
    import mccnn_amd.MCNetworkUtils as U
    from tests.oracle_ops import OracleOps
    rng = np.random.default_rng(4)
    B, n = 2, 48
    P = torch.from_numpy(rng.random((B * n, 3), dtype=np.float32))
    Bi = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), n).reshape(-1, 1))
    F = torch.ones((B * n, 1))
    N = torch.from_numpy(rng.standard_normal((B * n, 3)).astype(np.float32))
    y = mcclass_s.part_labels(N)
    assert y.dtype == torch.int32 and int(y.min()) >= 0 and int(y.max()) <= 7 and mcclass_s.NUM_PARTS == 8
    assert inspect.signature(mcclass_s.MCNormS.__init__).parameters["outFeatures"].default == 3
    torch.manual_seed(5)
    assert mcclass_s.MCNormS(1, B, 8, torch.device("cpu"), ops=OracleOps(oracle))(P, Bi, F, True).shape == (B * n, 3)
    net = mcclass_s.MCNormS(1, B, 8, torch.device("cpu"), ops=OracleOps(oracle), fusedLoss=True, outFeatures=16)
    head = net(P, Bi, F, True, partLabels=y, numParts=8)
    assert isinstance(head, U.LossHead) and head.pred.shape == (B * n,)
    cnt = U.segmentation_counts(head, y, 8, Bi, B, store=net.store)
    assert np.array_equal(cnt.numpy(), ref.counts(head.pred.numpy(), y.numpy(), 8, Bi.numpy().reshape(-1), B))
    assert int(cnt[:, :, 0].sum()) == int(head.correct) and int(cnt[:, :, 2].sum()) == int(head.denom) == B * n
    src = inspect.getsource(mcclass_s.main)
    assert "--parts" in src and "part_iou" in inspect.getsource(mcclass_s.train_parts)
