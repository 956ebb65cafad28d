"""Segmentation counts on the GPU (mccnn_seg_counts_add, MCConvModule.segmentation_counts, native.segmentation_counts,
MCNetworkUtils.segmentation_counts with VariableStore(fusedLoss=True), the --parts network of examples/mcclass_s.py) against
the NumPy model of tests/seg_counts_ref.py. Every comparison of counts is exact integer equality."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import seg_counts_ref as ref  # noqa: E402

ROUTES = ("abi", "glue", "native")


def _dev(a, offset=False):
    """`a` on the GPU; offset: as a contiguous view that starts 4 bytes into its buffer."""
    import torch
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    v = buf[1:]
    assert v.is_contiguous() and v.data_ptr() - buf.data_ptr() == 4 and v.data_ptr() % 16 == 4
    return v


def _add(route, d, out, offset=False, rows=None):
    """One call of `route` over the rows `rows` (a slice; None: all) of case `d` into the device tensor `out` -> launches."""
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    cut = (lambda a: None if a is None else a[rows]) if rows is not None else (lambda a: a)
    pred, labels, bid, rw = (_dev(cut(d[k]), offset) for k in ("pred", "labels", "bid", "rw"))
    before = lib.mccnn_debug_launch_count()
    if route == "abi":
        _lib.check(lib.mccnn_seg_counts_add(pred.data_ptr(), labels.data_ptr(), _lib.ptr(rw), _lib.ptr(bid), pred.shape[0], d["B"],
                                            d["C"], d["ignore"], out.data_ptr(), _lib.stream_handle()), "seg_counts_add")
    else:
        op = M.segmentation_counts if route == "glue" else native.segmentation_counts
        assert op(pred, labels, d["C"], bid, d["B"], rw, d["ignore"], out=out) is out
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return launches


def _zeros(d):
    import torch
    return torch.zeros((d["B"], d["C"], 3), dtype=torch.int64, device=torch.device("cuda", 0))


def _lds_bytes(d):
    from mccnn_amd import _lib
    return _lib.load().mccnn_seg_counts_lds_bytes(d["B"], d["C"])


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_counts_equal_the_model(mc, name, route):
    """Every shape through the C-ABI, the ctypes op and the extension op: one launch, the model's counts exactly."""
    d, want = ref.case(name)
    out = _zeros(d)
    assert _add(route, d, out) == 1
    got = out.cpu().numpy()
    print("%s/%s: n %d, lds %d bytes, I %d U %d G %d" % ((name, route, d["n"], _lds_bytes(d)) + tuple(got.sum((0, 1)).tolist())))
    assert np.array_equal(got, want)
    if name == "no-table":
        assert _lds_bytes(d) == 0
    else:
        assert _lds_bytes(d) > 0
    if d["n"] > 1:
        assert want[:, :, 0].sum() > 0 and (want[:, :, 1] > want[:, :, 2]).any()      # (hits, and misses into another class)


@pytest.mark.parametrize("route", ROUTES)
def test_views_that_start_four_bytes_into_their_buffers(mc, route):
    """The n = 1000 case with all four inputs misaligned for the 16-byte loads: the scalar form, the same counts."""
    d, want = ref.case("tail-1000")
    assert d["bid"] is not None and d["rw"] is not None
    out = _zeros(d)
    assert _add(route, d, out, offset=True) == 1
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["tail-257", "many", "no-table"])
def test_every_label_ignored_changes_nothing(mc, name, route):
    """All rows dead: counts keep their (non-zero) bytes."""
    import torch
    d0, _ = ref.case(name)
    d = dict(d0)
    d["ignore"] = 2
    d["labels"] = np.full(d["n"], 2, np.int32)
    start = (np.arange(d["B"] * d["C"] * 3, dtype=np.int64).reshape(d["B"], d["C"], 3) * 7919 + 1) << 20
    out = torch.from_numpy(start.copy()).to(torch.device("cuda", 0))
    assert _add(route, d, out) == 1
    assert out.cpu().numpy().tobytes() == start.tobytes()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["interleaved", "no-table", "tail-65"])
def test_accumulation(mc, name, route):
    """Two calls on two halves equal one call on the whole; a second call on the same rows gives exactly twice the counts; a
    non-zero int64 start above 2^32 is kept."""
    import torch
    d, want = ref.case(name)
    half = d["n"] // 2 + 1
    out = _zeros(d)
    assert _add(route, d, out, rows=slice(0, half)) == 1 and _add(route, d, out, rows=slice(half, None)) == 1
    assert np.array_equal(out.cpu().numpy(), want)
    assert _add(route, d, out) == 1
    assert np.array_equal(out.cpu().numpy(), 2 * want)
    start = np.full(want.shape, (1 << 40) + 5, np.int64)
    out = torch.from_numpy(start.copy()).to(out.device)
    _add(route, d, out)
    assert np.array_equal(out.cpu().numpy(), start + want)


def test_three_runs_give_the_same_bytes(mc):
    d, want = ref.case("many")
    runs = []
    for _ in range(3):
        out = _zeros(d)
        _add("abi", d, out)
        runs.append(out.cpu().numpy().tobytes())
    assert runs[0] == runs[1] == runs[2] == want.tobytes()


def test_int64_inputs_and_a_fresh_result(mc):
    """int64 pred / labels of shape (n, 1) are cast; out=None returns a zeroed tensor's counts."""
    import torch
    from mccnn_amd import native
    d, want = ref.case("tail-1000")
    for op in (mc.segmentation_counts, native.segmentation_counts):
        got = op(_dev(d["pred"]).to(torch.int64).reshape(-1, 1), _dev(d["labels"]).to(torch.int64).reshape(-1, 1), d["C"],
                 _dev(d["bid"]).reshape(-1, 1), d["B"], _dev(d["rw"]).reshape(-1, 1), d["ignore"])
        assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["interleaved", "scannet"])
def test_the_helper_takes_the_op(mc, name):
    """MCNetworkUtils.segmentation_counts on GPU tensors: with the switch on one library launch, with it off none and the
    torch code of the same definition -- the model's counts either way; the two scoring rules on the device."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    d, want = ref.case(name)
    pred, labels, bid, rw = (_dev(d[k]) for k in ("pred", "labels", "bid", "rw"))
    for switch, launches in ((True, 1), (False, 0)):
        st = U.VariableStore(fusedLoss=switch)
        out = _zeros(d)
        before = lib.mccnn_debug_launch_count()
        got = U.segmentation_counts(pred, labels, d["C"], bid, d["B"], rw, d["ignore"], out=out, store=st)
        assert lib.mccnn_debug_launch_count() - before == launches and got is out
        assert np.array_equal(got.cpu().numpy(), want)
    s, ws = U.segmentation_scores(got, d["ignore"]), ref.scores(want, d["ignore"])
    assert s.iou.is_cuda and np.abs(s.iou.cpu().numpy() - ws["iou"]).max() <= 1e-12 and np.abs(s.acc.cpu().numpy() - ws["acc"]).max() <= 1e-12
    for f in ("meanIoU", "meanAcc", "totalAcc"):
        assert abs(float(getattr(s, f)) - ws[f]) <= 1e-12, f
    mask = np.random.default_rng(2).random(want.shape[:2]) < 0.6
    p = U.part_iou(got, _dev(mask))
    assert p.is_cuda and np.abs(p.cpu().numpy() - ref.part_iou(want, mask)).max() <= 1e-12


def test_counts_of_a_loss_head(mc):
    """conv_1x1_softmax_cross_entropy (n = 1000, cin = 16, C = 8) with fusedLoss on, then segmentation_counts(head, ...): the
    model over head.pred read back; the I column sums to head.correct, the G column to head.denom."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    n, cin, C = 1000, 16, 8
    x = _dev(rng.standard_normal((n, cin)).astype(np.float32))
    y = rng.integers(0, C, n).astype(np.int32)
    torch.manual_seed(3)
    st = U.VariableStore(device, fusedLoss=True)
    before = lib.mccnn_debug_launch_count()
    head = U.conv_1x1_softmax_cross_entropy("Seg_Logits", x, cin, C, _dev(y), store=st)
    assert lib.mccnn_debug_launch_count() > before and isinstance(head, U.LossHead) and len(head) == 5
    before = lib.mccnn_debug_launch_count()
    got = U.segmentation_counts(head, _dev(y), C, store=st)
    assert lib.mccnn_debug_launch_count() - before == 1
    want = ref.counts(head.pred.cpu().numpy(), y, C)
    assert tuple(got.shape) == (1, C, 3) and np.array_equal(got.cpu().numpy(), want)
    assert int(got[0, :, 0].sum()) == int(head.correct) and int(got[0, :, 2].sum()) == int(head.denom) == n
    assert 0 < int(head.correct) < n


def test_the_parts_network(mc):
    """The --parts network of the example at 2 clouds x 256 points: the counts of either network are the model's over its own
    predictions read back, so where the two networks predict the same the counts are equal; five Adam steps with the switch
    on reduce the loss."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mcclass_s import MCNormS, NUM_PARTS, part_labels, synthetic_normals_batch
    from mccnn_amd import _lib
    lib = _lib.load()
    device = torch.device("cuda", 0)
    B, n, k = 2, 256, 8
    P, Bi, F, N = synthetic_normals_batch(B, n, np.random.default_rng(7), device)
    y = part_labels(N)
    assert y.dtype == torch.int32 and len(np.unique(y.cpu().numpy())) == NUM_PARTS == 8
    torch.manual_seed(9)
    off = MCNormS(1, B, k, device, outFeatures=16)
    with torch.no_grad():
        assert isinstance(off(P, Bi, F, True, partLabels=y, numParts=NUM_PARTS), U.LossHead)     # creates the variables
    on = MCNormS(1, B, k, device, fusedLoss=True, outFeatures=16)
    on.load_state_dict({k_: v.detach().clone() for k_, v in off.state_dict().items()})
    res = {}
    for tag, net, launches in (("off", off, 0), ("on", on, 1)):
        with torch.no_grad():
            head = net(P, Bi, F, True, partLabels=y, numParts=NUM_PARTS)
        before = lib.mccnn_debug_launch_count()
        cnt = U.segmentation_counts(head, y, NUM_PARTS, Bi, B, store=net.store)
        assert lib.mccnn_debug_launch_count() - before == launches, tag
        pred = head.pred.cpu().numpy()
        want = ref.counts(pred, y.cpu().numpy(), NUM_PARTS, Bi.cpu().numpy().reshape(-1), B)
        assert np.array_equal(cnt.cpu().numpy(), want), tag
        assert int(cnt[:, :, 0].sum()) == int(head.correct) and int(cnt[:, :, 2].sum()) == int(head.denom) == B * n
        mask = torch.ones((B, NUM_PARTS), dtype=torch.bool, device=device)
        assert np.abs(U.part_iou(cnt, mask).cpu().numpy() - ref.part_iou(want, np.ones((B, NUM_PARTS), bool))).max() <= 1e-12
        res[tag] = (pred, cnt.cpu().numpy(), float(head.loss))
    same = np.array_equal(res["on"][0], res["off"][0])
    print("loss off %.7g on %.7g; predictions equal: %s (%d rows differ)" % (res["off"][2], res["on"][2], same,
                                                                             int((res["on"][0] != res["off"][0]).sum())))
    if same:
        assert np.array_equal(res["on"][1], res["off"][1])
    opt = torch.optim.Adam(on.parameters(), lr=1e-2)
    losses = []
    for _ in range(5):
        head = on(P, Bi, F, True, partLabels=y, numParts=NUM_PARTS)
        opt.zero_grad(set_to_none=True)
        head.loss.backward()
        opt.step()
        losses.append(float(head.loss.detach()))
    last = float(on(P, Bi, F, True, partLabels=y, numParts=NUM_PARTS).loss.detach())
    print("losses", losses, last)
    assert last < losses[0]
