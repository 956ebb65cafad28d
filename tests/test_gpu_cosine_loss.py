"""The cosine-distance loss of normal estimation as one op on the GPU (mccnn_cosine_loss_fwd / _bwd,
MCConvModule.cosine_distance_loss, native.cosine_distance_loss, VariableStore(fusedLoss=True) through
MCNetworkUtils.cosine_distance_loss and MCNormS) against the float64 reference of tests/cosine_ref.py.

Bars. loss, cosSum, angleSum: |got - ref| <= 1e-4 max(sum of |terms|, 1) (cosSum cancels, so the scale is the sum of the absolute
terms). meta is exact. dpred: helpers.assert_float_close (1e-4 norm-wise and per element, with its floor), the clamped rows
and the remaining rows each against their OWN scale -- a clamped row's gradient is 1e6 / (1 / |pred|) times larger and would
hide every other row. With c = 1 the exact gradient of every unclamped row is 0 (u = +-1, v - cos u = 0 identically), so
there the scale is the largest sum of the absolute values of the two terms that cancel (cosine_ref.backward_terms)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import helpers  # noqa: E402
import cosine_ref as ref  # noqa: E402

GRAD = 0.37
CASES = [(s, wts) for s in ref.SHAPES for wts in (False, True)]
CASE_IDS = ["%dx%d%s" % (s + ("-weights" if wts else "",)) for s, wts in CASES]
OFFSET_SHAPES = [(257, 3), (4099, 3)]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def _dev_offset(a):
    """`a` as a contiguous [n, c] view that starts 12 bytes into its buffer."""
    import torch
    a = np.asarray(a, np.float32)
    buf = torch.zeros(a.size + 3, dtype=torch.float32, device=torch.device("cuda", 0))
    buf[3:] = torch.from_numpy(a.reshape(-1)).to(buf.device)
    v = buf[3:].view(a.shape)
    assert v.is_contiguous() and v.data_ptr() - buf.data_ptr() == 12
    return v


def _raw_fwd(pred, target, rw=None, offset=False):
    """The C-ABI forward -> dict(loss, sums, meta, launches), NumPy."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    p, t = (_dev_offset(pred) if offset else _dev(pred)), _dev(target)
    r = None if rw is None else _dev(rw)
    n, c = p.shape
    nan = float("nan")
    loss = torch.full((1,), nan, device=p.device)
    sums = torch.full((2,), nan, device=p.device)
    meta = torch.full((1,), -7, dtype=torch.int32, device=p.device)
    ws = _ws(lib.mccnn_cosine_loss_workspace_bytes(n, c), p.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_cosine_loss_fwd(p.data_ptr(), t.data_ptr(), n, c, _lib.ptr(r), loss.data_ptr(), sums.data_ptr(),
                                         meta.data_ptr(), _lib.ptr(ws), ws.numel(), _lib.stream_handle()), "cosine_loss_fwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dict(loss=loss.cpu().numpy(), sums=sums.cpu().numpy(), meta=meta.cpu().numpy(), launches=launches)


def _raw_bwd(pred, target, rw, meta, g=GRAD, offset=False):
    import torch
    from mccnn_amd import _lib
    lib = _lib.load()
    p, t = (_dev_offset(pred) if offset else _dev(pred)), _dev(target)
    r = None if rw is None else _dev(rw)
    mt, gd = _dev(meta), _dev(np.array([g], np.float32))
    n, c = p.shape
    dp = torch.full((n, c), float("nan"), device=p.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_cosine_loss_bwd(p.data_ptr(), t.data_ptr(), n, c, _lib.ptr(r), mt.data_ptr(), gd.data_ptr(), dp.data_ptr(),
                                         _lib.stream_handle()), "cosine_loss_bwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dict(dpred=dp.cpu().numpy(), launches=launches)


def _check_forward(got, want):
    for name, val, refv, scale in (("loss", got["loss"][0], want["loss"], want["lossAbs"]),
                                   ("cosSum", got["sums"][0], want["cosSum"], want["cosAbs"]),
                                   ("angleSum", got["sums"][1], want["angleSum"], want["angleAbs"])):
        err = abs(float(val) - refv)
        print("%s %.7g, reference %.7g, |diff| / max(sum |terms|, 1) = %.2e" % (name, val, refv, err / max(scale, 1.0)))
        assert err <= 1e-4 * max(scale, 1.0), name
    assert got["meta"].tolist() == [want["D"]]


def _check_grad(got, d, rw, g=GRAD, op=True):
    """op: `got` is the library op's dpred -- its dead rows are all-zero BYTES (torch code may leave -0.0 there)."""
    want = ref.backward(d["pred"], d["target"], rw, g=g)
    terms = ref.backward_terms(d["pred"], d["target"], rw, g=g)
    c = want.shape[1]
    for what, rows in (("clamped rows", d["clamped"]), ("other rows", ~d["clamped"])):
        if not rows.any():
            continue
        scale = ref.grad_scale(want, terms, rows, c)
        diff = np.abs(got[rows] - want[rows])
        print("dpred, %s: max |diff| / scale = %.3e" % (what, diff.max() / max(scale, 1e-30)))
        if c == 1:   # (the exact gradient of an unclamped row is 0: the scale of the terms that cancel -- see the module's text)
            assert diff.max() <= 1e-4 * scale, what
            assert np.all(diff <= 1e-4 * np.abs(want[rows]) + helpers.ELEMENT_FLOOR * scale), what
        else:
            helpers.assert_float_close(got[rows], want[rows], what="dpred, " + what)
    dead = ~ref.live_rows(len(want), rw)
    assert not got[dead].any()
    assert not op or got[dead].tobytes() == np.zeros_like(got[dead]).tobytes()
    assert np.isfinite(got).all()


@pytest.mark.parametrize("shape,wts", CASES, ids=CASE_IDS)
def test_forward_and_backward(mc, shape, wts):
    """Every shape with and without weights (zeros and non-unit values); (257, 3) and (4099, 3) also with pred as a view that
    starts 12 bytes into its buffer -- the same bytes as the aligned tensor's."""
    n, c = shape
    d = ref.case(n, c)
    rw = d["rw"] if wts else None
    want = ref.forward(d["pred"], d["target"], rw)
    got = _raw_fwd(d["pred"], d["target"], rw)
    _check_forward(got, want)
    assert got["launches"] == (1 if n <= 256 else 2)
    back = _raw_bwd(d["pred"], d["target"], rw, got["meta"])
    _check_grad(back["dpred"], d, rw)
    assert back["launches"] == 1
    if shape in OFFSET_SHAPES:
        off = _raw_fwd(d["pred"], d["target"], rw, offset=True)
        _check_forward(off, want)
        offb = _raw_bwd(d["pred"], d["target"], rw, off["meta"], offset=True)
        _check_grad(offb["dpred"], d, rw)
        for k in ("loss", "sums", "meta"):
            assert off[k].tobytes() == got[k].tobytes(), k
        assert offb["dpred"].tobytes() == back["dpred"].tobytes()


@pytest.mark.parametrize("shape", [(64, 3), (257, 3), (300, 5)], ids=lambda s: "%dx%d" % s)
def test_exactly_parallel_rows(mc, shape):
    """pred = 2 target on every row: angleSum is exactly 0, loss within 1e-6 of 0, cosSum within 1e-6 n of n."""
    d = ref.parallel_case(*shape)
    got = _raw_fwd(d["pred"], d["target"])
    print("loss %.3e angleSum %.3e cosSum - n %.3e" % (got["loss"][0], got["sums"][1], got["sums"][0] - shape[0]))
    assert got["sums"][1:].tobytes() == np.zeros(1, np.float32).tobytes()
    assert abs(float(got["loss"][0])) <= 1e-6 and abs(float(got["sums"][0]) - shape[0]) <= 1e-6 * shape[0]
    assert got["meta"].tolist() == [shape[0]]


@pytest.mark.parametrize("shape", [(63, 3), (300, 5), (4099, 3)], ids=lambda s: "%dx%d" % s)
def test_no_live_row(mc, shape):
    """All weights 0: loss +0.0, zero sums, D = 1, dpred all-zero bytes, no NaN anywhere."""
    n, c = shape
    d = ref.case(n, c)
    rw = np.zeros(n, np.float32)
    f = _raw_fwd(d["pred"], d["target"], rw)
    assert f["loss"].tobytes() == np.zeros(1, np.float32).tobytes() and f["sums"].tobytes() == np.zeros(2, np.float32).tobytes()
    assert f["meta"].tolist() == [1]
    g = _raw_bwd(d["pred"], d["target"], rw, f["meta"])
    assert g["dpred"].tobytes() == np.zeros_like(g["dpred"]).tobytes()


@pytest.mark.parametrize("shape", [(65, 3), (257, 3), (4099, 3)], ids=lambda s: "%dx%d" % s)
def test_two_runs_give_the_same_bytes(mc, shape):
    d = ref.case(*shape)
    a, b = _raw_fwd(d["pred"], d["target"], d["rw"]), _raw_fwd(d["pred"], d["target"], d["rw"])
    for k in ("loss", "sums", "meta"):
        assert a[k].tobytes() == b[k].tobytes(), k
    ga, gb = _raw_bwd(d["pred"], d["target"], d["rw"], a["meta"]), _raw_bwd(d["pred"], d["target"], d["rw"], a["meta"])
    assert ga["dpred"].tobytes() == gb["dpred"].tobytes()


def test_launch_counts(mc):
    for n, fwd in ((256, 1), (257, 2)):
        d = ref.case(n, 3)
        f = _raw_fwd(d["pred"], d["target"], d["rw"])
        assert f["launches"] == fwd
        assert _raw_bwd(d["pred"], d["target"], d["rw"], f["meta"])["launches"] == 1


def _through_autograd(op, d, wts, scale=None):
    """An op entry forward + backward through torch.autograd -> (bytes of loss, sums, meta, dpred; the outputs)."""
    import torch
    p = _dev(d["pred"]).requires_grad_(True)
    out = op(p, _dev(d["target"]), _dev(d["rw"]).reshape(-1, 1) if wts else None)
    (out[0] if scale is None else scale * out[0]).backward()
    torch.cuda.synchronize()
    outs = [out[0].detach().reshape(1), out[1], out[2], p.grad]
    return [o.cpu().numpy().tobytes() for o in outs], out


@pytest.mark.parametrize("shape", [(65, 3), (4099, 3)], ids=lambda s: "%dx%d" % s)
def test_extension_equals_ctypes_and_the_raw_calls(mc, shape):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    d = ref.case(*shape)
    assert native._EXT is not None, "the torch extension did not load"
    fwd = _raw_fwd(d["pred"], d["target"], d["rw"])
    for scale, g in ((None, 1.0), (GRAD, GRAD)):
        a, oa = _through_autograd(M.cosine_distance_loss, d, True, scale)
        e, oe = _through_autograd(native.cosine_distance_loss, d, True, scale)
        assert a == e
        raw = _raw_bwd(d["pred"], d["target"], d["rw"], fwd["meta"], g=g)
        assert a == [v.tobytes() for v in (fwd["loss"], fwd["sums"], fwd["meta"], raw["dpred"])]
    assert type(oa[0].grad_fn).__name__ == "_CosineDistanceLossBackward" and type(oe[0].grad_fn).__name__ != type(oa[0].grad_fn).__name__
    for o in (oa, oe):
        assert o[0].dim() == 0 and o[0].dtype == torch.float32 and o[0].requires_grad
        assert o[1].dtype == torch.float32 and tuple(o[1].shape) == (2,) and o[2].dtype == torch.int32 and tuple(o[2].shape) == (1,)
        assert not o[1].requires_grad and not o[2].requires_grad
    # once differentiable; no gradient with respect to the target
    for op in (M.cosine_distance_loss, native.cosine_distance_loss):
        p = _dev(d["pred"]).requires_grad_(True)
        out = op(p, _dev(d["target"]))
        (g1,) = torch.autograd.grad(out[0], p, create_graph=True)
        with pytest.raises(RuntimeError):
            g1.sum().backward()
        with pytest.raises(M.InvalidArgumentError, match="no gradient with respect to target"):
            op(p, _dev(d["target"]).requires_grad_(True))


@pytest.mark.parametrize("wts", [False, True], ids=["plain", "weights"])
def test_the_helper_takes_the_op(mc, wts):
    """MCNetworkUtils.cosine_distance_loss on GPU tensors: with the switch on the library launches (2 forward + 1 backward at 300
    rows) and the bytes are the op's; with it off nothing of the library runs and the torch code matches the reference at the
    same bars; a non-contiguous pred falls back with the switch on and still matches."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    d = ref.case(300, 3)
    rw = d["rw"] if wts else None
    want = ref.forward(d["pred"], d["target"], rw)
    raw = _raw_fwd(d["pred"], d["target"], rw)
    rawb = _raw_bwd(d["pred"], d["target"], rw, raw["meta"])
    wide = torch.zeros((300, 4), device=torch.device("cuda", 0))
    wide[:, :3] = _dev(d["pred"])
    for switch, pred, launches in ((True, _dev(d["pred"]), 3), (False, _dev(d["pred"]), 0), (True, wide[:, :3], 0)):
        st = U.VariableStore(fusedLoss=switch)
        p = pred.detach().requires_grad_(True)
        assert not (launches == 0 and switch) or not p.is_contiguous()
        before = lib.mccnn_debug_launch_count()
        head = U.cosine_distance_loss(p, _dev(d["target"]), None if rw is None else _dev(rw), store=st)
        (GRAD * head.loss).backward()
        torch.cuda.synchronize()
        assert lib.mccnn_debug_launch_count() - before == launches, (switch, launches)
        assert isinstance(head, U.NormalHead)
        for t in (head.loss, head.cosSum, head.angleSum, head.denom):
            assert t.is_cuda and t.dim() == 0
        got = dict(loss=head.loss.detach().reshape(1).cpu().numpy(), sums=torch.stack([head.cosSum, head.angleSum]).cpu().numpy(),
                   meta=head.denom.reshape(1).cpu().numpy())
        _check_forward(got, want)
        _check_grad(p.grad.cpu().numpy(), d, rw, op=bool(launches))
        if launches:
            assert got["loss"].tobytes() == raw["loss"].tobytes() and got["sums"].tobytes() == raw["sums"].tobytes()
            assert p.grad.cpu().numpy().tobytes() == rawb["dpred"].tobytes()
            assert abs(float(U.mean_angle(head)) - want["angleSum"] / want["D"]) <= 1e-4 * np.pi
            assert abs(float(U.reference_angle(head, 3)) - np.arccos(want["cosSum"] / (3 * want["D"]))) <= 1e-4


def test_mcnorm_s_with_the_switch_on_against_off(mc):
    """MCNormS (1 input feature, 4 x 256 points, k = 8) on the ellipsoids' normals: loss and every parameter gradient with the
    switch on within 1e-4 (norm-wise) of the switch-off network's, and five Adam steps with the switch on reduce the loss."""
    import torch
    from mcclass_s import MCNormS, synthetic_normals_batch
    from mccnn_amd import _lib
    lib = _lib.load()
    device = torch.device("cuda", 0)
    B, n, k = 4, 256, 8
    P, Bi, F, N = synthetic_normals_batch(B, n, np.random.default_rng(7), device)
    torch.manual_seed(9)
    off = MCNormS(1, B, k, device)
    with torch.no_grad():
        assert off(P, Bi, F, True).shape == (B * n, 3)     # creates the variables; without normals: the prediction
    on = MCNormS(1, B, k, device, fusedLoss=True)
    on.load_state_dict({k_: v.detach().clone() for k_, v in off.state_dict().items()})
    res = {}
    for tag, net in (("off", off), ("on", on)):
        for q in net.parameters():
            q.grad = None
        head = net(P, Bi, F, True, normals=N)
        head.loss.backward()
        named = dict(net.convBuilder.named_parameters())
        named.update(dict(net.store.named_parameters()))
        res[tag] = (float(head.loss.detach()), {k_: v.grad.detach().cpu().numpy() for k_, v in named.items()}, head)
    (loff, goff, hoff), (lon, gon, hon) = res["off"], res["on"]
    print("loss off %.7g on %.7g; angle off %.5f on %.5f" % (loff, lon, float(hoff.angleSum), float(hon.angleSum)))
    assert type(hon.loss.grad_fn).__name__ != type(hoff.loss.grad_fn).__name__           # (the op's node)
    assert abs(lon - loff) <= 1e-4 * abs(loff) and int(hon.denom) == int(hoff.denom) == B * n
    assert set(gon) == set(goff) and len(gon) >= 12
    # A tensor's scale is its largest entry, never taken below 1e-3 of the network's largest gradient entry (the rule of
    # tests/test_gpu_end2end.py): the bias in front of the batch norm (Conv_1's last) has the true gradient 0 and holds
    # nothing but the rounding noise of the convolution's backward, which is no scale at all.
    gmax = max(float(np.abs(v).max()) for v in goff.values())
    for k_ in goff:
        err = float(np.abs(gon[k_] - goff[k_]).max() / max(np.abs(goff[k_]).max(), 1e-3 * gmax))
        assert err <= 1e-4, (k_, err)
    opt = torch.optim.Adam(on.parameters(), lr=1e-2)
    losses = []
    before = lib.mccnn_debug_launch_count()
    for _ in range(5):
        head = on(P, Bi, F, True, normals=N)
        opt.zero_grad(set_to_none=True)
        head.loss.backward()
        opt.step()
        losses.append(float(head.loss.detach()))
    last = float(on(P, Bi, F, True, normals=N).loss.detach())
    print("losses", losses, last)
    assert lib.mccnn_debug_launch_count() > before and last < losses[0]
