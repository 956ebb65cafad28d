"""The last linear layer + softmax cross-entropy as one op on the GPU (mccnn_linear_xent_fwd / _bwd,
MCConvModule.linear_softmax_xent, native.linear_softmax_xent, VariableStore(fusedLoss=True)) against the float64 reference of
tests/xent_ref.py.

The logits are judged against the float64 x @ W + b; everything behind them -- lse, loss, pred, meta and the three gradients --
against the float64 reference evaluated on the GPU's own stored logits (the backward recomputes them with the forward's k
order, so they are the logits it differentiates). Integers are exact. The bar is helpers.assert_float_close: 1e-4 norm-wise
and per element, with its floor."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import helpers  # noqa: E402
import xent_ref as ref  # noqa: E402

GRAD = 0.75
CASES = [(s, hot, wts) for s in ref.SHAPES for hot in (False, True) for wts in (False, True)]
CASE_IDS = ["%dx%dx%d%s%s" % (s + ("-hot" if hot else "", "-weights" if wts else "")) for s, hot, wts in CASES]
_Z64 = {}


def _z64(shape, hot):
    """float64 x @ W + b of a case, computed once and shared (read-only)."""
    key = (shape, hot)
    if key not in _Z64:
        d = ref.case(*shape, hot=hot)
        z = ref.linear(d["x"], d["w"], d["b"])
        z.setflags(write=False)
        _Z64[key] = z
    return _Z64[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))   # (a copy: the cases are read-only)


def _raw_fwd(d, wts, want_logits=True, want_pred=True, rows=None, labels=None, rw=None):
    """The C-ABI forward -> dict(loss, lse, meta, pred, logits, launches), NumPy. rows: only the first `rows` rows; labels /
    rw: in place of the case's."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    cut = slice(None) if rows is None else slice(0, rows)
    x, w, b = _dev(d["x"][cut]), _dev(d["w"]), _dev(d["b"])
    y = _dev((d["labels"] if labels is None else labels)[cut])
    r = _dev((d["rw"] if rw is None else rw)[cut]) if wts else None
    n, cin = x.shape
    c = w.shape[1]
    nan = float("nan")
    loss = torch.full((1,), nan, device=x.device)
    lse = torch.full((n,), nan, device=x.device)
    meta = torch.full((2,), -7, dtype=torch.int32, device=x.device)
    pred = torch.full((n,), -7, dtype=torch.int32, device=x.device) if want_pred else None
    logits = torch.full((n, c), nan, device=x.device) if want_logits else None
    ws = _ws(lib.mccnn_linear_xent_workspace_bytes(n, cin, c), x.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_linear_xent_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), n, cin, c, y.data_ptr(), _lib.ptr(r),
                                         loss.data_ptr(), lse.data_ptr(), meta.data_ptr(), _lib.ptr(pred), _lib.ptr(logits),
                                         ws.data_ptr(), ws.numel(), _lib.stream_handle()), "linear_xent_fwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dict(loss=loss.cpu().numpy(), lse=lse.cpu().numpy(), meta=meta.cpu().numpy(),
                pred=None if pred is None else pred.cpu().numpy(), logits=None if logits is None else logits.cpu().numpy(),
                launches=launches)


def _raw_bwd(d, wts, lse, meta, g=GRAD, want_dx=True, labels=None, rw=None):
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    x, w, b = _dev(d["x"]), _dev(d["w"]), _dev(d["b"])
    y = _dev(d["labels"] if labels is None else labels)
    r = _dev(d["rw"] if rw is None else rw) if wts else None
    ls, mt, gd = _dev(lse), _dev(meta), _dev(np.array([g], np.float32))
    n, cin = x.shape
    c = w.shape[1]
    nan = float("nan")
    dx = torch.full((n, cin), nan, device=x.device) if want_dx else None
    dw = torch.full((cin, c), nan, device=x.device)
    db = torch.full((c,), nan, device=x.device)
    ws = _ws(lib.mccnn_linear_xent_workspace_bytes(n, cin, c), x.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_linear_xent_bwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), n, cin, c, y.data_ptr(), _lib.ptr(r),
                                         ls.data_ptr(), mt.data_ptr(), gd.data_ptr(), _lib.ptr(dx), dw.data_ptr(), db.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _lib.stream_handle()), "linear_xent_bwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dict(dx=None if dx is None else dx.cpu().numpy(), dw=dw.cpu().numpy(), db=db.cpu().numpy(), launches=launches)


_FWD = {}


def _gpu_forward(shape, hot, wts):
    """The storing forward of a case, once per case (read-only)."""
    key = (shape, hot, wts)
    if key not in _FWD:
        _FWD[key] = _raw_fwd(ref.case(*shape, hot=hot), wts)
    return _FWD[key]


@pytest.mark.parametrize("shape,hot,wts", CASES, ids=CASE_IDS)
def test_forward(mc, shape, hot, wts):
    n, _, C = shape
    d = ref.case(*shape, hot=hot)
    got = _gpu_forward(shape, hot, wts)
    helpers.assert_float_close(got["logits"], _z64(shape, hot), what="logits")
    want = ref.forward(got["logits"], d["labels"], d["rw"] if wts else None)
    helpers.assert_float_close(got["lse"], want["lse"], what="lse")
    err = abs(float(got["loss"][0]) - want["loss"])
    print("loss %.7g, reference %.7g, D %d, correct %d" % (got["loss"][0], want["loss"], want["D"], want["correct"]))
    assert err <= 1e-4 * abs(want["loss"])
    if not want["live"].any():
        assert got["loss"].tobytes() == np.zeros(1, np.float32).tobytes()
    assert np.array_equal(got["pred"], np.argmax(got["logits"], 1))
    assert got["meta"].tolist() == [want["D"], want["correct"]]
    assert got["launches"] <= 2
    if n <= 256:
        assert got["launches"] == 1


@pytest.mark.parametrize("shape,hot,wts", CASES, ids=CASE_IDS)
def test_backward(mc, shape, hot, wts):
    """loss_grad = 0.75. The rows of dx of rows that are not live are all-zero bytes; dx not wanted: the other gradients are
    the same bytes."""
    n, _, C = shape
    d = ref.case(*shape, hot=hot)
    rw = d["rw"] if wts else None
    fwd = _gpu_forward(shape, hot, wts)
    want = ref.backward(d["x"], d["w"], fwd["logits"], d["labels"], rw, g=GRAD)
    got = _raw_bwd(d, wts, fwd["lse"], fwd["meta"])
    for k, what in (("dx", "dx"), ("dw", "dW"), ("db", "db")):
        err = np.abs(got[k] - want[k]).max() / max(np.abs(want[k]).max(), 1e-30)
        print("%s: max |diff| / max |ref| = %.3e" % (what, err))
    helpers.assert_float_close(got["dx"], want["dx"], what="dx")
    helpers.assert_float_close(got["dw"], want["dw"], what="dW")
    helpers.assert_float_close(got["db"], want["db"], what="db")
    dead = ~ref.live_rows(d["labels"], C, rw)
    assert got["dx"][dead].tobytes() == np.zeros_like(got["dx"][dead]).tobytes()
    assert got["launches"] <= (3 if n <= 512 else 4)
    got2 = _raw_bwd(d, wts, fwd["lse"], fwd["meta"], want_dx=False)
    assert got2["dw"].tobytes() == got["dw"].tobytes() and got2["db"].tobytes() == got["db"].tobytes()
    assert got2["launches"] <= 3 and got2["launches"] < got["launches"]


@pytest.mark.parametrize("shape", [(65, 64, 40), (300, 40, 130), (4099, 24, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_outputs_not_wanted(mc, shape):
    """logits = NULL and pred = NULL: loss, lse and meta are the bytes of the storing call."""
    d = ref.case(*shape)
    a = _gpu_forward(shape, False, True)
    for kw in (dict(want_logits=False), dict(want_pred=False), dict(want_logits=False, want_pred=False)):
        b = _raw_fwd(d, True, **kw)
        for k in ("loss", "lse", "meta"):
            assert a[k].tobytes() == b[k].tobytes(), (kw, k)
        if kw.get("want_pred", True):
            assert a["pred"].tobytes() == b["pred"].tobytes()
        assert b["launches"] == a["launches"]


def test_rows_do_not_depend_on_the_other_rows(mc):
    """The first 64, 65 and 257 rows of (4099, 24, 40) alone: the same lse, pred and logits bytes for those rows (inside one
    workgroup, across a tile, and the one-launch form against the slabs of the two-launch form)."""
    shape = (4099, 24, 40)
    d = ref.case(*shape)
    a = _gpu_forward(shape, False, True)
    for rows in (64, 65, 257):
        b = _raw_fwd(d, True, rows=rows)
        for k in ("lse", "pred", "logits"):
            assert b[k].tobytes() == a[k][:rows].tobytes(), (rows, k)


@pytest.mark.parametrize("shape,hot", [((65, 64, 40), False), ((300, 40, 130), True), ((1000, 130, 65), False), ((4099, 24, 40), True)],
                         ids=lambda v: "%dx%dx%d" % v if isinstance(v, tuple) else ("hot" if v else "plain"))
def test_two_runs_give_the_same_bytes(mc, shape, hot):
    d = ref.case(*shape, hot=hot)
    a, b = _raw_fwd(d, True), _raw_fwd(d, True)
    for k in ("loss", "lse", "pred", "meta", "logits"):
        assert a[k].tobytes() == b[k].tobytes(), k
    ga, gb = _raw_bwd(d, True, a["lse"], a["meta"]), _raw_bwd(d, True, a["lse"], a["meta"])
    for k in ("dx", "dw", "db"):
        assert ga[k].tobytes() == gb[k].tobytes(), k


@pytest.mark.parametrize("shape", [(63, 5, 3), (300, 64, 64), (4099, 24, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_no_live_row(mc, shape):
    """All weights 0, and all labels out of range: loss +0.0, D = 1, correct = 0, every gradient all-zero bytes, no NaN."""
    n, _, C = shape
    d = ref.case(*shape, hot=True)
    outside = np.where(np.arange(n) % 2 == 0, -1, C).astype(np.int32)
    for wts, kw in ((True, dict(rw=np.zeros(n, np.float32))), (False, dict(labels=outside)), (True, dict(labels=outside))):
        f = _raw_fwd(d, wts, **kw)
        assert f["loss"].tobytes() == np.zeros(1, np.float32).tobytes() and f["meta"].tolist() == [1, 0]
        assert np.isfinite(f["lse"]).all() and np.isfinite(f["logits"]).all()
        assert np.array_equal(f["pred"], np.argmax(f["logits"], 1))
        g = _raw_bwd(d, wts, f["lse"], f["meta"], **kw)
        for k in ("dx", "dw", "db"):
            assert g[k].tobytes() == np.zeros_like(g[k]).tobytes(), k


def _through_autograd(op, d, wts, scale=None, want_dx=True, want_logits=True, labels64=False):
    """An op entry forward + backward through torch.autograd -> (bytes of loss, pred, meta, logits, dx, dW, db; the outputs)."""
    import torch
    t = {k: _dev(d[k]).requires_grad_(k != "x" or want_dx) for k in ("x", "w", "b")}
    y = _dev(d["labels"])
    if labels64:
        y = y.to(torch.int64).reshape(-1, 1)
    out = op(t["x"], t["w"], t["b"], y, _dev(d["rw"]) if wts else None, want_logits)
    loss = out[0]
    (loss if scale is None else scale * loss).backward()
    torch.cuda.synchronize()
    outs = [loss.detach().reshape(1), out[1], out[2], out[3] if want_logits else torch.zeros(1),
            t["x"].grad if want_dx else torch.zeros(1), t["w"].grad, t["b"].grad]
    return [o.cpu().numpy().tobytes() for o in outs], out


@pytest.mark.parametrize("shape", [(65, 64, 40), (1000, 130, 65), (4099, 24, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_extension_equals_ctypes_and_the_raw_calls(mc, shape):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    d = ref.case(*shape)
    assert native._EXT is not None, "the torch extension did not load"
    fwd = _gpu_forward(shape, False, True)
    for scale, g in ((None, 1.0), (2.0, 2.0)):
        a, oa = _through_autograd(M.linear_softmax_xent, d, True, scale)
        e, oe = _through_autograd(native.linear_softmax_xent, d, True, scale)
        assert a == e
        raw = _raw_bwd(d, True, fwd["lse"], fwd["meta"], g=g)
        want = [fwd["loss"], fwd["pred"], fwd["meta"], fwd["logits"], raw["dx"], raw["dw"], raw["db"]]
        assert a == [v.tobytes() for v in want]
    assert type(oa[0].grad_fn).__name__ == "_LinearSoftmaxXentBackward" and type(oe[0].grad_fn).__name__ != type(oa[0].grad_fn).__name__
    for o in (oa, oe):
        assert o[0].dim() == 0 and o[0].dtype == torch.float32 and o[0].requires_grad
        assert o[1].dtype == torch.int32 and o[2].dtype == torch.int32 and tuple(o[2].shape) == (2,)
        assert not o[1].requires_grad and not o[2].requires_grad and not o[3].requires_grad
    # int64 labels of shape (n, 1), no dx, no logits: the same bytes for the rest
    for op in (M.linear_softmax_xent, native.linear_softmax_xent):
        b, ob = _through_autograd(op, d, True, want_dx=False, want_logits=False, labels64=True)
        assert ob[3] is None and b[:3] == a[:3]
        assert b[5:] == _through_autograd(op, d, True, want_dx=True)[0][5:]
    # once differentiable
    for op in (M.linear_softmax_xent, native.linear_softmax_xent):
        t = [_dev(d[k]).requires_grad_(True) for k in ("x", "w", "b")]
        loss = op(*t, _dev(d["labels"]))[0]
        (gx,) = torch.autograd.grad(loss, t[0], create_graph=True)
        with pytest.raises(RuntimeError):
            gx.sum().backward()


def _grad_errors(got, want, cancelling=None):
    """Per tensor: max |got - want| / scale. A tensor's scale is its largest |want|, never taken below 1e-3 of the largest
    gradient of the network (the rule of tests/test_gpu_linear_bn.py's twin test). cancelling: name -> scale for the
    gradients that are cancelling sums with a true value of 0 -- a bias in front of a batch norm, db = sum_i dz[i, :] -- whose
    own magnitude is rounding noise and no scale at all: they are held to the largest column sum of |dz|, as
    tests/test_gpu_linear_bn.py holds db."""
    gmax = max(float(np.abs(v).max()) for v in want.values())
    scale = {k: max(float(np.abs(want[k]).max()), 1e-3 * gmax) for k in want}
    scale.update(cancelling or {})
    return {k: float(np.abs(got[k] - want[k]).max() / scale[k]) for k in want}


def _mlp2_dz_scales(sd, x, labels, rw):
    """MLP_2_hidden(labels=...) without dropout in training mode, restated in float64 torch on the CPU from the variables `sd`
    -> the largest column sum of |dz| in front of each hidden batch norm, and of the gradient of the first layer's input: the
    scales of the gradients of M2_biases1, M2_biases2 and M2_BN_Init/beta, three shifts that the next batch norm removes (true
    value 0). Nothing of the library runs here."""
    import torch
    v = {k: t.detach().double().cpu() for k, t in sd.items()}

    def bn(z, name):
        var, mean = torch.var_mean(z, 0, unbiased=False)
        return (z - mean) * torch.rsqrt(var + 1e-3) * v[name + "/gamma"] + v[name + "/beta"]

    f = bn(torch.from_numpy(x).double(), "M2_BN_Init").requires_grad_(True)
    z1 = f @ v["M2_weights1"] + v["M2_biases1"]
    z1.retain_grad()
    z2 = torch.relu(bn(z1, "M2_BN_h1")) @ v["M2_weights2"] + v["M2_biases2"]
    z2.retain_grad()
    z3 = torch.relu(bn(z2, "M2_BN_h2")) @ v["M2_weights3"] + v["M2_biases3"]
    live = ref.live_rows(labels, z3.shape[1], rw)
    y = torch.from_numpy(np.where(live, labels, -100).astype(np.int64))
    rows = torch.nn.functional.cross_entropy(z3, y, ignore_index=-100, reduction="none")
    if rw is not None:
        rows = rows * torch.from_numpy(rw).double()
    (rows.sum() / max(int(live.sum()), 1)).backward()
    return {"M2_BN_Init/beta": float(f.grad.abs().sum(0).max()), "M2_biases1": float(z1.grad.abs().sum(0).max()),
            "M2_biases2": float(z2.grad.abs().sum(0).max())}


def test_helpers_take_the_op(mc):
    """MLP_2_hidden(labels=...) on (96, 64) features, hidden 32 / 16, 40 classes, no dropout, fused and fusedLinear on:
    fusedLoss on against off from the same seeded initial values -- loss, pred, correct and every parameter gradient at 1e-4
    of each tensor's scale (_grad_errors; the three shifts in front of a batch norm at the scale of their cancelling sums, taken
    from a float64 restatement of the network: _mlp2_dz_scales); the switch on takes the library's single forward launch
    for the head."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    xh = (rng.standard_normal((96, 64)) * 2 + 1).astype(np.float32)
    x = _dev(xh)
    labels = rng.integers(0, 40, 96)
    labels[3], labels[5] = -1, 40
    y = _dev(labels)
    rw = rng.uniform(0.25, 4, 96).astype(np.float32)
    rw[::9] = 0
    for weights in (None, _dev(rw)):
        res = {}
        for on in (False, True):
            torch.manual_seed(6)
            st = U.VariableStore(dev, fused=True, fusedLinear=True, fusedLoss=on)
            xin = x.clone().requires_grad_(True)
            before = lib.mccnn_debug_launch_count()
            head = U.MLP_2_hidden(xin, 64, 32, 16, 40, "M2", 0.5, True, useDropOut=False, store=st, labels=y,
                                  labelWeights=weights, wantLogits=True)
            launches = lib.mccnn_debug_launch_count() - before
            head.loss.backward()
            torch.cuda.synchronize()
            grads = {k: v.grad.detach().cpu().numpy() for k, v in st.named_parameters()}
            grads["x"] = xin.grad.detach().cpu().numpy()
            res[on] = (head, grads, launches, list(st.state_dict().keys()))
            params = dict(st.named_parameters())
        (h1, g1, l1, k1), (h0, g0, l0, k0) = res[True], res[False]
        assert l1 == l0 + 1 and k1 == k0          # (the BN_Init glue and the two hidden layers are library ops either way)
        assert isinstance(h1, U.LossHead) and isinstance(h0, U.LossHead)
        assert "LinearXentBackward" in h1.loss.grad_fn.name()
        lerr = abs(float(h1.loss.detach()) - float(h0.loss.detach())) / abs(float(h0.loss.detach()))
        sums = _mlp2_dz_scales(params, xh, labels, None if weights is None else rw)
        err = _grad_errors(g1, g0, sums)
        worst = max(err, key=err.get)
        print("switch on against off: loss %.1e, worst gradient %.1e (%s); column sums of |dz| %s, largest gradient %.2e" % (
            lerr, err[worst], worst, sums, max(float(np.abs(g).max()) for g in g0.values())))
        assert lerr <= 1e-4
        assert torch.equal(h1.pred, h0.pred) and h1.pred.dtype == h0.pred.dtype == torch.int32
        assert int(h1.correct) == int(h0.correct) and int(h1.denom) == int(h0.denom)
        helpers.assert_float_close(h1.logits.cpu().numpy(), h0.logits.cpu().numpy(), what="logits")
        assert not h1.logits.requires_grad and not h0.logits.requires_grad
        assert set(g1) == set(g0) and "M2_weights3" in g1 and "M2_biases3" in g1
        for k in g0:
            assert err[k] <= 1e-4, (k, err[k])


def test_mcclass_s_with_the_switch_on_matches_switch_off(mc):
    """MCClassS(fused=True, fusedLinear=True, fusedLoss=True) for one training step on 8 x 256 points against fusedLoss=False:
    the same state_dict, batch, labels and dropSeed_. loss at 1e-4, pred and correct exactly, every parameter gradient at 1e-4
    of its scale (_grad_errors); the level sizes are equal."""
    import torch
    from mcclass_s import MCClassS
    from mccnn_amd.workloads import modelnet_like
    B, n, k, ncat = 8, 256, 16, 10
    pts, bids = modelnet_like(n, B, 51)
    dev = torch.device("cuda", 0)
    y = torch.from_numpy(np.random.default_rng(2).integers(0, ncat, B)).to(dev)
    torch.manual_seed(3)
    off = MCClassS(1, B, k, ncat, dev, fused=True, fusedLinear=True)
    P, Bi = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev)
    F = torch.ones((len(pts), 1), device=dev)
    with torch.no_grad():
        off(P, Bi, F, True, keepProbConv=0.8, useConvDropOut=True)   # creates the variables
    sd = {k_: v.detach().clone() for k_, v in off.state_dict().items()}
    on = MCClassS(1, B, k, ncat, dev, fused=True, fusedLinear=True, fusedLoss=True)
    on.load_state_dict(sd)
    off.load_state_dict(sd)                                          # (the moving statistics of the first call undone)
    assert on.store.fusedLoss_ is True and off.store.fusedLoss_ is False
    res = {}
    for tag, net in (("off", off), ("on", on)):
        net.store.dropSeed_, net.store.dropCalls_ = 9, 0
        for p in net.parameters():
            p.grad = None
        head = net(P, Bi, F, True, keepProbConv=0.8, useConvDropOut=True, useDropOutFull=True, labels=y)
        head.loss.backward()
        torch.cuda.synchronize()
        named = dict(net.convBuilder.named_parameters())
        named.update(dict(net.store.named_parameters()))
        res[tag] = (head, {k_: v.grad.detach().cpu().numpy() for k_, v in named.items()}, list(net.state_dict().keys()),
                    [int(p.shape[0]) for p in net.lastHierarchy.points_])
    (h1, g1, k1, s1), (h0, g0, k0, s0) = res["on"], res["off"]
    assert s1 == s0 and k1 == k0 and set(g1) == set(g0)
    assert "LinearXentBackward" in h1.loss.grad_fn.name() and h0.logits is None and h1.logits is None
    lerr = abs(float(h1.loss.detach()) - float(h0.loss.detach())) / abs(float(h0.loss.detach()))
    err = _grad_errors(g1, g0)
    worst = max(err, key=err.get)
    print("switch on against off: loss %.1e, worst gradient %.1e (%s) over %d tensors" % (lerr, err[worst], worst, len(g0)))
    assert lerr <= 1e-4
    assert torch.equal(h1.pred, h0.pred) and int(h1.correct) == int(h0.correct) and int(h1.denom) == int(h0.denom) == B
    for k_ in g0:
        assert err[k_] <= 1e-4, (k_, err[k_])
    # without labels the network returns its logits, whatever the switch says
    with torch.no_grad():
        assert tuple(on(P, Bi, F, False).shape) == (B, ncat)
