"""The linear layer + dense glue as one op on the GPU (mccnn_linear_bn_act_fwd / _bwd, MCConvModule.linear_bn_relu_dropout,
native.linear_bn_relu_drop, VariableStore(fusedLinear=True)) against the float64 reference of tests/linear_bn_ref.py.

z is judged against the float64 x @ W + b. The columns of the cases are ill-conditioned on purpose (|mean| of hundreds of
std), so rounding z to f32 alone moves y by up to 3.5e-5 of its scale: the batch-norm half -- saved, the moving statistics,
y, the gates and every gradient -- is judged against the float64 reference evaluated on the GPU's own z."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import bn_act_ref as bn  # noqa: E402
import helpers  # noqa: E402
import linear_bn_ref as ref  # noqa: E402

SEED = 77
MODES = [(True, None), (True, 0.7), (False, 0.7)]
MODE_IDS = ["relu", "relu-drop", "linear-drop"]
_Z64 = {}


def _z64(shape):
    """float64 x @ W + b of a case, computed once and shared (read-only)."""
    if shape not in _Z64:
        d = ref.case(*shape)
        z = ref.linear(d["x"], d["w"], d["b"])
        z.setflags(write=False)
        _Z64[shape] = z
    return _Z64[shape]


def _mask(shape, keepProb):
    if keepProb is None:
        return None, 1.0
    return bn.keep_mask(SEED, shape[0], shape[2], bn.threshold(keepProb)), 1.0 / keepProb


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))   # (a copy: the cases are read-only)


def _thr(keepProb):
    if keepProb is None:
        return 1 << 32, 1.0
    return int(float(keepProb) * 4294967296.0), float(np.float32(1.0) / np.float32(keepProb))


def _raw_fwd(d, relu, keepProb, training=True, bf16=False, seed=SEED, gamma=None, beta=None, x=None, rows=None):
    """The C-ABI forward -> dict(z, y, saved, mm, mv, launches), NumPy (y as a torch CPU tensor when bf16). x: a device
    tensor in place of the case's; rows: only the first `rows` rows."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    x = _dev(d["x"] if rows is None else d["x"][:rows]) if x is None else x
    w, b = _dev(d["w"]), _dev(d["b"])
    g, be = _dev(d["gamma"] if gamma is None else gamma), _dev(d["beta"] if beta is None else beta)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    n, cin = x.shape
    cout = w.shape[1]
    thr, scale = _thr(keepProb)
    z = torch.full((n, cout), float("nan"), device=x.device) if training else None
    y = torch.empty((n, cout), dtype=torch.bfloat16 if bf16 else torch.float32, device=x.device)
    saved = torch.full((3, cout), float("nan"), device=x.device) if training else None
    ws = _ws(lib.mccnn_linear_bn_act_workspace_bytes(n, cin, cout), x.device) if training else None
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_linear_bn_act_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), n, cin, cout, g.data_ptr(), be.data_ptr(),
                                           mm.data_ptr(), mv.data_ptr(), 0.99, 1e-3, int(training), int(relu), thr, scale, seed,
                                           _lib.ptr(z), y.data_ptr(), int(bf16), _lib.ptr(saved), _lib.ptr(ws),
                                           0 if ws is None else ws.numel(), _lib.stream_handle()), "linear_bn_act_fwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dict(z=None if z is None else z.cpu().numpy(), y=y.cpu() if bf16 else y.cpu().numpy(),
                saved=None if saved is None else saved.cpu().numpy(), mm=mm.cpu().numpy(), mv=mv.cpu().numpy(), launches=launches)


def _raw_bwd(d, z, saved, relu, keepProb, want_dx=True, seed=SEED, x=None):
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    x = _dev(d["x"]) if x is None else x
    w, zz, dy, g, be, sv = _dev(d["w"]), _dev(z), _dev(d["dy"]), _dev(d["gamma"]), _dev(d["beta"]), _dev(saved)
    n, cin = x.shape
    cout = w.shape[1]
    thr, scale = _thr(keepProb)
    nan = float("nan")
    dx = torch.full((n, cin), nan, device=x.device) if want_dx else None
    dw = torch.full((cin, cout), nan, device=x.device)
    dv = torch.full((3, cout), nan, device=x.device)
    ws = _ws(lib.mccnn_linear_bn_act_workspace_bytes(n, cin, cout), x.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_linear_bn_act_bwd(x.data_ptr(), w.data_ptr(), zz.data_ptr(), dy.data_ptr(), 0, n, cin, cout, g.data_ptr(),
                                           be.data_ptr(), sv.data_ptr(), int(relu), thr, scale, seed, _lib.ptr(dx), dw.data_ptr(),
                                           dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), ws.data_ptr(), ws.numel(),
                                           _lib.stream_handle()), "linear_bn_act_bwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    dv = dv.cpu().numpy()
    return dict(dx=None if dx is None else dx.cpu().numpy(), dw=dw.cpu().numpy(), db=dv[0], dgamma=dv[1], dbeta=dv[2],
                launches=launches)


@pytest.mark.parametrize("relu,keepProb", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_forward(mc, shape, relu, keepProb):
    d = ref.case(*shape)
    got = _raw_fwd(d, relu, keepProb)
    helpers.assert_float_close(got["z"], _z64(shape), what="z")
    mask, scale = _mask(shape, keepProb)
    out = ref.forward(d, True, relu, mask, scale, z=got["z"])
    helpers.assert_float_close(got["saved"][0], out["mean"], what="saved mean")
    helpers.assert_float_close(got["saved"][1], out["rstd"], what="saved rstd")
    helpers.assert_float_close(got["mm"], out["mov_mean"], what="moving mean")
    helpers.assert_float_close(got["mv"], out["mov_var"], what="moving variance")
    helpers.assert_float_close(got["y"], out["y"], what="y")
    assert got["launches"] <= 2


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_eval_forward_and_bf16_rows(mc, shape):
    """Eval: the moving statistics, nothing updated, at most two launches. bf16 y (even cout), eval and training: the
    nearest-even rounding of the f32 y of the same call, byte for byte."""
    import torch
    d = ref.case(*shape)
    got = _raw_fwd(d, True, 0.7, training=False)   # (a keep probability is ignored in eval mode)
    out = ref.forward(d, False, True)
    helpers.assert_float_close(got["y"], out["y"], what="eval y")
    assert got["mm"].tobytes() == d["mov_mean"].tobytes() and got["mv"].tobytes() == d["mov_var"].tobytes()
    assert got["launches"] <= 2
    if shape[2] % 2 == 0:
        for training in (False, True):
            f = _raw_fwd(d, True, 0.7, training=training)
            h = _raw_fwd(d, True, 0.7, training=training, bf16=True)
            assert torch.equal(h["y"].view(torch.int16), torch.from_numpy(f["y"]).to(torch.bfloat16).view(torch.int16))
            assert h["launches"] <= 2
            if training:
                assert h["z"].tobytes() == f["z"].tobytes() and h["saved"].tobytes() == f["saved"].tobytes()


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_dropped_set_is_exact(mc, shape):
    """relu off, gamma = 1, beta = 10: no kept element is zero, so the zeros of y are the mask's complement."""
    n, _, c = shape
    y = _raw_fwd(ref.case(*shape), False, 0.7, gamma=np.ones(c, np.float32), beta=np.full(c, 10.0, np.float32))["y"]
    assert np.array_equal(y == 0.0, ~bn.keep_mask(SEED, n, c, bn.threshold(0.7)))


_GATES = {}


def _gpu_forward_nodrop(shape):
    """(z, gates) of the GPU's relu forward without dropout, once per shape."""
    if shape not in _GATES:
        got = _raw_fwd(ref.case(*shape), True, None)
        _GATES[shape] = (got["z"], got["y"] > 0.0)
    return _GATES[shape]


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_relu_gates(mc, shape):
    z, gates = _gpu_forward_nodrop(shape)
    pre = ref.forward(ref.case(*shape), True, True, z=z)["pre"]
    band = np.abs(pre) <= 1e-5 * np.abs(pre).max()
    diff = gates != (pre > 0.0)
    assert not (diff & ~band).any()
    assert diff.sum() <= 1e-3 * pre.size


@pytest.mark.parametrize("relu,keepProb", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_backward(mc, shape, relu, keepProb):
    """The reference runs in float64 from the GPU's z, saved and gates. saved carries the mean in two parts (its f32 rounding
    and what the exact mean has over it, [3, cout]): their float64 sum is the reference's mean -- on these columns, hundreds
    of std from zero, the f32 mean alone is off by up to 3e-5 std, and a reference normalising with it would differ from
    the gradient by that shift times dbeta, above the bar. db is a cancelling sum whose true value is about 0: it is held
    to 1e-4 of the largest column sum of |dz|. dx not wanted: the other gradients are the same bytes."""
    d = ref.case(*shape)
    mask, scale = _mask(shape, keepProb)
    fwd = _raw_fwd(d, relu, keepProb)
    z, saved = fwd["z"], fwd["saved"]
    gates = _gpu_forward_nodrop(shape)[1] if relu else None
    mean = saved[0].astype(np.float64) + saved[2].astype(np.float64)
    want = ref.backward(d, z.astype(np.float64), mean, saved[1].astype(np.float64), relu, mask, scale, gate=gates)
    got = _raw_bwd(d, z, saved, relu, keepProb)
    helpers.assert_float_close(got["dgamma"], want["dgamma"], what="dgamma")
    helpers.assert_float_close(got["dbeta"], want["dbeta"], what="dbeta")
    helpers.assert_float_close(got["dx"], want["dx"], what="dx")
    helpers.assert_float_close(got["dw"], want["dw"], what="dW")
    db_scale = np.abs(want["dz"]).sum(0).max()
    db_err = np.abs(got["db"] - want["db"]).max()
    print("db: max |diff| %.3e, scale %.3e" % (db_err, db_scale))
    assert db_err <= 1e-4 * db_scale
    assert got["launches"] <= (4 if shape[0] <= 256 else 5)
    got2 = _raw_bwd(d, z, saved, relu, keepProb, want_dx=False)
    for k in ("dw", "db", "dgamma", "dbeta"):
        assert got2[k].tobytes() == got[k].tobytes(), k
    assert got2["launches"] < got["launches"]


@pytest.mark.parametrize("shape", [(65, 16, 16), (300, 64, 128), (1000, 130, 70), (4099, 24, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_reproducible_and_rows_independent(mc, shape):
    d = ref.case(*shape)
    a, b = _raw_fwd(d, True, 0.7), _raw_fwd(d, True, 0.7)
    for k in ("z", "y", "saved", "mm", "mv"):
        assert a[k].tobytes() == b[k].tobytes(), k
    ga, gb = _raw_bwd(d, a["z"], a["saved"], True, 0.7), _raw_bwd(d, a["z"], a["saved"], True, 0.7)
    for k in ("dx", "dw", "db", "dgamma", "dbeta"):
        assert ga[k].tobytes() == gb[k].tobytes(), k
    # rows [0, n') of z from a call on the first n' rows: inside a tile, across a tile, across a slab boundary
    for rows in (1, 37, 65, 129, 300, shape[0] - 1):
        if rows < shape[0]:
            assert _raw_fwd(d, True, 0.7, rows=rows)["z"].tobytes() == a["z"][:rows].tobytes(), rows


@pytest.mark.parametrize("shape", [(65, 16, 16), (4099, 24, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_x_off_the_16_byte_grid(mc, shape):
    """cin % 4 == 0 but x four bytes off a 16-byte boundary: single-float loads, the same bytes as the aligned copy."""
    import torch
    n, cin, _ = shape
    d = ref.case(*shape)
    buf = torch.empty(n * cin + 1, device=torch.device("cuda", 0))
    x = buf[1:].view(n, cin)
    x.copy_(_dev(d["x"]))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    a, b = _raw_fwd(d, True, 0.7), _raw_fwd(d, True, 0.7, x=x)
    for k in ("z", "y", "saved", "mm", "mv"):
        assert a[k].tobytes() == b[k].tobytes(), k
    ga, gb = _raw_bwd(d, a["z"], a["saved"], True, 0.7), _raw_bwd(d, a["z"], a["saved"], True, 0.7, x=x)
    for k in ("dx", "dw", "db", "dgamma", "dbeta"):
        assert ga[k].tobytes() == gb[k].tobytes(), k
    e = _raw_fwd(d, True, None, training=False)["y"]
    assert e.tobytes() == _raw_fwd(d, True, None, training=False, x=x)["y"].tobytes()


def _through_autograd(op, d, keepProb, want_dx=True, outDtype=None):
    """An op entry forward + backward through torch.autograd -> bytes of y, the five gradients and the moving statistics."""
    import torch
    t = {k: _dev(d[k]).requires_grad_(k != "x" or want_dx) for k in ("x", "w", "b", "gamma", "beta")}
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    y = op(t["x"], t["w"], t["b"], t["gamma"], t["beta"], mm, mv, True, True, keepProb, SEED, outDtype=outDtype)
    y.backward(_dev(d["dy"]).to(y.dtype))
    torch.cuda.synchronize()
    outs = [y.detach().float(), t["x"].grad if want_dx else torch.zeros(1), t["w"].grad, t["b"].grad, t["gamma"].grad,
            t["beta"].grad, mm, mv]
    return [o.cpu().numpy().tobytes() for o in outs], y


@pytest.mark.parametrize("shape", [(65, 16, 16), (1000, 130, 70), (4099, 24, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_extension_equals_ctypes_and_the_raw_calls(mc, shape):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    d = ref.case(*shape)
    assert native._EXT is not None, "the torch extension did not load"
    a, ya = _through_autograd(M.linear_bn_relu_dropout, d, 0.7)
    e, ye = _through_autograd(native.linear_bn_relu_drop, d, 0.7)
    assert a == e
    assert type(ya.grad_fn).__name__ == "_LinearBnReluDropoutBackward" and type(ye.grad_fn).__name__ != type(ya.grad_fn).__name__
    fwd = _raw_fwd(d, True, 0.7)
    raw = _raw_bwd(d, fwd["z"], fwd["saved"], True, 0.7)
    want = [fwd["y"], raw["dx"], raw["dw"], raw["db"], raw["dgamma"], raw["dbeta"], fwd["mm"], fwd["mv"]]
    assert a == [v.tobytes() for v in want]
    e2, _ = _through_autograd(native.linear_bn_relu_drop, d, 0.7, want_dx=False)
    assert e2[2:6] == a[2:6]
    if shape[2] % 2 == 0:
        assert _through_autograd(M.linear_bn_relu_dropout, d, 0.7, outDtype=torch.bfloat16)[0] == \
            _through_autograd(native.linear_bn_relu_drop, d, 0.7, outDtype=torch.bfloat16)[0]
    # once differentiable; the eval form refuses gradients
    for op in (M.linear_bn_relu_dropout, native.linear_bn_relu_drop):
        t = [_dev(d[k]).requires_grad_(True) for k in ("x", "w", "b", "gamma", "beta")]
        yy = op(*t, _dev(d["mov_mean"]), _dev(d["mov_var"]), True)
        (gx,) = torch.autograd.grad(yy.sum(), t[0], create_graph=True)
        with pytest.raises(RuntimeError):
            gx.sum().backward()
        with pytest.raises(M.InvalidArgumentError):
            op(*t, _dev(d["mov_mean"]), _dev(d["mov_var"]), False)
        with torch.no_grad():
            ev = op(*t, _dev(d["mov_mean"]), _dev(d["mov_var"]), False)
        assert ev.cpu().numpy().tobytes() == _raw_fwd(d, True, None, training=False)["y"].tobytes()


def test_helpers_take_the_op_and_count_launches(mc):
    """conv_1x1_batch_norm_RELU_drop_out and the MLPs with the switch on: the library's launches, the values of the switch-off
    path within the f32 bar, the same names, dropCalls_ advancing equally."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    torch.manual_seed(5)
    res = {}
    for n, fwd_want in ((200, 1), (700, 2)):
        x = torch.randn(n, 12, device=dev) * 3 + 5
        for fl in (False, True):
            torch.manual_seed(6)
            st = U.VariableStore(dev, fused=True, fusedLinear=fl)
            before = lib.mccnn_debug_launch_count()
            r = U.conv_1x1_batch_norm_RELU_drop_out("R", "R_Out", x, 12, 6, True, True, 0.8, st)
            launches = lib.mccnn_debug_launch_count() - before
            assert launches == (fwd_want if fl else (1 if n <= 256 else 2))
            outs = [r, U.MLP_2_hidden(x, 12, 10, 8, 5, "M2", 0.5, True, useDropOut=True, store=st),
                    U.MLP_1_hidden(x, 12, 9, 4, "M1", 0.5, True, useDropOut=True, store=st)]
            sum(o.sum() for o in outs).backward()
            with torch.no_grad():
                outs.append(U.conv_1x1_batch_norm_RELU_drop_out("R", "R_Out", x, 12, 6, False, True, 0.8, st, outDtype=torch.bfloat16))
            res[fl] = (outs, st.state_dict(), st.dropCalls_, {k: v.grad for k, v in st.named_parameters()})
        assert res[True][2] == res[False][2] == 4
        for a, b in zip(res[True][0], res[False][0]):
            assert a.dtype == b.dtype
            # (bf16 rows: two f32 values 1e-4 apart round to neighbouring bf16 values at the most, 2^-8 apart)
            rtol = 1e-4 if a.dtype == torch.float32 else 1e-4 + 2.0 ** -8
            helpers.assert_float_close(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), rtol=rtol,
                                       what="helper output")
        assert list(res[True][1].keys()) == list(res[False][1].keys())
        assert all(g is not None for g in res[True][3].values())
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", [None, "bf16"], ids=["f32rows", "bf16rows"])
def test_mcclass_s_with_the_switch_on_matches_switch_off(mc, rows):
    """MCClassS(fused=True, fusedLinear=True) against MCClassS(fused=True): the same state_dict, batch and dropSeed_, training
    mode, conv and full dropout on. Bars of tests/test_gpu_bn_act.py's twin test: logits and every parameter gradient at
    1e-4, a gradient's scale never taken below 1e-3 of the largest gradient; the moving statistics likewise."""
    import torch
    from mcclass_s import MCClassS
    from mccnn_amd.workloads import modelnet_like
    B, n, k, ncat = 8, 256, 16, 10
    pts, bids = modelnet_like(n, B, 51)
    y = np.random.default_rng(2).integers(0, ncat, B)
    dev = torch.device("cuda", 0)
    rows = torch.bfloat16 if rows else None
    torch.manual_seed(3)
    off = MCClassS(1, B, k, ncat, dev, fused=True, rows=rows)
    P, Bi = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev)
    F = torch.ones((len(pts), 1), device=dev)
    with torch.no_grad():
        off(P, Bi, F, True, keepProbConv=0.8, useConvDropOut=True)   # creates the variables
    sd = {k_: v.detach().clone() for k_, v in off.state_dict().items()}
    on = MCClassS(1, B, k, ncat, dev, fused=True, rows=rows, fusedLinear=True)
    on.load_state_dict(sd)
    off.load_state_dict(sd)                                          # (the moving statistics of the first call undone)
    res = {}
    for tag, net in (("off", off), ("on", on)):
        net.store.dropSeed_, net.store.dropCalls_ = 9, 0
        for p in net.parameters():
            p.grad = None
        logits = net(P, Bi, F, True, keepProbConv=0.8, useConvDropOut=True, useDropOutFull=True)
        torch.nn.functional.cross_entropy(logits, torch.from_numpy(y).to(dev)).backward()
        named = dict(net.convBuilder.named_parameters())
        named.update(dict(net.store.named_parameters()))
        res[tag] = (logits.detach().cpu().numpy(), {k_: v.grad.detach().cpu().numpy() for k_, v in named.items()},
                    {k_: v.detach().cpu().numpy() for k_, v in net.state_dict().items()}, net.store.dropCalls_)
    (gl, gg, gsd, gcalls), (cl, cg, csd, ccalls) = res["on"], res["off"]
    assert gcalls == ccalls == 7                                     # five blocks around the convolutions, two in the MLP
    assert list(gsd.keys()) == list(csd.keys()) and set(gg) == set(cg)
    gmax = max(float(np.abs(v).max()) for v in cg.values())
    err = {k_: float(np.abs(gg[k_] - cg[k_]).max() / max(np.abs(cg[k_]).max(), 1e-3 * gmax)) for k_ in cg}
    worst = max(err, key=err.get)
    lerr = float(np.abs(gl - cl).max() / np.abs(cl).max())
    print("switch on against off: logits %.1e, worst gradient %.1e (%s) over %d tensors" % (lerr, err[worst], worst, len(cg)))
    assert lerr <= 1e-4
    for k_ in cg:
        assert err[k_] <= 1e-4, (k_, err[k_])
    moving = [k_ for k_ in csd if k_.endswith("/moving_mean") or k_.endswith("/moving_variance")]
    assert len(moving) == 16
    smax = max(float(np.abs(csd[k_]).max()) for k_ in moving)
    for k_ in moving:
        assert np.abs(gsd[k_] - csd[k_]).max() <= 1e-4 * max(np.abs(csd[k_]).max(), 1e-3 * smax), k_
