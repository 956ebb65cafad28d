"""The fused dense glue on the GPU (mccnn_bn_act_fwd / _bwd, MCConvModule.bn_relu_dropout, native.bn_relu_drop,
VariableStore(fused=True)) against the float64 reference of tests/bn_act_ref.py: every shared case, forward and
backward, the exact dropped set, the ReLU gates outside a narrow band, eval mode, byte reproducibility, the ctypes op
against the extension entry, launch counts, and MCClassS(fused=True) against its CPU twin."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import bn_act_ref as ref  # noqa: E402
import helpers  # noqa: E402

IDS = ["%dx%d" % s for s in ref.SHAPES]
SEED = 77
_REF = {}


def _reference(shape, relu, keepProb):
    """float64 forward of a case, computed once and shared (read-only)."""
    key = (shape, relu, keepProb)
    if key not in _REF:
        n, c = shape
        d = ref.case(n, c)
        mask = None if keepProb is None else ref.keep_mask(SEED, n, c, ref.threshold(keepProb))
        scale = 1.0 if keepProb is None else 1.0 / keepProb
        _REF[key] = (ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, relu, mask, scale), mask, scale)
    return _REF[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))   # (a copy: the cases are read-only)


def _raw_fwd(d, relu, keepProb, training=True, seed=SEED, gamma=None, beta=None):
    """The C-ABI forward -> (y, saved, moving_mean, moving_var, launches), NumPy."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    x = _dev(d["x"])
    g, b = _dev(d["gamma"] if gamma is None else gamma), _dev(d["beta"] if beta is None else beta)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    n, c = x.shape
    thr, scale = _bn_act_args(x, g, b, mm, mv, keepProb, seed)
    y = torch.empty_like(x)
    saved = torch.full((2, c), float("nan"), device=x.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_bn_act_fwd(x.data_ptr(), n, c, g.data_ptr(), b.data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.99, 1e-3,
                                    int(training), int(relu), thr, scale, seed, y.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                                    ws.numel(), _lib.stream_handle()), "bn_act_fwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return y.cpu().numpy(), saved.cpu().numpy(), mm.cpu().numpy(), mv.cpu().numpy(), launches


def _raw_bwd(d, saved, relu, keepProb, want_dx=True, seed=SEED):
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    x, dy, g, b, sv = _dev(d["x"]), _dev(d["dy"]), _dev(d["gamma"]), _dev(d["beta"]), _dev(saved)
    n, c = x.shape
    thr, scale = _bn_act_args(x, g, b, g, g, keepProb, seed)
    dx = torch.empty_like(x) if want_dx else None
    dg, db = torch.empty(c, device=x.device), torch.empty(c, device=x.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_bn_act_bwd(x.data_ptr(), dy.data_ptr(), n, c, g.data_ptr(), b.data_ptr(), sv.data_ptr(), int(relu), thr,
                                    scale, seed, None if dx is None else dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _lib.stream_handle()), "bn_act_bwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return None if dx is None else dx.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy(), launches


@pytest.mark.parametrize("keepProb", [None, 0.7], ids=["nodrop", "drop0.7"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_forward(mc, shape, relu, keepProb):
    d = ref.case(*shape)
    out, _mask, _scale = _reference(shape, relu, keepProb)
    y, saved, mm, mv, launches = _raw_fwd(d, relu, keepProb)
    helpers.assert_float_close(saved[0], out["mean"], what="saved mean")
    helpers.assert_float_close(saved[1], out["rstd"], what="saved rstd")
    helpers.assert_float_close(mm, out["mov_mean"], what="moving mean")
    helpers.assert_float_close(mv, out["mov_var"], what="moving variance")
    helpers.assert_float_close(y, out["y"], what="y")
    assert launches == (1 if shape[0] <= 256 else 2)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_dropped_set_is_exact(mc, shape):
    """relu off, gamma = 1, beta = 10: no kept element is zero, so the zeros of y are the mask's complement."""
    n, c = shape
    d = ref.case(n, c)
    y = _raw_fwd(d, False, 0.7, gamma=np.ones(c, np.float32), beta=np.full(c, 10.0, np.float32))[0]
    assert np.array_equal(y == 0.0, ~ref.keep_mask(SEED, n, c, ref.threshold(0.7)))


def _gpu_gates(shape):
    d = ref.case(*shape)
    return _raw_fwd(d, True, None)[0] > 0.0


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_relu_gates(mc, shape):
    out, _, _ = _reference(shape, True, None)
    gates = _gpu_gates(shape)
    pre = out["pre"]
    band = np.abs(pre) <= 1e-5 * np.abs(pre).max()
    diff = gates != (pre > 0.0)
    assert not (diff & ~band).any()
    assert diff.sum() <= 1e-3 * pre.size


@pytest.mark.parametrize("relu,keepProb", [(True, 0.7), (True, None), (False, 0.7)], ids=["relu-drop", "relu", "linear-drop"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_backward(mc, shape, relu, keepProb):
    """dx, dgamma, dbeta against the reference evaluated with the GPU's own gates; dx not wanted: the same sums, byte for byte."""
    d = ref.case(*shape)
    out, mask, scale = _reference(shape, relu, keepProb)
    saved = _raw_fwd(d, relu, keepProb)[1]
    gates = _gpu_gates(shape) if relu else None
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale, gate=gates)
    dx, dg, db, launches = _raw_bwd(d, saved, relu, keepProb)
    helpers.assert_float_close(dg, rdg, what="dgamma")
    helpers.assert_float_close(db, rdb, what="dbeta")
    helpers.assert_float_close(dx, rdx, what="dx")
    assert launches == (1 if shape[0] <= 256 else 2)
    _, dg2, db2, launches2 = _raw_bwd(d, saved, relu, keepProb, want_dx=False)
    assert dg2.tobytes() == dg.tobytes() and db2.tobytes() == db.tobytes()
    assert launches2 <= launches


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_eval_forward(mc, shape, relu):
    d = ref.case(*shape)
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], False, relu)
    y, _saved, mm, mv, launches = _raw_fwd(d, relu, 0.7, training=False)   # (a keep probability is ignored in eval mode)
    helpers.assert_float_close(y, out["y"], what="eval y")
    assert mm.tobytes() == d["mov_mean"].tobytes() and mv.tobytes() == d["mov_var"].tobytes()
    assert launches == 1


def _through_autograd(op, d, relu, keepProb, want_dx=True):
    """An op entry forward + backward through torch.autograd -> bytes of y, dx, dgamma, dbeta, moving statistics."""
    import torch
    x = _dev(d["x"]).requires_grad_(want_dx)
    g, b = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    y = op(x, g, b, mm, mv, True, relu, keepProb, SEED)
    y.backward(_dev(d["dy"]))
    torch.cuda.synchronize()
    outs = [y.detach(), x.grad if want_dx else torch.zeros(1), g.grad, b.grad, mm, mv]
    return [t.cpu().numpy().tobytes() for t in outs], y


@pytest.mark.parametrize("shape", [(65, 16), (257, 64), (1000, 130), (4099, 33)], ids=lambda s: "%dx%d" % s)
def test_reproducible_and_extension_equals_ctypes(mc, shape):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    d = ref.case(*shape)
    a, y = _through_autograd(M.bn_relu_dropout, d, True, 0.7)
    b, _ = _through_autograd(M.bn_relu_dropout, d, True, 0.7)
    assert a == b                                            # two runs: identical bytes for all outputs
    out, _, _ = _reference(shape, True, 0.7)
    helpers.assert_float_close(y.detach().cpu().numpy(), out["y"], what="op y")
    assert native._EXT is not None, "the torch extension did not load"
    e, ye = _through_autograd(native.bn_relu_drop, d, True, 0.7)
    assert e == a                                            # the extension entry: the same bytes, forward and backward
    assert type(ye.grad_fn).__name__ != "_BnReluDropoutBackward"   # ... through its own C++ node
    e2, _ = _through_autograd(native.bn_relu_drop, d, True, 0.7, want_dx=False)
    assert e2[2:4] == a[2:4]
    # once differentiable
    x = _dev(d["x"]).requires_grad_(True)
    g, bt = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    for op in (M.bn_relu_dropout, native.bn_relu_drop):
        yy = op(x, g, bt, _dev(d["mov_mean"]), _dev(d["mov_var"]), True)
        (gx,) = torch.autograd.grad(yy.sum(), x, create_graph=True)
        with pytest.raises(RuntimeError):
            gx.sum().backward()


@pytest.mark.parametrize("shape", [(65, 16), (257, 64), (4099, 32)], ids=lambda s: "%dx%d" % s)
def test_rows_off_the_16_byte_grid(mc, shape):
    """c % 4 == 0 but x, dy four bytes off a 16-byte boundary: the one-column-per-thread kernels run (no 16-byte access),
    forward and backward, small form and slabs; same bars."""
    import torch
    import mccnn_amd.MCConvModule as M
    n, c = shape
    d = ref.make_case(n, c)

    def off(a):   # a contiguous [n, c] view that starts 4 bytes behind an aligned allocation
        buf = torch.empty(n * c + 1, device=torch.device("cuda", 0))
        v = buf[1:].view(n, c)
        v.copy_(_dev(a))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    x = off(d["x"]).requires_grad_(True)
    g, b = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    y = M.bn_relu_dropout(x, g, b, mm, mv, True, True, 0.7, SEED)
    y.backward(off(d["dy"]))
    torch.cuda.synchronize()
    mask, scale = ref.keep_mask(SEED, n, c, ref.threshold(0.7)), 1.0 / 0.7
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, True, mask, scale)
    helpers.assert_float_close(y.detach().cpu().numpy(), out["y"], what="y")
    helpers.assert_float_close(mv.cpu().numpy(), out["mov_var"], what="moving variance")
    # the op's own gates: where the mask kept an element, y > 0; elsewhere the reference's (the gradient there is zero)
    gates = np.where(mask, y.detach().cpu().numpy() > 0.0, out["pre"] > 0.0)
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], True, mask, scale, gate=gates)
    helpers.assert_float_close(x.grad.cpu().numpy(), rdx, what="dx")
    helpers.assert_float_close(g.grad.cpu().numpy(), rdg, what="dgamma")
    helpers.assert_float_close(b.grad.cpu().numpy(), rdb, what="dbeta")


def test_eval_with_gradients_is_refused(mc):
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    d = ref.case(65, 16)
    for op in (M.bn_relu_dropout, native.bn_relu_drop):
        with pytest.raises(M.InvalidArgumentError):
            op(_dev(d["x"]).requires_grad_(True), _dev(d["gamma"]), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"]), False)


def test_launch_counts_of_the_glue(mc):
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    for n, want in ((200, 1), (256, 1), (257, 2), (5000, 2)):
        x = torch.randn(n, 24, device=dev)
        for fused in (False, True):
            st = U.VariableStore(dev, fused=fused)
            U.batch_norm_RELU_drop_out("L", x, True, True, 0.8, st)            # creates the variables
            before = lib.mccnn_debug_launch_count()
            y = U.batch_norm_RELU_drop_out("L", x, True, True, 0.8, st)
            fwd = lib.mccnn_debug_launch_count() - before
            y.sum().backward()
            bwd = lib.mccnn_debug_launch_count() - before - fwd
            with torch.no_grad():
                before = lib.mccnn_debug_launch_count()
                U.batch_norm_RELU_drop_out("L", x, False, True, 0.8, st)
                ev = lib.mccnn_debug_launch_count() - before
            assert (fwd, bwd, ev) == ((want, want, 1) if fused else (0, 0, 0)), (n, fused, fwd, bwd, ev)
            assert st.dropCalls_ == (2 if fused else 0)
            assert st.variables_["L_BN/gamma"].grad is not None
    torch.cuda.synchronize()


def test_fused_store_matches_the_torch_path(mc):
    """The helpers with fused on against fused off, no dropout: the same values within the f32 bar, the same names."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    dev = torch.device("cuda", 0)
    torch.manual_seed(5)
    x = torch.randn(700, 12, device=dev) * 3 + 5
    res = {}
    for fused in (False, True):
        torch.manual_seed(6)
        st = U.VariableStore(dev, fused=fused)
        outs = [U.batch_norm_RELU_drop_out("A", x, True, False, None, st),
                U.MLP_2_hidden(x, 12, 10, 8, 5, "M2", 0.5, True, useDropOut=False, store=st),
                U.MLP_1_hidden(x, 12, 9, 4, "M1", 0.5, True, useDropOut=False, store=st)]
        with torch.no_grad():
            outs.append(U.MLP_2_hidden(x, 12, 10, 8, 5, "M2", 0.5, False, useDropOut=True, store=st))
        res[fused] = (outs, st.state_dict())
    for a, b in zip(res[True][0], res[False][0]):
        helpers.assert_float_close(a.detach().cpu().numpy(), b.detach().cpu().numpy(), what="helper output")
    assert list(res[True][1].keys()) == list(res[False][1].keys())
    # Statistics whose EXACT value is zero (the moving mean behind a batch norm with beta = 0 and a zero bias: M2_BN_h1)
    # hold only the rounding noise of the matmul in front of them, ~1e-10 here: as tests/test_gpu_end2end.py does for such
    # gradients, the scale a difference is measured against is never taken below 1e-3 of the largest entry of all of them.
    smax = max(float(v.abs().max()) for v in res[False][1].values())
    for k, v in res[False][1].items():
        a, b = res[True][1][k].cpu().numpy(), v.cpu().numpy()
        assert np.abs(a - b).max() <= 1e-4 * max(np.abs(b).max(), 1e-3 * smax), k


def test_mcclass_s_fused_matches_the_cpu_twin(mc):
    """tests/test_gpu_end2end.py's CPU-twin design and bars with the GPU net MCClassS(fused=True): the twin is the CPU net
    with oracle ops and stock torch dense layers; cfg1 shape, conv and full dropout off."""
    import torch
    from mcclass_s import MCClassS
    from oracle.oracle import Oracle
    from tests.oracle_ops import OracleOps
    from mccnn_amd import _lib
    from mccnn_amd.workloads import modelnet_like
    B, n, k, ncat = 32, 1024, 16, 40
    pts, bids = modelnet_like(n, B, 51)
    y = np.random.default_rng(2).integers(0, ncat, B)
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    gnet = MCClassS(1, B, k, ncat, dev, fused=True)
    P, Bi = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev)
    F = torch.ones((len(pts), 1), device=dev)
    gnet.store.fused_ = False
    with torch.no_grad():
        gnet(P, Bi, F, True, useDropOutFull=False)              # creates the variables (the torch path: the parent's state)
    gnet.store.fused_ = True
    cnet = MCClassS(1, B, k, ncat, torch.device("cpu"), ops=OracleOps(Oracle(omp=True)))
    sd = {k_: v.detach().cpu().clone() for k_, v in gnet.state_dict().items()}
    cnet.load_state_dict(sd)
    res = {}
    lib = _lib.load()
    for tag, net, dv in (("gpu", gnet, dev), ("cpu", cnet, torch.device("cpu"))):
        for p in net.parameters():
            p.grad = None
        logits = net(torch.from_numpy(pts).to(dv), torch.from_numpy(bids).to(dv), torch.ones((len(pts), 1), device=dv), True,
                     useDropOutFull=False)
        loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(y).to(dv))
        loss.backward()
        named = dict(net.convBuilder.named_parameters())
        named.update(dict(net.store.named_parameters()))
        res[tag] = (logits.detach().cpu().numpy(), float(loss.detach()), {k_: v.grad.detach().cpu().numpy() for k_, v in named.items()},
                    {k_: v.detach().cpu().numpy() for k_, v in net.state_dict().items()})
    (gl, gloss, gg, gsd), (cl, closs, cg, csd) = res["gpu"], res["cpu"]
    assert gnet.store.dropCalls_ == 0                            # no block dropped
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))  # noqa: E731
    gmax = max(float(np.abs(v).max()) for v in cg.values())
    err = {k_: float(np.abs(gg[k_] - cg[k_]).max() / max(np.abs(cg[k_]).max(), 1e-3 * gmax)) for k_ in cg}
    worst = max(err, key=err.get)
    print("cfg1 end to end, fused glue: logits %.1e loss %.1e worst gradient %.1e (%s) over %d tensors" % (
        rel(gl, cl), abs(gloss - closs), err[worst], worst, len(cg)))
    assert rel(gl, cl) <= 1e-4 and abs(gloss - closs) <= 1e-5 * abs(closs)
    assert set(gg) == set(cg)
    for k_ in cg:
        assert err[k_] <= 1e-4, (k_, err[k_])
    assert set(gsd) == set(csd)
    moving = [k_ for k_ in csd if k_.endswith("/moving_mean") or k_.endswith("/moving_variance")]
    assert len(moving) == 16                                     # eight batch-norm blocks
    # (a moving mean whose exact value is zero -- Final_Logits_BN_h1 sits behind a batch norm with beta = 0 and a zero bias
    # -- holds only the matmul's rounding noise, ~1e-10: the scale is never taken below 1e-3 of the largest moving
    # statistic, the floor the gradients above have)
    smax = max(float(np.abs(csd[k_]).max()) for k_ in moving)
    for k_ in moving:
        assert np.abs(gsd[k_] - csd[k_]).max() <= 1e-4 * max(np.abs(csd[k_]).max(), 1e-3 * smax), k_

    # with the full dropout on: a function of (dropSeed_, dropCalls_)
    def logits_at(seed, calls):
        gnet.store.dropSeed_, gnet.store.dropCalls_ = seed, calls
        with torch.no_grad():
            out = gnet(P, Bi, F, True, useDropOutFull=True)
        assert gnet.store.dropCalls_ == calls + 2                # the two hidden layers of Final_Logits dropped
        return out.cpu().numpy()

    a, b, c = logits_at(4, 0), logits_at(4, 0), logits_at(5, 7)
    assert a.tobytes() == b.tobytes()
    assert not np.array_equal(a, c)
    assert lib.mccnn_debug_launch_count() > 0
