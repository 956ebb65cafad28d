"""The dense glue over a concatenation on the GPU (mccnn_bn_act_cat_fwd / _bwd, dense_glue.bn_relu_dropout_cat,
native.bn_relu_drop_cat, VariableStore(fused=True, fusedCat=True)) on the cases of tests/bn_cat_ref.py: forward and backward
against the float64 reference of the whole [n, C] array with the bars and the GPU's-own-gates design of
tests/test_gpu_bn_act.py, the exact dropped set under global column indices, and -- wherever the library takes the plan of
the contiguous op -- every output byte for byte that of mccnn_bn_act_fwd_rows / _bwd_rows on torch.cat(xs, 1), computed in
the same test. Eval, bf16 y / dy, segments without a gradient, reproducibility, the extension route, launch counts, and
batch_norm_RELU_drop_out on a list."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bn_act_ref as ref  # noqa: E402
import bn_cat_ref as cat  # noqa: E402
import helpers  # noqa: E402

SEED = 77
_REF = {}


def _reference(c, relu, keepProb):
    """float64 forward of a case over the whole [n, C] array, computed once and shared (read-only)."""
    key = (c, relu, keepProb)
    if key not in _REF:
        n, w = c.n, cat.width(c)
        d = cat.data(c)
        mask = None if keepProb is None else ref.keep_mask(SEED, n, w, ref.threshold(keepProb))
        scale = 1.0 if keepProb is None else 1.0 / keepProb
        _REF[key] = (ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, relu, mask, scale), mask, scale)
    return _REF[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))   # (a copy: the cases are read-only)


def _off(a):
    """A contiguous device copy of `a` that starts 4 bytes behind a 16-byte boundary."""
    import torch
    buf = torch.empty(a.size + 1, device=torch.device("cuda", 0))
    v = buf[1:].view(*a.shape)
    v.copy_(_dev(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _segments(c, a):
    """The column blocks of a [n, C] array as device tensors, each contiguous; the `off` ones 4 bytes off the 16-byte grid."""
    return [_off(s) if k in c.off else _dev(s) for k, s in enumerate(cat.split(a, c.widths))]


def _table(ts):
    return ((C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts]),
            (C.c_int * len(ts))(*[0 if t is None else t.shape[1] for t in ts]))


def _thr(keepProb):
    return ref.threshold(keepProb), 1.0 if keepProb is None else float(np.float32(1.0) / np.float32(keepProb))


def _ydtype(bf16):
    import torch
    return torch.bfloat16 if bf16 else torch.float32


def _np(t):
    import torch
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _raw_fwd(c, relu, keepProb, training=True, gamma=None, beta=None, y_bf16=False, plain=False):
    """The C-ABI forward over the segments (plain: mccnn_bn_act_fwd_rows on their torch.cat) -> (y, saved, moving_mean,
    moving_var, launches), NumPy (a bf16 y as its int16 bits)."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    d = cat.data(c)
    xs = _segments(c, d["x"])
    g, b = _dev(d["gamma"] if gamma is None else gamma), _dev(d["beta"] if beta is None else beta)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    n, w = c.n, cat.width(c)
    thr, scale = _thr(keepProb)
    y = torch.empty((n, w), dtype=_ydtype(y_bf16), device=g.device)
    saved = torch.full((2, w), float("nan"), device=g.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, w), g.device)
    tail = (g.data_ptr(), b.data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.99, 1e-3, int(training), int(relu), thr, scale, SEED,
            y.data_ptr(), int(y_bf16), saved.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    if plain:
        x = torch.cat(xs, 1)
        assert x.data_ptr() % 16 == 0
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_act_fwd_rows(x.data_ptr(), 0, n, w, *tail), "bn_act_fwd_rows")
    else:
        px, cs = _table(xs)
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_act_cat_fwd(px, cs, len(xs), n, *tail), "bn_act_cat_fwd")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return _np(y), saved.cpu().numpy(), mm.cpu().numpy(), mv.cpu().numpy(), launches


def _raw_bwd(c, saved, relu, keepProb, want=None, dy_bf16=False, plain=False):
    """The C-ABI backward -> (dxs, dgamma, dbeta, launches). want: per segment whether dx_s is asked for (None: all; all
    False: dxs == NULL). plain: mccnn_bn_act_bwd_rows on torch.cat(xs, 1), its dx cut into the column slices."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    d = cat.data(c)
    xs = _segments(c, d["x"])
    dy = _dev(d["dy"]).to(_ydtype(dy_bf16))
    g, b, sv = _dev(d["gamma"]), _dev(d["beta"]), _dev(saved)
    n, w = c.n, cat.width(c)
    thr, scale = _thr(keepProb)
    want = [True] * len(xs) if want is None else list(want)
    dg, db = torch.empty(w, device=g.device), torch.empty(w, device=g.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, w), g.device)
    tail = (dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    if plain:
        x = torch.cat(xs, 1)
        dx = torch.empty_like(x) if any(want) else None
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_act_bwd_rows(x.data_ptr(), 0, dy.data_ptr(), int(dy_bf16), n, w, g.data_ptr(), b.data_ptr(),
                                             sv.data_ptr(), int(relu), thr, scale, SEED, None if dx is None else dx.data_ptr(), *tail),
                   "bn_act_bwd_rows")
        launches = lib.mccnn_debug_launch_count() - before
        torch.cuda.synchronize()
        dxs = [None] * len(xs) if dx is None else [s if k else None for s, k in zip(cat.split(dx.cpu().numpy(), c.widths), want)]
    else:
        dts = [torch.full_like(x, float("nan")) if k else None for x, k in zip(xs, want)]
        px, cs = _table(xs)
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_act_cat_bwd(px, cs, len(xs), dy.data_ptr(), int(dy_bf16), n, g.data_ptr(), b.data_ptr(), sv.data_ptr(),
                                            int(relu), thr, scale, SEED, _table(dts)[0] if any(want) else None, *tail), "bn_act_cat_bwd")
        launches = lib.mccnn_debug_launch_count() - before
        torch.cuda.synchronize()
        dxs = [None if t is None else t.cpu().numpy() for t in dts]
    return dxs, dg.cpu().numpy(), db.cpu().numpy(), launches


def _same_bytes(a, b):
    return all((p is None and q is None) or (p is not None and q is not None and p.tobytes() == q.tobytes()) for p, q in zip(a, b))


@pytest.mark.parametrize("keepProb", [None, 0.7], ids=["nodrop", "drop0.7"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("c", cat.CASES, ids=cat.IDS)
def test_forward(mc, c, relu, keepProb):
    out, _mask, _scale = _reference(c, relu, keepProb)
    y, saved, mm, mv, launches = _raw_fwd(c, relu, keepProb)
    helpers.assert_float_close(saved[0], out["mean"], what="saved mean")
    helpers.assert_float_close(saved[1], out["rstd"], what="saved rstd")
    helpers.assert_float_close(mm, out["mov_mean"], what="moving mean")
    helpers.assert_float_close(mv, out["mov_var"], what="moving variance")
    helpers.assert_float_close(y, out["y"], what="y")
    assert launches == (1 if c.n <= 256 else 2)
    if cat.plans_coincide(c):   # the plan of the contiguous op on the concatenation: its bytes
        p = _raw_fwd(c, relu, keepProb, plain=True)
        assert p[4] == launches
        assert _same_bytes((y, saved, mm, mv), p[:4])


@pytest.mark.parametrize("c", cat.CASES, ids=cat.IDS)
def test_dropped_set_is_exact(mc, c):
    """relu off, gamma = 1, beta = 10: no kept element is zero, so the zeros of y are the complement of the mask over
    (row, GLOBAL column)."""
    n, w = c.n, cat.width(c)
    y = _raw_fwd(c, False, 0.7, gamma=np.ones(w, np.float32), beta=np.full(w, 10.0, np.float32))[0]
    assert np.array_equal(y == 0.0, ~ref.keep_mask(SEED, n, w, ref.threshold(0.7)))


def _gpu_gates(c):
    return _raw_fwd(c, True, None)[0] > 0.0


@pytest.mark.parametrize("relu,keepProb", [(True, 0.7), (True, None), (False, 0.7), (False, None)],
                         ids=["relu-drop", "relu", "linear-drop", "linear"])
@pytest.mark.parametrize("c", cat.CASES, ids=cat.IDS)
def test_backward(mc, c, relu, keepProb):
    """dx_s, dgamma, dbeta against the reference evaluated with the GPU's own gates; no dx wanted: the same sums, byte for
    byte; coinciding plans: the bytes of the contiguous backward, dx_s its column slice."""
    d = cat.data(c)
    out, mask, scale = _reference(c, relu, keepProb)
    saved = _raw_fwd(c, relu, keepProb)[1]
    gates = _gpu_gates(c) if relu else None
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale, gate=gates)
    dxs, dg, db, launches = _raw_bwd(c, saved, relu, keepProb)
    helpers.assert_float_close(dg, rdg, what="dgamma")
    helpers.assert_float_close(db, rdb, what="dbeta")
    helpers.assert_float_close(np.concatenate(dxs, 1), rdx, what="dx")   # (one scale for all segments: dx's own)
    assert launches == (1 if c.n <= 256 else 2)
    none, dg2, db2, launches2 = _raw_bwd(c, saved, relu, keepProb, want=[False] * len(c.widths))
    assert all(t is None for t in none) and _same_bytes((dg2, db2), (dg, db)) and launches2 == launches
    if cat.plans_coincide(c):
        pdxs, pdg, pdb, pl = _raw_bwd(c, saved, relu, keepProb, plain=True)
        assert pl == launches and _same_bytes((dg, db), (pdg, pdb)) and _same_bytes(dxs, pdxs)


@pytest.mark.parametrize("c", cat.CASES, ids=cat.IDS)
def test_eval_forward(mc, c):
    d = cat.data(c)
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], False, True)
    y, _saved, mm, mv, launches = _raw_fwd(c, True, 0.7, training=False)   # (a keep probability is ignored in eval mode)
    helpers.assert_float_close(y, out["y"], what="eval y")
    assert mm.tobytes() == d["mov_mean"].tobytes() and mv.tobytes() == d["mov_var"].tobytes()
    assert launches == 1
    if cat.plans_coincide(c):
        assert _raw_fwd(c, True, 0.7, training=False, plain=True)[0].tobytes() == y.tobytes()


@pytest.mark.parametrize("c", [cat.CASES[2], cat.CASES[3]], ids=[cat.IDS[2], cat.IDS[3]])
def test_bf16_rows_are_the_contiguous_ops_bytes(mc, c):
    """bf16 y and dy on [8, 8] (one launch) and [4, 8, 4] (two): mccnn_bn_act_fwd_rows / _bwd_rows on the concatenation."""
    assert c.widths in ((8, 8), (4, 8, 4)) and cat.plans_coincide(c)
    a = _raw_fwd(c, True, 0.7, y_bf16=True)
    p = _raw_fwd(c, True, 0.7, y_bf16=True, plain=True)
    assert a[0].dtype == np.int16 and _same_bytes(a[:4], p[:4]) and a[4] == p[4]
    f32 = _raw_fwd(c, True, 0.7)
    assert _same_bytes(a[1:4], f32[1:4])                       # the statistics do not know y's type
    dxs, dg, db, launches = _raw_bwd(c, a[1], True, 0.7, dy_bf16=True)
    pdxs, pdg, pdb, pl = _raw_bwd(c, a[1], True, 0.7, dy_bf16=True, plain=True)
    assert _same_bytes(dxs, pdxs) and _same_bytes((dg, db), (pdg, pdb)) and launches == pl


def _through_autograd(op, c, relu, keepProb, want=None, outDtype=None):
    """A Python route forward + backward through torch.autograd -> (bytes of y, dgamma, dbeta, the moving statistics and
    every segment's gradient (None where it has none), y)."""
    import torch
    d = cat.data(c)
    want = [True] * len(c.widths) if want is None else want
    xs = [x.requires_grad_(k) for x, k in zip(_segments(c, d["x"]), want)]
    g, b = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    y = op(xs, g, b, mm, mv, True, relu, keepProb, SEED, outDtype=outDtype)
    y.backward(_dev(d["dy"]).to(y.dtype))
    torch.cuda.synchronize()
    outs = [_np(y.detach()).tobytes()] + [t.cpu().numpy().tobytes() for t in (g.grad, b.grad, mm, mv)]
    return outs + [None if x.grad is None else x.grad.cpu().numpy().tobytes() for x in xs], y


@pytest.mark.parametrize("c", [cat.CASES[2], cat.CASES[5], cat.CASES[6], cat.CASES[10]],
                         ids=[cat.IDS[2], cat.IDS[5], cat.IDS[6], cat.IDS[10]])
def test_reproducible_and_extension_equals_ctypes(mc, c):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    a, y = _through_autograd(M.bn_relu_dropout_cat, c, True, 0.7)
    b, _ = _through_autograd(M.bn_relu_dropout_cat, c, True, 0.7)
    assert a == b                                            # two runs: identical bytes for all outputs
    out, _, _ = _reference(c, True, 0.7)
    helpers.assert_float_close(y.detach().cpu().numpy(), out["y"], what="op y")
    raw = _raw_fwd(c, True, 0.7)
    assert a[0] == raw[0].tobytes() and a[3] == raw[2].tobytes() and a[4] == raw[3].tobytes()   # ... those of the C entry
    assert native._EXT is not None, "the torch extension did not load"
    e, ye = _through_autograd(native.bn_relu_drop_cat, c, True, 0.7)
    assert e == a                                            # the extension entry: the same bytes, forward and backward
    assert type(ye.grad_fn).__name__ != "_BnReluDropoutCatBackward" and type(y.grad_fn).__name__ == "_BnReluDropoutCatBackward"
    # once differentiable
    d = cat.data(c)
    for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
        xs = [x.requires_grad_(True) for x in _segments(c, d["x"])]
        yy = op(xs, _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"]), True)
        (gx,) = torch.autograd.grad(yy.sum(), xs[0], create_graph=True)
        with pytest.raises(RuntimeError):
            gx.sum().backward()


@pytest.mark.parametrize("c", [cat.CASES[3], cat.CASES[6]], ids=[cat.IDS[3], cat.IDS[6]])
def test_segment_without_a_gradient_gets_none(mc, c):
    """Both routes: the segment's gradient is None, every other output keeps its bytes; bf16 y as well."""
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    want = [True, False, True]
    for dt in (None, _ydtype(True) if cat.width(c) % 2 == 0 else None):
        full, _ = _through_autograd(M.bn_relu_dropout_cat, c, True, 0.7, outDtype=dt)
        for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
            part, _ = _through_autograd(op, c, True, 0.7, want=want, outDtype=dt)
            assert part[:5] == full[:5]
            assert part[6] is None and part[5] == full[5] and part[7] == full[7]
            none, _ = _through_autograd(op, c, True, 0.7, want=[False] * 3, outDtype=dt)
            assert none[:5] == full[:5] and none[5:] == [None] * 3


def test_eval_with_gradients_is_refused(mc):
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    c = cat.CASES[2]
    d = cat.data(c)
    for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
        xs = _segments(c, d["x"])
        xs[1].requires_grad_(True)
        with pytest.raises(M.InvalidArgumentError):
            op(xs, _dev(d["gamma"]), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"]), False)


@pytest.mark.parametrize("widths", [(24,), (8, 9, 7), (3,) * 8], ids=["S1", "S3", "S8"])
def test_launch_counts_are_the_contiguous_ops(mc, widths):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    w = sum(widths)
    for n, want in ((200, 1), (256, 1), (257, 2), (5000, 2)):
        for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
            xs = [torch.randn(n, k, device=dev, requires_grad=True) for k in widths]
            g, b = torch.ones(w, device=dev, requires_grad=True), torch.zeros(w, device=dev, requires_grad=True)
            mm, mv = torch.zeros(w, device=dev), torch.ones(w, device=dev)
            before = lib.mccnn_debug_launch_count()
            y = op(xs, g, b, mm, mv, True, True, 0.8, 3)
            fwd = lib.mccnn_debug_launch_count() - before
            y.backward(torch.ones_like(y))
            bwd = lib.mccnn_debug_launch_count() - before - fwd
            with torch.no_grad():
                before = lib.mccnn_debug_launch_count()
                op(xs, g, b, mm, mv, False)
                ev = lib.mccnn_debug_launch_count() - before
            assert (fwd, bwd, ev) == (want, want, 1), (n, widths, fwd, bwd, ev)
    torch.cuda.synchronize()


@pytest.mark.parametrize("widths,coincide", [((8, 4, 12), True), ((6, 10, 4), False), ((3, 5, 2), True)],
                         ids=["by4", "C%4==0", "C%4!=0"])
def test_helper_on_a_list(mc, widths, coincide):
    """batch_norm_RELU_drop_out("L", [a, b, c], ...) with fused_ and fusedCat_ on: launches (1 | 2, 1 | 2, 1), the state_dict
    keys and dropCalls_ of the fusedCat_-off path, values within the f32 bar of it and, where the plans coincide, its bytes
    (the off path is torch.cat + the contiguous op + slices of its gradient)."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    for n, want in ((200, 1), (5000, 2)):
        torch.manual_seed(n)
        parts = [torch.randn(n, k, device=dev) * 3 + 5 for k in widths]
        gy = torch.randn(n, sum(widths), device=dev)
        res = {}
        for fusedCat in (False, True):
            st = U.VariableStore(dev, fused=True, fusedCat=fusedCat)
            st.dropSeed_ = 11
            xs = [p.clone().requires_grad_(True) for p in parts]
            U.batch_norm_RELU_drop_out("L", xs, True, True, 0.8, st)            # creates the variables
            before = lib.mccnn_debug_launch_count()
            y = U.batch_norm_RELU_drop_out("L", xs, True, True, 0.8, st)
            fwd = lib.mccnn_debug_launch_count() - before
            y.backward(gy)
            bwd = lib.mccnn_debug_launch_count() - before - fwd
            with torch.no_grad():
                before = lib.mccnn_debug_launch_count()
                ye = U.batch_norm_RELU_drop_out("L", xs, False, True, 0.8, st)
                ev = lib.mccnn_debug_launch_count() - before
            assert (fwd, bwd, ev) == (want, want, 1), (n, fusedCat, fwd, bwd, ev)
            assert st.dropCalls_ == 2
            assert ("Cat" in y.grad_fn.name()) == fusedCat               # (BnCatBackward, or the contiguous op's node)
            res[fusedCat] = ([y.detach(), ye] + [x.grad for x in xs] + [st.variables_["L_BN/gamma"].grad, st.variables_["L_BN/beta"].grad],
                             st.state_dict())
        torch.cuda.synchronize()
        (on, sd_on), (off, sd_off) = res[True], res[False]
        assert list(sd_on.keys()) == list(sd_off.keys()) == ["L_BN/gamma", "L_BN/beta", "L_BN/moving_mean", "L_BN/moving_variance"]
        # one scale for the segments' gradients: dx's own
        on_v = on[:2] + [torch.cat(on[2:2 + len(widths)], 1)] + on[2 + len(widths):] + [sd_on[k] for k in sd_on]
        off_v = off[:2] + [torch.cat(off[2:2 + len(widths)], 1)] + off[2 + len(widths):] + [sd_off[k] for k in sd_off]
        for a, b in zip(on_v, off_v):
            helpers.assert_float_close(a.cpu().numpy(), b.cpu().numpy(), what="helper output")
        if coincide:
            for a, b in zip(on + [sd_on[k] for k in sd_on], off + [sd_off[k] for k in sd_off]):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # the switch is reassignable, and a single tensor takes today's path whatever it says
    st = U.VariableStore(dev, fused=True, fusedCat=True)
    x = torch.cat(parts, 1).requires_grad_(True)
    y = U.batch_norm_RELU_drop_out("L", x, True, False, None, st)
    assert "Cat" not in y.grad_fn.name()
    st.fusedCat_ = False
    y = U.batch_norm_RELU_drop_out("L", [p.clone().requires_grad_(True) for p in parts], True, False, None, st)
    assert "Cat" not in y.grad_fn.name()
