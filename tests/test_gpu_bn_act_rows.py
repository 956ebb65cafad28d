"""The fused dense glue on bf16 rows on the GPU (mccnn_bn_act_fwd_rows / _bwd_rows, bn_relu_dropout(outDtype=...),
native.bn_relu_drop, batch_norm_RELU_drop_out(outDtype=...), MCClassS(rows=torch.bfloat16)): x and y each float32 or
bfloat16, against the float64 reference of tests/bn_act_rows_ref.py evaluated on the rounded operands.

Bars: an f32 output is held to helpers.assert_float_close (1e-4, norm-wise and per element) as in the f32 op; a bf16 output
v with reference r to |v - r| <= 2^-8 |r| + 1e-4 max|r| (rows.assert_bf16_close). The sharpest tests are exact: E1 (f32
x: statistics are the f32 entry's bytes, a bf16 y is the rounding of its y, a bf16 dy gives its gradients) and E2 (bf16 x:
the output type changes the store only)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import bn_act_ref as ref  # noqa: E402
import bn_act_rows_ref as rows  # noqa: E402
import helpers  # noqa: E402

IDS = ["%dx%d" % s for s in rows.SHAPES]
SEED = 77
combos = pytest.mark.parametrize("combo", rows.COMBOS, ids=rows.COMBO_IDS)
shapes = pytest.mark.parametrize("shape", rows.SHAPES, ids=IDS)


def _dev(a, bf16=False):
    """A device copy of a NumPy array; bf16: as bfloat16 (exact for the rounded operands of rows.case)."""
    import torch
    t = torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))
    return t.to(torch.bfloat16) if bf16 else t


def _np(t):
    """A device tensor -> float32 NumPy (bf16 widened exactly)."""
    return t.detach().float().cpu().numpy()


def _bits(t):
    """The bytes of a device tensor."""
    import torch
    t = t.detach().contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()


def _check(got, want, bf16, what):
    if bf16:
        rows.assert_bf16_close(got, want, what)
    else:
        helpers.assert_float_close(got, want, what=what)


def _raw_fwd(d, xb, yb, relu, keepProb, training=True, gamma=None, beta=None, x=None, y=None):
    """mccnn_bn_act_fwd_rows -> dict(y, saved, mm, mv: device tensors; launches). x, y: tensors to use in place of fresh ones."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    x = _dev(d["x"], xb) if x is None else x
    g, b = _dev(d["gamma"] if gamma is None else gamma), _dev(d["beta"] if beta is None else beta)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    n, c = x.shape
    thr, scale = _bn_act_args(x, g, b, mm, mv, keepProb, SEED)
    if y is None:
        y = torch.empty((n, c), dtype=torch.bfloat16 if yb else torch.float32, device=x.device)
    saved = torch.full((2, c), float("nan"), device=x.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_bn_act_fwd_rows(x.data_ptr(), int(xb), n, c, g.data_ptr(), b.data_ptr(), mm.data_ptr(), mv.data_ptr(),
                                         0.99, 1e-3, int(training), int(relu), thr, scale, SEED, y.data_ptr(), int(yb),
                                         saved.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle()), "bn_act_fwd_rows")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dict(y=y, saved=saved, mm=mm, mv=mv, launches=launches)


def _raw_bwd(d, xb, yb, saved, relu, keepProb, want_dx=True, x=None, dy=None):
    """mccnn_bn_act_bwd_rows -> (dx or None, dgamma, dbeta: device tensors; launches)."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    x = _dev(d["x"], xb) if x is None else x
    dy = _dev(d["dy"], yb) if dy is None else dy
    g, b = _dev(d["gamma"]), _dev(d["beta"])
    n, c = x.shape
    thr, scale = _bn_act_args(x, g, b, g, g, keepProb, SEED)
    dx = torch.empty_like(x) if want_dx else None
    dg, db = torch.empty(c, device=x.device), torch.empty(c, device=x.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_bn_act_bwd_rows(x.data_ptr(), int(xb), dy.data_ptr(), int(yb), n, c, g.data_ptr(), b.data_ptr(),
                                         saved.data_ptr(), int(relu), thr, scale, SEED, None if dx is None else dx.data_ptr(),
                                         dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle()),
               "bn_act_bwd_rows")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dx, dg, db, launches


def _old_fwd(d, relu, keepProb):
    """The float32 entry mccnn_bn_act_fwd: the yardstick of E1."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    x, g, b, mm, mv = _dev(d["x"]), _dev(d["gamma"]), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"])
    n, c = x.shape
    thr, scale = _bn_act_args(x, g, b, mm, mv, keepProb, SEED)
    y, saved = torch.empty_like(x), torch.empty((2, c), device=x.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    _lib.check(lib.mccnn_bn_act_fwd(x.data_ptr(), n, c, g.data_ptr(), b.data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.99, 1e-3, 1,
                                    int(relu), thr, scale, SEED, y.data_ptr(), saved.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_handle()), "bn_act_fwd")
    torch.cuda.synchronize()
    return dict(y=y, saved=saved, mm=mm, mv=mv)


def _old_bwd(d, saved, relu, keepProb, want_dx=True):
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    x, dy, g, b = _dev(d["x"]), _dev(d["dy"]), _dev(d["gamma"]), _dev(d["beta"])
    n, c = x.shape
    thr, scale = _bn_act_args(x, g, b, g, g, keepProb, SEED)
    dx = torch.empty_like(x) if want_dx else None
    dg, db = torch.empty(c, device=x.device), torch.empty(c, device=x.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    _lib.check(lib.mccnn_bn_act_bwd(x.data_ptr(), dy.data_ptr(), n, c, g.data_ptr(), b.data_ptr(), saved.data_ptr(), int(relu), thr,
                                    scale, SEED, None if dx is None else dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _lib.stream_handle()), "bn_act_bwd")
    torch.cuda.synchronize()
    return dx, dg, db


def _check_stats(o, out):
    helpers.assert_float_close(_np(o["saved"])[0], out["mean"], what="saved mean")
    helpers.assert_float_close(_np(o["saved"])[1], out["rstd"], what="saved rstd")
    helpers.assert_float_close(_np(o["mm"]), out["mov_mean"], what="moving mean")
    helpers.assert_float_close(_np(o["mv"]), out["mov_var"], what="moving variance")


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("keepProb", [None, 0.7], ids=["nodrop", "drop0.7"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@combos
@shapes
def test_forward(mc, shape, combo, relu, keepProb):
    xb, yb = combo
    d = rows.case(*shape, xb, yb)
    out, _mask, _scale = rows.reference(shape, xb, relu, keepProb, SEED)
    o = _raw_fwd(d, xb, yb, relu, keepProb)
    _check_stats(o, out)
    _check(_np(o["y"]), out["y"], yb, "y")
    assert o["launches"] == (1 if shape[0] <= 256 else 2)


# ------------------------------------------------------------------------------------------------- E1, E2: byte for byte
@pytest.mark.parametrize("relu,keepProb", [(True, 0.7), (False, None)], ids=["relu-drop", "linear"])
@pytest.mark.parametrize("shape", rows.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_e1_f32_rows_are_the_f32_entry(mc, shape, relu, keepProb):
    """f32 x. Whatever y's type: saved and the moving statistics are the bytes of mccnn_bn_act_fwd, a bf16 y is the RNE
    rounding of its y; with a bf16 dy, dx / dgamma / dbeta are the bytes of mccnn_bn_act_bwd on the widened dy."""
    d = rows.case(*shape, False, True)                 # (dy rounded to bf16: the f32 entry reads it widened)
    old = _old_fwd(d, relu, keepProb)
    for yb in (False, True):
        o = _raw_fwd(d, False, yb, relu, keepProb)
        for k in ("saved", "mm", "mv"):
            assert _bits(o[k]) == _bits(old[k]), (k, yb)
        if yb:
            assert rows.to_bf16_bits(_np(old["y"])).tobytes() == _bits(o["y"])
        else:
            assert _bits(o["y"]) == _bits(old["y"])
    for want_dx in (True, False):
        odx, odg, odb = _old_bwd(d, old["saved"], relu, keepProb, want_dx)
        for yb in (False, True):
            dx, dg, db, _ = _raw_bwd(d, False, yb, old["saved"], relu, keepProb, want_dx)
            assert _bits(dg) == _bits(odg) and _bits(db) == _bits(odb), (yb, want_dx)
            assert (dx is None and odx is None) or _bits(dx) == _bits(odx), (yb, want_dx)


@pytest.mark.parametrize("relu,keepProb", [(True, 0.7), (False, None)], ids=["relu-drop", "linear"])
@pytest.mark.parametrize("shape", rows.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_e2_bf16_rows_the_output_type_changes_the_store_only(mc, shape, relu, keepProb):
    d = rows.case(*shape, True, False)
    a, b = _raw_fwd(d, True, False, relu, keepProb), _raw_fwd(d, True, True, relu, keepProb)
    for k in ("saved", "mm", "mv"):
        assert _bits(a[k]) == _bits(b[k]), k
    assert rows.to_bf16_bits(_np(a["y"])).tobytes() == _bits(b["y"])


# ------------------------------------------------------------------------------------------------- mask, gates
@pytest.mark.parametrize("xb", [False, True], ids=["f32", "bf16"])
@shapes
def test_dropped_set_is_exact_with_a_bf16_output(mc, shape, xb):
    """relu off, gamma = 1, beta = 10: no kept element is zero (nor rounds to it), so the zeros of y are the mask's complement."""
    n, c = shape
    d = rows.case(n, c, xb, True)
    y = _np(_raw_fwd(d, xb, True, False, 0.7, gamma=np.ones(c, np.float32), beta=np.full(c, 10.0, np.float32))["y"])
    assert np.array_equal(y == 0.0, ~ref.keep_mask(SEED, n, c, ref.threshold(0.7)))


_GATES = {}


def _gpu_gates(shape, xb, yb):
    """The op's own gates, read off a forward without dropout (a positive pre does not round to zero in bf16)."""
    key = (shape, xb, yb)
    if key not in _GATES:
        _GATES[key] = _np(_raw_fwd(rows.case(*shape, xb, yb), xb, yb, True, None)["y"]) > 0.0
    return _GATES[key]


@combos
@shapes
def test_relu_gates(mc, shape, combo):
    xb, yb = combo
    out, _, _ = rows.reference(shape, xb, True, None, SEED)
    gates = _gpu_gates(shape, xb, yb)
    pre = out["pre"]
    band = np.abs(pre) <= 1e-5 * np.abs(pre).max()
    diff = gates != (pre > 0.0)
    assert not (diff & ~band).any()
    assert diff.sum() <= 1e-3 * pre.size


# ------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("relu,keepProb", [(True, 0.7), (True, None), (False, 0.7)], ids=["relu-drop", "relu", "linear-drop"])
@combos
@shapes
def test_backward(mc, shape, combo, relu, keepProb):
    """dx, dgamma, dbeta against the reference evaluated with the GPU's own gates; dx not wanted: the same sums, byte for byte."""
    xb, yb = combo
    d = rows.case(*shape, xb, yb)
    out, mask, scale = rows.reference(shape, xb, relu, keepProb, SEED)
    saved = _raw_fwd(d, xb, yb, relu, keepProb)["saved"]
    gates = _gpu_gates(shape, xb, yb) if relu else None
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale, gate=gates)
    dx, dg, db, launches = _raw_bwd(d, xb, yb, saved, relu, keepProb)
    helpers.assert_float_close(_np(dg), rdg, what="dgamma")
    helpers.assert_float_close(_np(db), rdb, what="dbeta")
    assert dx.dtype == _dev(d["x"][:1], xb).dtype
    _check(_np(dx), rdx, xb, "dx")
    assert launches == (1 if shape[0] <= 256 else 2)
    _, dg2, db2, launches2 = _raw_bwd(d, xb, yb, saved, relu, keepProb, want_dx=False)
    assert _bits(dg2) == _bits(dg) and _bits(db2) == _bits(db)
    assert launches2 <= launches


# ------------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@combos
@shapes
def test_eval_forward(mc, shape, combo, relu):
    xb, yb = combo
    d = rows.case(*shape, xb, yb)
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], False, relu)
    o = _raw_fwd(d, xb, yb, relu, 0.7, training=False)   # (a keep probability is ignored in eval mode)
    _check(_np(o["y"]), out["y"], yb, "eval y")
    assert _np(o["mm"]).tobytes() == d["mov_mean"].tobytes() and _np(o["mv"]).tobytes() == d["mov_var"].tobytes()
    assert o["launches"] == 1


# ------------------------------------------------------------------------------------------------- the op entries
def _through_autograd(op, d, xb, yb, relu, keepProb, want_dx=True, x=None, dy=None, name_type=True):
    """An op entry forward + backward through torch.autograd -> (bytes of y, dx, dgamma, dbeta, moving statistics; y; x)."""
    import torch
    x = (_dev(d["x"], xb) if x is None else x).requires_grad_(want_dx)
    g, b = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    kw = {"outDtype": torch.bfloat16 if yb else torch.float32} if name_type else {}
    y = op(x, g, b, mm, mv, True, relu, keepProb, SEED, **kw)
    y.backward(_dev(d["dy"], yb) if dy is None else dy)
    torch.cuda.synchronize()
    outs = [y, x.grad if want_dx else torch.zeros(1), g.grad, b.grad, mm, mv]
    return [_bits(t) for t in outs], y, x, g


@combos
@pytest.mark.parametrize("shape", [(65, 16), (257, 64), (1000, 130), (4099, 34)], ids=lambda s: "%dx%d" % s)
def test_reproducible_and_extension_equals_ctypes(mc, shape, combo):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    xb, yb = combo
    d = rows.case(*shape, xb, yb)
    a, y, x, g = _through_autograd(M.bn_relu_dropout, d, xb, yb, True, 0.7)
    b, _, _, _ = _through_autograd(M.bn_relu_dropout, d, xb, yb, True, 0.7)
    assert a == b                                            # two runs: identical bytes for all outputs
    assert y.dtype == (torch.bfloat16 if yb else torch.float32)
    assert x.grad.dtype == x.dtype and g.grad.dtype == torch.float32
    out, _, _ = rows.reference(shape, xb, True, 0.7, SEED)
    _check(_np(y), out["y"], yb, "op y")
    assert native._EXT is not None, "the torch extension did not load"
    e, ye, xe, ge = _through_autograd(native.bn_relu_drop, d, xb, yb, True, 0.7)
    assert e == a                                            # the extension entry: the same bytes, forward and backward
    assert type(ye.grad_fn).__name__ != "_BnReluDropoutBackward"   # ... through its own C++ node
    assert xe.grad.dtype == xe.dtype and ge.grad.dtype == torch.float32
    e2, _, _, _ = _through_autograd(native.bn_relu_drop, d, xb, yb, True, 0.7, want_dx=False)
    assert e2[2:4] == a[2:4]
    if xb == yb:                                             # no type named: y has x's type, the same bytes
        for op in (M.bn_relu_dropout, native.bn_relu_drop):
            assert _through_autograd(op, d, xb, yb, True, 0.7, name_type=False)[0] == a
    # a gradient of another type than y's is cast, a non-contiguous one made contiguous
    other = _dev(d["dy"], yb).to(torch.float32 if yb else torch.bfloat16)
    if yb:      # (bf16 dy widened and handed over as f32: the cast back is exact)
        for op in (M.bn_relu_dropout, native.bn_relu_drop):
            assert _through_autograd(op, d, xb, yb, True, 0.7, dy=other)[0] == a
    strided = _dev(d["dy"], yb).t().contiguous().t()
    assert not strided.is_contiguous()
    assert _through_autograd(M.bn_relu_dropout, d, xb, yb, True, 0.7, dy=strided)[0] == a
    # once differentiable
    x = _dev(d["x"], xb).requires_grad_(True)
    gm, bt = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    for op in (M.bn_relu_dropout, native.bn_relu_drop):
        yy = op(x, gm, bt, _dev(d["mov_mean"]), _dev(d["mov_var"]), True, outDtype=torch.bfloat16 if yb else torch.float32)
        (gx,) = torch.autograd.grad(yy.float().sum(), x, create_graph=True)
        with pytest.raises(RuntimeError):
            gx.float().sum().backward()


def test_eval_with_gradients_is_refused(mc):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    d = rows.case(65, 16, True, True)
    for op in (M.bn_relu_dropout, native.bn_relu_drop):
        with pytest.raises(M.InvalidArgumentError):
            op(_dev(d["x"], True).requires_grad_(True), _dev(d["gamma"]), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"]),
               False, outDtype=torch.float32)


# ------------------------------------------------------------------------------------------------- alignment
def _off(a, elems):
    """A contiguous bf16 [n, c] view that starts `elems` elements behind an aligned allocation."""
    import torch
    n, c = a.shape
    buf = torch.empty(n * c + elems, dtype=torch.bfloat16, device=torch.device("cuda", 0))
    v = buf[elems:].view(n, c)
    v.copy_(_dev(a, True))
    assert v.is_contiguous() and v.data_ptr() % 16 == (2 * elems) % 16
    return v


@pytest.mark.parametrize("shape", [(65, 16), (257, 64)], ids=lambda s: "%dx%d" % s)
def test_rows_two_bytes_off_a_word_are_copied_by_the_op_and_refused_by_the_abi(mc, shape):
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    d = rows.case(*shape, True, True)
    for op in (M.bn_relu_dropout, native.bn_relu_drop):
        want = _through_autograd(op, d, True, True, True, 0.7)[0]
        x, dy = _off(d["x"], 1), _off(d["dy"], 1)
        assert x.data_ptr() % 4 == 2 and dy.data_ptr() % 4 == 2
        assert _through_autograd(op, d, True, True, True, 0.7, x=x, dy=dy)[0] == want
    # the same views handed to the C ABI: MCCNN_E_SHAPE, nothing launched
    x, dy = _off(d["x"], 1), _off(d["dy"], 1)
    good = _raw_fwd(d, True, True, True, 0.7)
    before = lib.mccnn_debug_launch_count()
    with pytest.raises(_lib.MCCNNError, match="code -5"):
        _raw_fwd(d, True, True, True, 0.7, x=x)
    with pytest.raises(_lib.MCCNNError, match="code -5"):
        _raw_fwd(d, True, True, True, 0.7, y=_off(d["x"], 1))
    with pytest.raises(_lib.MCCNNError, match="code -5"):
        _raw_bwd(d, True, True, good["saved"], True, 0.7, x=x)
    with pytest.raises(_lib.MCCNNError, match="code -5"):
        _raw_bwd(d, True, True, good["saved"], True, 0.7, dy=dy)
    assert lib.mccnn_debug_launch_count() == before


@pytest.mark.parametrize("shape", [(65, 16), (257, 64), (4099, 32)], ids=lambda s: "%dx%d" % s)
def test_rows_off_the_16_byte_grid_take_the_pair_form(mc, shape):
    """c % 8 == 0 but x, y, dy four bytes off a 16-byte boundary, through the C ABI (the ops would copy them): no 16-byte
    access, forward and backward, small form and slabs; same bars."""
    import torch
    n, c = shape
    d = rows.case(n, c, True, True)
    x, dy = _off(d["x"], 2), _off(d["dy"], 2)
    ybuf = torch.zeros(n * c + 2 + 8, dtype=torch.bfloat16, device=x.device)
    y = ybuf[2:2 + n * c].view(n, c)
    assert x.data_ptr() % 16 == 4 and y.data_ptr() % 16 == 4
    out, mask, scale = rows.reference(shape, True, True, 0.7, SEED)
    o = _raw_fwd(d, True, True, True, 0.7, x=x, y=y)
    _check_stats(o, out)
    rows.assert_bf16_close(_np(y), out["y"], "y")
    assert float(ybuf[:2].float().abs().sum()) == 0.0 and float(ybuf[2 + n * c:].float().abs().sum()) == 0.0   # nothing beside y
    assert o["launches"] == (1 if n <= 256 else 2)
    gates = np.where(mask, _np(y) > 0.0, out["pre"] > 0.0)   # the op's own gates where the mask kept an element
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], True, mask, scale, gate=gates)
    dx, dg, db, launches = _raw_bwd(d, True, True, o["saved"], True, 0.7, x=x, dy=dy)
    rows.assert_bf16_close(_np(dx), rdx, "dx")
    helpers.assert_float_close(_np(dg), rdg, what="dgamma")
    helpers.assert_float_close(_np(db), rdb, what="dbeta")
    assert launches == (1 if n <= 256 else 2)


# ------------------------------------------------------------------------------------------------- helpers
@pytest.mark.parametrize("outDtype", [None, "float32", "bfloat16"])
def test_launch_counts_of_the_glue_on_bf16_rows(mc, outDtype):
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    kw = {} if outDtype is None else {"outDtype": getattr(torch, outDtype)}
    want_type = torch.bfloat16 if outDtype is None else getattr(torch, outDtype)
    for n, want in ((200, 1), (256, 1), (257, 2), (5000, 2)):
        x = torch.randn(n, 24, device=dev).to(torch.bfloat16).requires_grad_(True)
        st = U.VariableStore(dev, fused=True)
        U.batch_norm_RELU_drop_out("L", x, True, True, 0.8, st, **kw)            # creates the variables
        before = lib.mccnn_debug_launch_count()
        y = U.batch_norm_RELU_drop_out("L", x, True, True, 0.8, st, **kw)
        fwd = lib.mccnn_debug_launch_count() - before
        assert y.dtype == want_type
        y.float().sum().backward()
        bwd = lib.mccnn_debug_launch_count() - before - fwd
        with torch.no_grad():
            before = lib.mccnn_debug_launch_count()
            ye = U.batch_norm_RELU_drop_out("L", x, False, True, 0.8, st, **kw)
            ev = lib.mccnn_debug_launch_count() - before
        assert ye.dtype == want_type
        assert (fwd, bwd, ev) == (want, want, 1), (n, fwd, bwd, ev)
        assert st.dropCalls_ == 2                                                # as for f32 rows
        assert st.variables_["L_BN/gamma"].grad.dtype == torch.float32 and x.grad.dtype == torch.bfloat16
    # an odd c: the fused form does not apply, the torch code runs and no library launch is made
    x = torch.randn(300, 5, device=dev).to(torch.bfloat16)
    st = U.VariableStore(dev, fused=True)
    before = lib.mccnn_debug_launch_count()
    with torch.no_grad():
        y = U.batch_norm_RELU_drop_out("O", x, False, False, None, st, **kw)
    assert lib.mccnn_debug_launch_count() == before and st.dropCalls_ == 0
    assert outDtype is None or y.dtype == want_type
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- network
def test_mcclass_s_with_bf16_rows_matches_the_f32_glue_with_casts(mc):
    """MCClassS(fused=True, rows=torch.bfloat16) against the same graph built from the f32 fused glue with explicit
    .to(torch.bfloat16) / .float() around Conv_2 and Conv_3 (the ops of before this feature), on the cfg1 batch of
    test_mcclass_s_fused_matches_the_cpu_twin with its bars: the two formulations do the same arithmetic, the tolerance
    covers the convolutions' own run-to-run freedom and the summation order of the statistics."""
    import math
    import torch
    from mcclass_s import MCClassS
    from mccnn_amd.MCNetworkUtils import MLP_2_hidden, batch_norm_RELU_drop_out, conv_1x1
    from mccnn_amd.workloads import modelnet_like

    class Casts(MCClassS):
        def forward(self, points, batchIds, features, isTraining, useDropOutFull=True):
            numInputFeatures, batchSize, k, numOutCat = self.args
            st, cb = self.store, self.convBuilder
            cb.reset()
            ph = self.hierarchy(points, batchIds, features)
            bn = lambda name, f: batch_norm_RELU_drop_out(name, f, isTraining, False, 1.0, st)   # noqa: E731
            f1 = cb.create_convolution(convName="Conv_1", inPointHierarchy=ph, inPointLevel=0, outPointLevel=1, inFeatures=features,
                                       inNumFeatures=numInputFeatures, outNumFeatures=k, convRadius=0.2, multiFeatureConv=True)
            f1 = bn("Reduce_1_Out_BN", conv_1x1("Reduce_1", bn("Reduce_1_In_BN", f1), k, k * 2, st)).to(torch.bfloat16)
            f2 = cb.create_convolution(convName="Conv_2", inPointHierarchy=ph, inPointLevel=1, outPointLevel=2, inFeatures=f1,
                                       inNumFeatures=k * 2, convRadius=0.8)
            assert f2.dtype == torch.bfloat16
            f2 = bn("Reduce_2_Out_BN", conv_1x1("Reduce_2", bn("Reduce_2_In_BN", f2.float()), k * 2, k * 4, st)).to(torch.bfloat16)
            f3 = cb.create_convolution(convName="Conv_3", inPointHierarchy=ph, inPointLevel=2, outPointLevel=3, inFeatures=f2,
                                       inNumFeatures=k * 4, convRadius=math.sqrt(3.0) + 0.1)
            fin = bn("BNRELUDROP_final", f3.float())
            return MLP_2_hidden(fin, k * 4, k * 2, k, numOutCat, "Final_Logits", 0.5, isTraining, useDropOutFull, store=st)

    B, n, k, ncat = 32, 1024, 16, 40
    pts, bids = modelnet_like(n, B, 51)
    y = np.random.default_rng(2).integers(0, ncat, B)
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    net = MCClassS(1, B, k, ncat, dev, fused=True, rows=torch.bfloat16)
    twin = Casts(1, B, k, ncat, dev, fused=True)
    P, Bi = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev)
    F = torch.ones((len(pts), 1), device=dev)
    Y = torch.from_numpy(y).to(dev)
    with torch.no_grad():
        net(P, Bi, F, False, useDropOutFull=False)               # creates the variables (eval: the statistics stay put)
        twin(P, Bi, F, False, useDropOutFull=False)
    sd = {k_: v.detach().clone() for k_, v in net.state_dict().items()}
    assert list(twin.state_dict().keys()) == list(sd.keys())     # the same state dict
    twin.load_state_dict(sd)
    res = {}
    for tag, m in (("rows", net), ("casts", twin)):
        for p in m.parameters():
            p.grad = None
        if tag == "rows":
            logits = m(P, Bi, F, True, useConvDropOut=False, useDropOutFull=False)
        else:
            logits = m(P, Bi, F, True, useDropOutFull=False)
        assert logits.dtype == torch.float32
        loss = torch.nn.functional.cross_entropy(logits, Y)
        loss.backward()
        named = dict(m.convBuilder.named_parameters())
        named.update(dict(m.store.named_parameters()))
        res[tag] = (logits.detach().cpu().numpy(), float(loss.detach()), {k_: v.grad.detach().cpu().numpy() for k_, v in named.items()},
                    {k_: v.detach().cpu().numpy() for k_, v in m.state_dict().items()})
        assert all(v.grad.dtype == torch.float32 for v in named.values())
    (gl, gloss, gg, gsd), (cl, closs, cg, csd) = res["rows"], res["casts"]
    assert net.store.dropCalls_ == 0                             # no block dropped
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))  # noqa: E731
    gmax = max(float(np.abs(v).max()) for v in cg.values())
    err = {k_: float(np.abs(gg[k_] - cg[k_]).max() / max(np.abs(cg[k_]).max(), 1e-3 * gmax)) for k_ in cg}
    worst = max(err, key=err.get)
    print("cfg1 end to end, bf16 rows: logits %.1e loss %.1e worst gradient %.1e (%s) over %d tensors" % (
        rel(gl, cl), abs(gloss - closs), err[worst], worst, len(cg)))
    assert rel(gl, cl) <= 1e-4 and abs(gloss - closs) <= 1e-5 * abs(closs)
    assert set(gg) == set(cg)
    for k_ in cg:
        assert err[k_] <= 1e-4, (k_, err[k_])
    assert set(gsd) == set(csd)
    moving = [k_ for k_ in csd if k_.endswith("/moving_mean") or k_.endswith("/moving_variance")]
    assert len(moving) == 16                                     # eight batch-norm blocks
    smax = max(float(np.abs(csd[k_]).max()) for k_ in moving)
    for k_ in moving:
        assert np.abs(gsd[k_] - csd[k_]).max() <= 1e-4 * max(np.abs(csd[k_]).max(), 1e-3 * smax), k_
