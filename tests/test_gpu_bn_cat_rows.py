"""The dense glue over a concatenation of typed segments on the GPU (mccnn_bn_act_cat_fwd_rows / _bwd_rows,
dense_glue.bn_relu_dropout_cat, native.bn_relu_drop_cat, VariableStore(fused=True, fusedCat=True) and MCSeg(rows=bfloat16))
on the cases of tests/bn_cat_rows_ref.py.

The yardstick of the bytes is the existing float32 entry (mccnn_bn_act_cat_fwd / _bwd) on the segments widened to float32 in
fresh allocations: wherever the two take the same number of columns per thread (bn_cat_rows_ref.same_plan) y, saved, both
moving statistics, dgamma, dbeta and the dx_s of every f32 segment are its bytes, and the dx_s of a bf16 segment is its f32
dx_s rounded to nearest even. Every case is also held against the float64 reference of the whole [n, C] array with the bars
of tests/test_gpu_bn_cat.py -- helpers.assert_float_close for an f32 output, bn_act_rows_ref.assert_bf16_close for a bf16 one
(2^-8 |r| + 1e-4 max |r|: the bar of tests/test_gpu_bn_act_rows.py) -- and the GPU's-own-gates design of that file."""
import ctypes as C
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
import bn_cat_ref as cat  # noqa: E402
import bn_cat_rows_ref as rc  # noqa: E402
import helpers  # noqa: E402

SEED = 77


def _torch_dtype(bf16):
    import torch
    return torch.bfloat16 if bf16 else torch.float32


def _dev(a, bf16=False):
    """A device copy of a NumPy array (the cases are read-only); bf16: as bfloat16, exact for operands rounded to it."""
    import torch
    t = torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))
    return t.to(torch.bfloat16) if bf16 else t


def _view_at(t, elems):
    """A contiguous copy of t that starts `elems` elements behind a fresh allocation."""
    import torch
    buf = torch.empty(t.numel() + elems + 8, dtype=t.dtype, device=t.device)
    v = buf[elems:elems + t.numel()].view(*t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (elems * t.element_size()) % 16
    return v


def _segments(c, x, widen=False):
    """The column blocks of the case's x as device tensors, each contiguous: in the segment's type and at the segment's
    offset, or (widen) every one float32 in a fresh allocation -- w(x_s) of the definition."""
    out = []
    for k, (s, t) in enumerate(zip(cat.split(x, c.widths), c.types)):
        if widen:
            out.append(_dev(s))
            assert out[-1].data_ptr() % 16 == 0
        else:
            out.append(_view_at(_dev(s, t), rc.offset(c, k)))
    return out


def _table(ts):
    import torch
    return ((C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts]),
            (C.c_int * len(ts))(*[int(t is not None and t.dtype == torch.bfloat16) for t in ts]),
            (C.c_int * len(ts))(*[0 if t is None else t.shape[1] for t in ts]))


def _thr(keepProb):
    return ref.threshold(keepProb), 1.0 if keepProb is None else float(np.float32(1.0) / np.float32(keepProb))


def _bits(t):
    """A tensor's bytes as a host int tensor (None stays None)."""
    import torch
    if t is None:
        return None
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)).cpu()


def _f32(t):
    return t.float().cpu().numpy()


def _raw_fwd(c, relu, keepProb, training=True, y_bf16=False, widen=False, gamma=None, beta=None):
    """The C-ABI forward: mccnn_bn_act_cat_fwd_rows over the typed segments, or (widen) the existing mccnn_bn_act_cat_fwd over
    their widened copies -> (y, saved, moving_mean, moving_var) as device tensors, and the launches."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    d = rc.data(c)
    xs = _segments(c, d["x"], widen)
    g, b = _dev(d["gamma"] if gamma is None else gamma), _dev(d["beta"] if beta is None else beta)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    n, w = c.n, rc.width(c)
    thr, scale = _thr(keepProb)
    y = torch.empty((n, w), dtype=_torch_dtype(y_bf16), device=g.device)
    saved = torch.full((2, w), float("nan"), device=g.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, w), g.device)
    tail = (g.data_ptr(), b.data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.99, 1e-3, int(training), int(relu), thr, scale, SEED,
            y.data_ptr(), int(y_bf16), saved.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    px, bf, cs = _table(xs)
    before = lib.mccnn_debug_launch_count()
    if widen:
        _lib.check(lib.mccnn_bn_act_cat_fwd(px, cs, len(xs), n, *tail), "bn_act_cat_fwd")
    else:
        _lib.check(lib.mccnn_bn_act_cat_fwd_rows(px, bf, cs, len(xs), n, *tail), "bn_act_cat_fwd_rows")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return (y, saved, mm, mv), launches


def _raw_bwd(c, saved, relu, keepProb, want=None, dy_bf16=False, widen=False):
    """The C-ABI backward -> (dxs, dgamma, dbeta, launches). want: per segment whether dx_s is asked for (None: all; all
    False: dxs == NULL). widen: the existing mccnn_bn_act_cat_bwd over the widened copies."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    d = rc.data(c, dy_bf16)
    xs = _segments(c, d["x"], widen)
    dy = _dev(d["dy"], dy_bf16)
    g, b = _dev(d["gamma"]), _dev(d["beta"])
    n, w = c.n, rc.width(c)
    thr, scale = _thr(keepProb)
    want = [True] * len(xs) if want is None else list(want)
    dg, db = torch.empty(w, device=g.device), torch.empty(w, device=g.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, w), g.device)
    # dx_s sits where x_s sits relative to its allocation, in x_s's type
    dts = [_view_at(torch.full_like(x, float("nan")), 0 if widen else rc.offset(c, k)) if k_ else None
           for k, (x, k_) in enumerate(zip(xs, want))]
    px, bf, cs = _table(xs)
    pdx = _table(dts)[0] if any(want) else None
    head = (dy.data_ptr(), int(dy_bf16), n, g.data_ptr(), b.data_ptr(), saved.data_ptr(), int(relu), thr, scale, SEED, pdx,
            dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    before = lib.mccnn_debug_launch_count()
    if widen:
        _lib.check(lib.mccnn_bn_act_cat_bwd(px, cs, len(xs), *head), "bn_act_cat_bwd")
    else:
        _lib.check(lib.mccnn_bn_act_cat_bwd_rows(px, bf, cs, len(xs), *head), "bn_act_cat_bwd_rows")
    launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return dts, dg, db, launches


def _equal(a, b):
    import torch
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)))


def _check_out(got, want, what):
    """An output against its float64 reference: the bar of its storage type."""
    import torch
    if got.dtype == torch.bfloat16:
        rows.assert_bf16_close(_f32(got), want, what)
    else:
        helpers.assert_float_close(_f32(got), want, what=what)


_REF = {}


def _reference(c, relu, keepProb):
    """float64 forward of a case over the whole [n, C] array, computed once and shared (read-only)."""
    key = (c, relu, keepProb)
    if key not in _REF:
        n, w = c.n, rc.width(c)
        d = rc.data(c)
        mask = None if keepProb is None else ref.keep_mask(SEED, n, w, ref.threshold(keepProb))
        scale = 1.0 if keepProb is None else 1.0 / keepProb
        _REF[key] = (ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, relu, mask, scale), mask, scale)
    return _REF[key]


_GATES = {}


def _gpu_gates(c):
    """The op's own gates, read off an f32 forward without dropout."""
    if c not in _GATES:
        _GATES[c] = _f32(_raw_fwd(c, True, None)[0][0]) > 0.0
    return _GATES[c]


def _launches_of(c):
    return 1 if c.n <= 256 else 2


# every case with f32 and with bf16 y / dy; a bf16 y of an odd C does not exist (MCCNN_E_SHAPE: tests/test_bn_cat_rows_cpu.py)
_TYPED = [(c, yb) for c in rc.CASES for yb in (False, True) if not (yb and rc.width(c) % 2)]


@pytest.mark.parametrize("keepProb", [None, 0.7], ids=["nodrop", "drop0.7"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("c,yb", _TYPED, ids=["%s-%s" % (rc.case_id(c), "bf16y" if yb else "f32y") for c, yb in _TYPED])
def test_bytes_and_reference(mc, c, yb, relu, keepProb):
    """Forward, moving statistics and backward of the typed entries: the launches of the existing entries; wherever both take
    the same columns per thread, their bytes on the widened segments (a bf16 dx_s: the rounding of their f32 dx_s); and every
    output within its bar of the float64 reference (dx, dgamma, dbeta with the GPU's own gates)."""
    import torch
    out, mask, scale = _reference(c, relu, keepProb)
    (y, saved, mm, mv), launches = _raw_fwd(c, relu, keepProb, y_bf16=yb)
    (wy, wsaved, wmm, wmv), wl = _raw_fwd(c, relu, keepProb, y_bf16=yb, widen=True)
    assert launches == wl == _launches_of(c)
    if rc.same_plan(c):
        assert _equal(y, wy) and _equal(saved, wsaved) and _equal(mm, wmm) and _equal(mv, wmv)
    helpers.assert_float_close(_f32(saved[0]), out["mean"], what="saved mean")
    helpers.assert_float_close(_f32(saved[1]), out["rstd"], what="saved rstd")
    helpers.assert_float_close(_f32(mm), out["mov_mean"], what="moving mean")
    helpers.assert_float_close(_f32(mv), out["mov_var"], what="moving variance")
    _check_out(y, out["y"], "y")
    # backward
    d = rc.data(c, yb)
    gates = _gpu_gates(c) if relu else None
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale, gate=gates)
    dxs, dg, db, bl = _raw_bwd(c, saved, relu, keepProb, dy_bf16=yb)
    wdxs, wdg, wdb, wbl = _raw_bwd(c, saved, relu, keepProb, dy_bf16=yb, widen=True)
    assert bl == wbl == _launches_of(c)
    assert [t.dtype for t in dxs] == [_torch_dtype(t) for t in c.types]
    if rc.same_plan(c):
        assert _equal(dg, wdg) and _equal(db, wdb)
        for t, a, b in zip(c.types, dxs, wdxs):
            assert b.dtype == torch.float32 and _equal(a, b.to(torch.bfloat16) if t else b)
    helpers.assert_float_close(_f32(dg), rdg, what="dgamma")
    helpers.assert_float_close(_f32(db), rdb, what="dbeta")
    # one scale for all segments, dx's own: the f32 segments at the float bar, the bf16 ones at the bf16 bar
    dx = np.concatenate([_f32(t) for t in dxs], 1)
    is_bf = np.concatenate([np.full(w, bool(t)) for w, t in zip(c.widths, c.types)])
    big = np.abs(rdx).max()
    if (~is_bf).any():
        got, want = dx[:, ~is_bf], rdx[:, ~is_bf]
        helpers.assert_float_close(np.concatenate([got.ravel(), [big]]), np.concatenate([want.ravel(), [big]]), what="dx of the f32 segments")
    got, want = dx[:, is_bf], rdx[:, is_bf]
    rows.assert_bf16_close(np.concatenate([got.ravel(), [big]]), np.concatenate([want.ravel(), [big]]), "dx of the bf16 segments")
    # no dx wanted: the same sums, byte for byte, from the same launches
    none, dg2, db2, l2 = _raw_bwd(c, saved, relu, keepProb, want=[False] * len(c.widths), dy_bf16=yb)
    assert all(t is None for t in none) and _equal(dg2, dg) and _equal(db2, db) and l2 == bl


@pytest.mark.parametrize("c", rc.CASES, ids=rc.IDS)
def test_dropped_set_is_exact(mc, c):
    """relu off, gamma = 1, beta = 10: no kept element is zero, so the zeros of y are the complement of the mask over
    (row, GLOBAL column), whatever the types of the segments."""
    n, w = c.n, rc.width(c)
    y = _raw_fwd(c, False, 0.7, gamma=np.ones(w, np.float32), beta=np.full(w, 10.0, np.float32))[0][0]
    assert np.array_equal(_f32(y) == 0.0, ~ref.keep_mask(SEED, n, w, ref.threshold(0.7)))


@pytest.mark.parametrize("c", rc.CASES, ids=rc.IDS)
def test_eval_forward(mc, c):
    d = rc.data(c)
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], False, True)
    for yb in (False, True) if rc.width(c) % 2 == 0 else (False,):
        (y, _saved, mm, mv), launches = _raw_fwd(c, True, 0.7, training=False, y_bf16=yb)   # (a keep probability is ignored in eval mode)
        _check_out(y, out["y"], "eval y")
        assert _f32(mm).tobytes() == d["mov_mean"].tobytes() and _f32(mv).tobytes() == d["mov_var"].tobytes()
        assert launches == 1
        if rc.same_plan(c):
            (wy, _s, _m, _v), wl = _raw_fwd(c, True, 0.7, training=False, y_bf16=yb, widen=True)
            assert _equal(y, wy) and wl == 1


@pytest.mark.parametrize("c", [rc.CASES[3], rc.CASES[6]], ids=[rc.IDS[3], rc.IDS[6]])
def test_raw_segments_without_a_gradient(mc, c):
    """A bf16 and an f32 segment that want no gradient, at 4 columns per thread (f b f) and at 1 (b f b): their dx stays
    untouched (NULL in the call), every other output keeps its bytes."""
    saved = _raw_fwd(c, True, 0.7)[0][1]
    full = _raw_bwd(c, saved, True, 0.7)
    for want in ([True, False, True], [False, True, False], [False, False, True]):
        part = _raw_bwd(c, saved, True, 0.7, want=want)
        assert part[3] == full[3] and _equal(part[1], full[1]) and _equal(part[2], full[2])
        for k, a, b in zip(want, part[0], full[0]):
            assert (a is None) if not k else _equal(a, b)


def _through_autograd(op, c, relu, keepProb, want=None, outDtype=None):
    """A Python route forward + backward through torch.autograd -> ([bits of y, dgamma, dbeta, the moving statistics and every
    segment's gradient (None where it has none)], y, the segments)."""
    import torch
    d = rc.data(c)
    want = [True] * len(c.widths) if want is None else want
    xs = [x.requires_grad_(k) for x, k in zip(_segments(c, d["x"]), want)]
    g, b = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    y = op(xs, g, b, mm, mv, True, relu, keepProb, SEED, outDtype=outDtype)
    y.backward(_dev(d["dy"]).to(y.dtype))
    torch.cuda.synchronize()
    return [_bits(y.detach()), _bits(g.grad), _bits(b.grad), _bits(mm), _bits(mv)] + [_bits(x.grad) for x in xs], y, xs


def _same(a, b):
    import torch
    return len(a) == len(b) and all((p is None and q is None) or (p is not None and q is not None and p.dtype == q.dtype and torch.equal(p, q))
                                    for p, q in zip(a, b))


@pytest.mark.parametrize("c", [rc.CASES[2], rc.CASES[5], rc.CASES[6], rc.CASES[9]],
                         ids=[rc.IDS[2], rc.IDS[5], rc.IDS[6], rc.IDS[9]])
def test_reproducible_and_extension_equals_ctypes(mc, c):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    a, y, xs = _through_autograd(M.bn_relu_dropout_cat, c, True, 0.7)
    b, _, _ = _through_autograd(M.bn_relu_dropout_cat, c, True, 0.7)
    assert _same(a, b)                                        # two runs: identical bytes for all outputs
    assert y.dtype == _torch_dtype(rc.out_dtype_is_bf16(c.types))      # outDtype=None: torch.cat's type
    assert [x.grad.dtype for x in xs] == [_torch_dtype(t) for t in c.types]
    out, _, _ = _reference(c, True, 0.7)
    _check_out(y.detach(), out["y"], "op y")
    raw = _raw_fwd(c, True, 0.7, y_bf16=rc.out_dtype_is_bf16(c.types))[0]
    assert _same([a[0], a[3], a[4]], [_bits(raw[0]), _bits(raw[2]), _bits(raw[3])])   # ... those of the C entry
    assert native._EXT is not None, "the torch extension did not load"
    e, ye, _ = _through_autograd(native.bn_relu_drop_cat, c, True, 0.7)
    assert _same(e, a)                                        # the extension entry: the same bytes, forward and backward
    assert type(ye.grad_fn).__name__ != "_BnReluDropoutCatBackward" and type(y.grad_fn).__name__ == "_BnReluDropoutCatBackward"
    for dt in (torch.float32, torch.bfloat16) if rc.width(c) % 2 == 0 else (torch.float32,):   # y's type asked for
        p, yp, _ = _through_autograd(M.bn_relu_dropout_cat, c, True, 0.7, outDtype=dt)
        q, yq, _ = _through_autograd(native.bn_relu_drop_cat, c, True, 0.7, outDtype=dt)
        assert yp.dtype == yq.dtype == dt and _same(p, q)
        assert _same(p[3:5], a[3:5])                          # the statistics do not know y's type


@pytest.mark.parametrize("c", [rc.CASES[3], rc.CASES[6]], ids=[rc.IDS[3], rc.IDS[6]])
def test_segment_without_a_gradient_gets_none(mc, c):
    """Both routes, a bf16 and an f32 segment in turn: the segment's gradient is None, every other output keeps its bytes."""
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import native
    full, _, _ = _through_autograd(M.bn_relu_dropout_cat, c, True, 0.7)
    for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
        for want in ([True, False, True], [False, True, True]):
            part, _, _ = _through_autograd(op, c, True, 0.7, want=want)
            assert _same(part[:5], full[:5])
            for k, a, b in zip(want, part[5:], full[5:]):
                assert (a is None) if not k else _same([a], [b])
        none, _, _ = _through_autograd(op, c, True, 0.7, want=[False] * 3)
        assert _same(none[:5], full[:5]) and none[5:] == [None] * 3


def _helper_runs(parts, gy, n_calls=1):
    """batch_norm_RELU_drop_out("L", list, ...) with fusedCat off and on, same inputs and seed -> per switch ([y, eval y,
    the segments' gradients ..., dgamma, dbeta], state_dict, dropCalls_, the node's name)."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    res = {}
    for fusedCat in (False, True):
        st = U.VariableStore(parts[0].device, fused=True, fusedCat=fusedCat)
        st.dropSeed_ = 11
        xs = [p.clone().requires_grad_(True) for p in parts]
        U.batch_norm_RELU_drop_out("L", xs, True, True, 0.8, st)            # creates the variables
        y = U.batch_norm_RELU_drop_out("L", xs, True, True, 0.8, st)
        y.backward(gy.to(y.dtype))
        with torch.no_grad():
            ye = U.batch_norm_RELU_drop_out("L", xs, False, True, 0.8, st)
        res[fusedCat] = ([y.detach(), ye] + [x.grad for x in xs] + [st.variables_["L_BN/gamma"].grad, st.variables_["L_BN/beta"].grad],
                         st.state_dict(), st.dropCalls_, y.grad_fn.name())
    torch.cuda.synchronize()
    return res[True], res[False]


@pytest.mark.parametrize("widths,types", [((8, 4, 12), (1, 0, 1)), ((16, 32), (0, 1)), ((3, 5, 2, 1), (1, 0, 1, 1)), ((2, 5), (0, 1))],
                         ids=["by4-bfb", "by4-fb", "C%4!=0-bfbb", "C%4!=0-fb"])
def test_helper_on_a_mixed_list_is_the_off_path_bit_for_bit(mc, widths, types):
    """Mixed lists where bn_cat_ref.plans_coincide: the off path is torch.cat (which widens) + the contiguous f32 op + autograd's
    slices cast back, i.e. "widen, then the contiguous f32 op" -- y, the four state tensors and every gradient are bit-equal,
    each segment's gradient has the segment's dtype, and dropCalls_ counts the same."""
    import torch
    assert cat.plans_coincide(cat.Case(0, widths, ())) and 0 in types and 1 in types
    dev = torch.device("cuda", 0)
    for n in (200, 5000):
        torch.manual_seed(n)
        parts = [(torch.randn(n, k, device=dev) * 3 + 5).to(_torch_dtype(t)) for k, t in zip(widths, types)]
        gy = torch.randn(n, sum(widths), device=dev)
        (on, sd_on, calls_on, name_on), (off, sd_off, calls_off, name_off) = _helper_runs(parts, gy)
        assert "Cat" in name_on and "Cat" not in name_off
        assert calls_on == calls_off == 2
        assert list(sd_on.keys()) == list(sd_off.keys()) == ["L_BN/gamma", "L_BN/beta", "L_BN/moving_mean", "L_BN/moving_variance"]
        assert on[0].dtype == off[0].dtype == torch.float32 and on[1].dtype == off[1].dtype == torch.float32
        assert [g.dtype for g in on[2:2 + len(widths)]] == [p.dtype for p in parts] == [g.dtype for g in off[2:2 + len(widths)]]
        for a, b in zip(on + [sd_on[k] for k in sd_on], off + [sd_off[k] for k in sd_off]):
            assert _equal(a, b)


@pytest.mark.parametrize("widths", [(8, 8), (32, 4, 28), (3, 5)], ids=["8+8", "32+4+28", "3+5"])
def test_helper_on_an_all_bf16_list_matches_the_off_path(mc, widths):
    """All bf16: the off path runs the contiguous op in its bf16 layout (64-column tiles, another merge order), so the two
    agree to the bars only -- f32 outputs (the state, dgamma, dbeta) at the float bar, bf16 outputs (y, the segments'
    gradients) at the bf16 bar against the other path widened -- with the same result dtype and the same dropCalls_."""
    import torch
    dev = torch.device("cuda", 0)
    for n in (200, 5000):
        torch.manual_seed(n + 1)
        parts = [(torch.randn(n, k, device=dev) * 3 + 5).to(torch.bfloat16) for k in widths]
        gy = torch.randn(n, sum(widths), device=dev)
        (on, sd_on, calls_on, name_on), (off, sd_off, calls_off, name_off) = _helper_runs(parts, gy)
        assert "Cat" in name_on and "Cat" not in name_off and calls_on == calls_off == 2
        assert on[0].dtype == off[0].dtype == torch.bfloat16 and on[1].dtype == off[1].dtype == torch.bfloat16
        assert all(g.dtype == torch.bfloat16 for g in on[2:2 + len(widths)] + off[2:2 + len(widths)])
        # one scale for the segments' gradients: dx's own
        k = len(widths)
        on_v = on[:2] + [torch.cat(on[2:2 + k], 1)] + on[2 + k:] + [sd_on[key] for key in sd_on]
        off_v = off[:2] + [torch.cat(off[2:2 + k], 1)] + off[2 + k:] + [sd_off[key] for key in sd_off]
        for a, b in zip(on_v, off_v):
            assert a.dtype == b.dtype
            _check_out(a, _f32(b).astype(np.float64), "helper output")


def test_launch_counts_of_typed_segments(mc):
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    for widths, types in (((24,), (1,)), ((8, 9, 7), (1, 0, 1)), ((3,) * 8, (0, 1) * 4)):
        w = sum(widths)
        for n, want in ((256, 1), (257, 2)):
            for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
                xs = [torch.randn(n, k, device=dev).to(_torch_dtype(t)).requires_grad_(True) for k, t in zip(widths, types)]
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


def test_mcseg_with_bf16_rows_reads_its_six_concatenations_in_place(mc, monkeypatch):
    """MCSeg(1, 4, 8, 3, 6, rows=bfloat16, fused=True, fusedCat=True) on the batch of tests/test_gpu_mcseg.py: every one of the
    six blocks over a concatenation goes through native._bn_cat_run (all bf16, or bf16 mixed with f32), the loss is finite,
    and logits, loss and every gradient are those of the same network with fusedCat off -- the path of before, torch.cat and
    the contiguous op -- within max(1e-4, 2 d) per quantity, d that quantity's distance between the fusedCat-off network with
    bf16 rows and with f32 rows: the network's own bf16 noise, measured here (a flipped bf16 rounding moves an element by
    2^-8 relative, so the 1e-4 bar of the f32 network need not hold).

    Observed on an MI355X: on against off logits 0.0e+00, loss 0.0e+00, worst gradient 1.7e-07 (Reduce_Pool_2_In_BN_BN/beta) over
    146 tensors; d, bf16 against f32 rows with fusedCat off: logits 3.2e-03, loss 1.4e-05, worst gradient 2.7e-01
    (Conv_3_biases3, an exactly-zero gradient measured against the floor)."""
    import torch
    import test_gpu_mcseg as seg
    from mcseg import MCSeg
    from mccnn_amd import native
    dev = torch.device("cuda", 0)
    calls = []
    real = native._bn_cat_run

    def counted(xs, *a, **k):
        calls.append(tuple(x.dtype for x in xs))
        return real(xs, *a, **k)
    monkeypatch.setattr(native, "_bn_cat_run", counted)
    torch.manual_seed(3)
    net = MCSeg(1, seg.B, seg.K, seg.NUM_CATS, seg.NUM_PARTS, dev, rows=torch.bfloat16, fused=True, fusedCat=True)
    with torch.no_grad():
        net(*seg._batch(dev)[:4], True, useDropOutFull=False)     # creates the variables
    assert len(calls) == 6
    start = {k: v.detach().clone() for k, v in net.state_dict().items()}
    res = {}
    for tag, fusedCat, rows_ in (("on", True, torch.bfloat16), ("off", False, torch.bfloat16), ("f32", False, None)):
        net.load_state_dict(start)                                 # (the moving statistics of the run before)
        net.store.fusedCat_, net.rows = fusedCat, rows_
        del calls[:]
        res[tag] = seg._run(net, dev)
        assert len(calls) == (6 if fusedCat else 0), (tag, calls)
        if fusedCat:
            bf, f32 = torch.bfloat16, torch.float32
            assert sorted(calls, key=str) == sorted([(bf, bf)] * 3 + [(bf, bf, bf)] * 2 + [(bf, bf, f32)], key=str), calls
    assert net.store.dropCalls_ == 0
    assert np.isfinite(res["on"][1]) and np.isfinite(res["on"][0]).all()
    assert res["on"][4] == res["off"][4] == res["f32"][4]
    e = seg._errors(res["on"], res["off"])
    d = seg._errors(res["off"], res["f32"])
    print("typed cat on vs off: " + seg._worst(e))
    print("bf16 rows vs f32 rows, both off: " + seg._worst(d))
    over = {k: (v, max(1e-4, 2 * d[k])) for k, v in e.items() if v > max(1e-4, 2 * d[k])}
    for k, (v, bar) in sorted(over.items()):
        print("  over its bar: %s %.2e > %.2e" % (k, v, bar))
    assert not over, over
