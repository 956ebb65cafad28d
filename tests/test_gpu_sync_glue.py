"""The dense glue with batch statistics across ranks on the GPU (mccnn_bn_sync_stats / _apply / _bwd_sums / _bwd_dx,
MCConvModule.bn_relu_dropout_sync, native.bn_relu_drop_sync, VariableStore(fused=True, fusedSync=True)).

In one process through the C-ABI: the shards of tests/sync_glue_ref.py's splits play the ranks -- stats per shard, the rows
stacked (the gather), apply per shard; likewise backward -- against the float64 WHOLE-batch reference of
tests/bn_act_ref.py at helpers.assert_float_close (1e-4, norm-wise and per element), the bar of the plain op. Then two
real ranks over gloo sharing the one GPU, through the helper layers."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bn_act_ref as ref  # noqa: E402
import bn_act_rows_ref as rows  # noqa: E402
import helpers  # noqa: E402
import sync_glue_ref as sref  # noqa: E402

SEED = 77
IDS = ["%dx%d" % s for s in sref.SHAPES]
shapes = pytest.mark.parametrize("shape", sref.SHAPES, ids=IDS)


def _dev(a, bf16=False):
    import torch
    t = torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))
    return t.to(torch.bfloat16) if bf16 else t


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    import torch
    t = t.detach().contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()


def _reference(shape, xb, relu, keepProb):
    """float64, whole batch -> (case, dict of ref.forward, mask, scale); x rounded to bf16 where it is a bf16 operand."""
    d = rows.case(shape[0], shape[1], xb, False)
    out, mask, scale = rows.reference(shape, xb, relu, keepProb, SEED)
    return d, out, mask, scale


def _sync_forward(d, shape, relu, keepProb, xb=False, yb=False, gamma=None, beta=None, bs=None):
    """The split forward through the C-ABI -> dict(y [per shard], saved, mm, mv, meta [per shard], parts [world, 3c],
    stats_launches, apply_launches [per shard], xs)."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    bs = bs or sref.bounds(shape)
    world, c = len(bs), shape[1]
    g, b = _dev(d["gamma"] if gamma is None else gamma), _dev(d["beta"] if beta is None else beta)
    xs = [_dev(d["x"][r0:r1], xb) for r0, r1 in bs]
    thr, scale = _bn_act_args(xs[0], g, b, g, g, keepProb, SEED)
    gathered = torch.empty((world, 3 * c), device=g.device)
    res = dict(y=[], saved=[], mm=[], mv=[], meta=[], stats_launches=[], apply_launches=[], xs=xs)
    for r, x in enumerate(xs):
        n = x.shape[0]
        parts = torch.full((world, 3 * c), float("nan"), device=g.device)
        ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_sync_stats(x.data_ptr(), int(xb), n, c, r, world, parts.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _lib.stream_handle()), "bn_sync_stats")
        res["stats_launches"].append(lib.mccnn_debug_launch_count() - before)
        raw = parts.view(torch.int32).cpu().numpy()
        assert not np.delete(raw, r, 0).any(), "another rank's row is not +0.0"         # (bit patterns: no -0.0, no NaN left)
        assert np.array_equal(_np(parts[r, :c]), np.full(c, n, np.float32))             # the count, per column
        gathered[r] = parts[r]
    for r, x in enumerate(xs):
        n = x.shape[0]
        mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
        y = torch.empty((n, c), dtype=torch.bfloat16 if yb else torch.float32, device=x.device)
        saved = torch.full((2, c), float("nan"), device=x.device)
        meta = torch.full((2,), -1, dtype=torch.int32, device=x.device)
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_sync_apply(x.data_ptr(), int(xb), n, c, r, world, gathered.data_ptr(), g.data_ptr(), b.data_ptr(),
                                           mm.data_ptr(), mv.data_ptr(), 0.99, 1e-3, int(relu), thr, scale, SEED, y.data_ptr(),
                                           int(yb), saved.data_ptr(), meta.data_ptr(), _lib.stream_handle()), "bn_sync_apply")
        res["apply_launches"].append(lib.mccnn_debug_launch_count() - before)
        for k, v in (("y", y), ("saved", saved), ("mm", mm), ("mv", mv), ("meta", meta)):
            res[k].append(v)
    torch.cuda.synchronize()
    res["parts"] = gathered
    return res


def _sync_backward(d, shape, fwd, relu, keepProb, xb=False, yb=False, want_dx=True, bs=None):
    """The split backward -> (dx [per shard], dgamma [per shard], dbeta [per shard], sums launches, dx launches)."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    bs = bs or sref.bounds(shape)
    world, c = len(bs), shape[1]
    g, b = _dev(d["gamma"]), _dev(d["beta"])
    dys = [_dev(d["dy"][r0:r1], yb) for r0, r1 in bs]
    thr, scale = _bn_act_args(fwd["xs"][0], g, b, g, g, keepProb, SEED)
    gathered = torch.empty((world, 3 * c), device=g.device)
    dgs, dbs, l1, l2, dxs = [], [], [], [], []
    for r, (x, dy) in enumerate(zip(fwd["xs"], dys)):
        n = x.shape[0]
        parts = torch.full((world, 3 * c), float("nan"), device=g.device)
        dg, db = torch.full((c,), float("nan"), device=g.device), torch.full((c,), float("nan"), device=g.device)
        ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_sync_bwd_sums(x.data_ptr(), int(xb), dy.data_ptr(), int(yb), n, c, r, world, g.data_ptr(), b.data_ptr(),
                                              fwd["saved"][r].data_ptr(), fwd["meta"][r].data_ptr(), int(relu), thr, scale, SEED,
                                              parts.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _lib.stream_handle()), "bn_sync_bwd_sums")
        l1.append(lib.mccnn_debug_launch_count() - before)
        raw = parts.view(torch.int32).cpu().numpy()
        assert not np.delete(raw, r, 0).any(), "another rank's row is not +0.0"
        assert _bits(parts[r, :c]) == _bits(db) and _bits(parts[r, c:2 * c]) == _bits(dg)   # this rank's own sums
        gathered[r] = parts[r]
        dgs.append(dg)
        dbs.append(db)
    for r, (x, dy) in enumerate(zip(fwd["xs"], dys)):
        n = x.shape[0]
        dx = torch.empty_like(x) if want_dx else None
        before = lib.mccnn_debug_launch_count()
        _lib.check(lib.mccnn_bn_sync_bwd_dx(x.data_ptr(), int(xb), dy.data_ptr(), int(yb), n, c, r, world, g.data_ptr(), b.data_ptr(),
                                            gathered.data_ptr(), fwd["saved"][r].data_ptr(), fwd["meta"][r].data_ptr(), int(relu),
                                            thr, scale, SEED, None if dx is None else dx.data_ptr(), dgs[r].data_ptr(),
                                            _lib.stream_handle()), "bn_sync_bwd_dx")
        l2.append(lib.mccnn_debug_launch_count() - before)
        dxs.append(dx)
    torch.cuda.synchronize()
    return dxs, dgs, dbs, l1, l2


def _cat(ts):
    return np.concatenate([_np(t) for t in ts])


_FWD = {}


def _forward_once(shape, relu, keepProb):
    """The f32 split forward of a configuration, run once and shared (read-only)."""
    key = (shape, relu, keepProb)
    if key not in _FWD:
        _FWD[key] = _sync_forward(rows.case(shape[0], shape[1], False, False), shape, relu, keepProb)
    return _FWD[key]


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("keepProb", [None, 0.7], ids=["nodrop", "drop0.7"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@shapes
def test_forward(mc, shape, relu, keepProb):
    d, out, _, _ = _reference(shape, False, relu, keepProb)
    o = _forward_once(shape, relu, keepProb)
    bs = sref.bounds(shape)
    helpers.assert_float_close(_cat(o["y"]), out["y"], what="y")
    for r, (r0, r1) in enumerate(bs):
        helpers.assert_float_close(_np(o["saved"][r])[0], out["mean"], what="saved mean")
        helpers.assert_float_close(_np(o["saved"][r])[1], out["rstd"], what="saved rstd")
        helpers.assert_float_close(_np(o["mm"][r]), out["mov_mean"], what="moving mean")
        helpers.assert_float_close(_np(o["mv"][r]), out["mov_var"], what="moving variance")
        for k in ("saved", "mm", "mv"):                         # from the same gathered partials: the same bytes everywhere
            assert _bits(o[k][r]) == _bits(o[k][0]), (k, r)
        assert o["meta"][r].cpu().tolist() == [r0, shape[0]]    # (rowBase, N)
        assert o["stats_launches"][r] == (1 if r1 - r0 <= 256 else 2)
        assert o["apply_launches"][r] == 1


@shapes
def test_dropped_set_is_the_whole_batch_mask(mc, shape):
    """relu off, gamma = 1, beta = 10: no kept element is zero, so the zeros of the concatenated y are the complement of the
    mask of the UNSHARDED batch -- the mask is taken at global rows."""
    n, c = shape
    d = rows.case(n, c, False, False)
    o = _sync_forward(d, shape, False, 0.7, gamma=np.ones(c, np.float32), beta=np.full(c, 10.0, np.float32))
    assert np.array_equal(_cat(o["y"]) == 0.0, ~ref.keep_mask(SEED, n, c, ref.threshold(0.7)))


def _gpu_gates(shape):
    return _cat(_forward_once(shape, True, None)["y"]) > 0.0


@shapes
def test_relu_gates(mc, shape):
    _, out, _, _ = _reference(shape, False, True, None)
    gates = _gpu_gates(shape)
    pre = out["pre"]
    band = np.abs(pre) <= 1e-5 * np.abs(pre).max()
    diff = gates != (pre > 0.0)
    assert not (diff & ~band).any()
    assert diff.sum() <= 1e-3 * pre.size


# ------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("relu,keepProb", [(True, 0.7), (True, None), (False, 0.7)], ids=["relu-drop", "relu", "linear-drop"])
@shapes
def test_backward(mc, shape, relu, keepProb):
    d, out, mask, scale = _reference(shape, False, relu, keepProb)
    fwd = _forward_once(shape, relu, keepProb)
    gates = _gpu_gates(shape) if relu else None
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale, gate=gates)
    dxs, dgs, dbs, l1, l2 = _sync_backward(d, shape, fwd, relu, keepProb)
    for r, (r0, r1) in enumerate(sref.bounds(shape)):
        # per shard, against the whole batch's dx: its scale and floor are those of the shard's rows
        helpers.assert_float_close(_np(dxs[r]), rdx[r0:r1], what="dx of shard %d" % r)
        assert l1[r] == (1 if r1 - r0 <= 256 else 2) and l2[r] == 1
    helpers.assert_float_close(_cat(dxs), rdx, what="dx")
    helpers.assert_float_close(np.sum([_np(t).astype(np.float64) for t in dgs], 0), rdg, what="sum of dgamma")
    helpers.assert_float_close(np.sum([_np(t).astype(np.float64) for t in dbs], 0), rdb, what="sum of dbeta")
    # dx not wanted: the same dgamma bytes, one launch
    _, dgs2, dbs2, _, l2b = _sync_backward(d, shape, fwd, relu, keepProb, want_dx=False)
    assert [_bits(t) for t in dgs2] == [_bits(t) for t in dgs] and [_bits(t) for t in dbs2] == [_bits(t) for t in dbs]
    assert l2b == [1] * len(l2b)


# ------------------------------------------------------------------------------------------------- types
@pytest.mark.parametrize("relu,keepProb", [(True, 0.7), (False, None)], ids=["relu-drop", "linear"])
def test_f32_rows_with_a_bf16_output_round_the_f32_result(mc, relu, keepProb):
    shape = (1000, 130)
    d = rows.case(shape[0], shape[1], False, True)              # (dy rounded to bf16: the f32 form reads it widened)
    a = _sync_forward(d, shape, relu, keepProb)
    b = _sync_forward(d, shape, relu, keepProb, yb=True)
    for r in range(len(a["y"])):
        for k in ("saved", "mm", "mv", "meta"):
            assert _bits(a[k][r]) == _bits(b[k][r]), (k, r)
        assert rows.to_bf16_bits(_np(a["y"][r])).tobytes() == _bits(b["y"][r])
    assert _bits(a["parts"]) == _bits(b["parts"])
    fa, fb = _sync_backward(d, shape, a, relu, keepProb), _sync_backward(d, shape, b, relu, keepProb, yb=True)
    for r in range(len(a["y"])):                                # a bf16 dy gives the gradients of the widened dy
        assert _bits(fa[0][r]) == _bits(fb[0][r]) and _bits(fa[1][r]) == _bits(fb[1][r]) and _bits(fa[2][r]) == _bits(fb[2][r])


@pytest.mark.parametrize("shape", [(1000, 130), (257, 64)], ids=lambda s: "%dx%d" % s)
def test_bf16_rows(mc, shape):
    """bf16 x: against the float64 reference on the rounded operands with an f32 y; a bf16 y changes the store only; dx has
    x's type."""
    import torch
    relu, keepProb = True, 0.7
    d, out, mask, scale = _reference(shape, True, relu, keepProb)
    d = rows.case(shape[0], shape[1], True, True)
    a = _sync_forward(d, shape, relu, keepProb, xb=True)
    b = _sync_forward(d, shape, relu, keepProb, xb=True, yb=True)
    helpers.assert_float_close(_cat(a["y"]), out["y"], what="y")
    helpers.assert_float_close(_np(a["saved"][0])[0], out["mean"], what="saved mean")
    helpers.assert_float_close(_np(a["saved"][0])[1], out["rstd"], what="saved rstd")
    for r in range(len(a["y"])):
        for k in ("saved", "mm", "mv"):
            assert _bits(a[k][r]) == _bits(b[k][r]) == _bits(a[k][0]), (k, r)
        assert rows.to_bf16_bits(_np(a["y"][r])).tobytes() == _bits(b["y"][r])
    y = _cat(a["y"])
    gates = np.where(mask, y > 0.0, out["pre"] > 0.0)           # the op's own gates where the mask kept an element
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale, gate=gates)
    dxs, dgs, dbs, _, _ = _sync_backward(d, shape, b, relu, keepProb, xb=True, yb=True)
    assert all(t.dtype == torch.bfloat16 for t in dxs)
    rows.assert_bf16_close(_cat(dxs), rdx, "dx")
    helpers.assert_float_close(np.sum([_np(t).astype(np.float64) for t in dgs], 0), rdg, what="sum of dgamma")
    helpers.assert_float_close(np.sum([_np(t).astype(np.float64) for t in dbs], 0), rdb, what="sum of dbeta")


# ------------------------------------------------------------------------------------------------- existing entries, errors
def _plain(d, relu, keepProb):
    """mccnn_bn_act_fwd + _bwd -> (bytes of y, saved, mm, mv, dx, dgamma, dbeta; forward launches, backward launches)."""
    import torch
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _bn_act_args, _ws
    lib = _lib.load()
    x, dy, g, b, mm, mv = (_dev(d[k]) for k in ("x", "dy", "gamma", "beta", "mov_mean", "mov_var"))
    n, c = x.shape
    thr, scale = _bn_act_args(x, g, b, mm, mv, keepProb, SEED)
    y, saved, dx = torch.empty_like(x), torch.empty((2, c), device=x.device), torch.empty_like(x)
    dg, db = torch.empty(c, device=x.device), torch.empty(c, device=x.device)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    l0 = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_bn_act_fwd(x.data_ptr(), n, c, g.data_ptr(), b.data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.99, 1e-3, 1,
                                    int(relu), thr, scale, SEED, y.data_ptr(), saved.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_handle()), "bn_act_fwd")
    l1 = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_bn_act_bwd(x.data_ptr(), dy.data_ptr(), n, c, g.data_ptr(), b.data_ptr(), saved.data_ptr(), int(relu), thr,
                                    scale, SEED, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_handle()), "bn_act_bwd")
    l2 = lib.mccnn_debug_launch_count()
    torch.cuda.synchronize()
    return [_bits(t) for t in (y, saved, mm, mv, dx, dg, db)], l1 - l0, l2 - l1


@pytest.mark.parametrize("shape", [(257, 64), (1000, 130), (63, 3)], ids=lambda s: "%dx%d" % s)
def test_plain_entries_are_untouched_and_one_rank_is_the_plain_forward(mc, shape):
    d = ref.case(*shape)
    before, f0, b0 = _plain(d, True, 0.7)
    assert (f0, b0) == ((1, 1) if shape[0] <= 256 else (2, 2))
    _forward_once(shape, True, 0.7)
    fwd = _sync_forward(d, shape, True, 0.7)
    _sync_backward(d, shape, fwd, True, 0.7)
    after, f1, b1 = _plain(d, True, 0.7)
    assert after == before and (f1, b1) == (f0, b0)
    # world == 1: the same partials merged in the same order, so the plain forward's bytes
    one = _sync_forward(d, shape, True, 0.7, bs=[(0, shape[0])])
    back = _sync_backward(d, shape, one, True, 0.7, bs=[(0, shape[0])])
    assert [_bits(one[k][0]) for k in ("y", "saved", "mm", "mv")] == before[:4]
    assert one["meta"][0].cpu().tolist() == [0, shape[0]]
    assert [_bits(back[0][0]), _bits(back[1][0]), _bits(back[2][0])] == before[4:]


@pytest.mark.parametrize("combo", [(True, True), (False, True), (True, False)], ids=["bf16-bf16", "f32-bf16", "bf16-f32"])
@pytest.mark.parametrize("shape", [(63, 6), (257, 8), (300, 72)], ids=lambda s: "%dx%d" % s)
def test_one_rank_on_typed_rows_is_the_typed_plain_op(mc, shape, combo):
    """The four stages with world == 1 give the bytes of mccnn_bn_act_fwd_rows / _bwd_rows whatever the types of x and y:
    the same merges in the same order, and the one rank's row added to nothing. Shapes: one launch on the pair form / two
    launches on the widest form / three slabs and more than one column tile."""
    import test_gpu_bn_act_rows as plain
    xb, yb = combo
    d = rows.case(shape[0], shape[1], xb, yb)
    bs = [(0, shape[0])]
    pf = plain._raw_fwd(d, xb, yb, True, 0.7)
    one = _sync_forward(d, shape, True, 0.7, xb=xb, yb=yb, bs=bs)
    assert [_bits(one[k][0]) for k in ("y", "saved", "mm", "mv")] == [_bits(pf[k]) for k in ("y", "saved", "mm", "mv")]
    assert one["meta"][0].cpu().tolist() == [0, shape[0]]
    for want_dx in (True, False):
        pdx, pdg, pdb, _ = plain._raw_bwd(d, xb, yb, pf["saved"], True, 0.7, want_dx=want_dx)
        dxs, dgs, dbs, _, _ = _sync_backward(d, shape, one, True, 0.7, xb=xb, yb=yb, want_dx=want_dx, bs=bs)
        assert (_bits(dgs[0]), _bits(dbs[0])) == (_bits(pdg), _bits(pdb)), want_dx
        assert (dxs[0] is None and pdx is None) if not want_dx else _bits(dxs[0]) == _bits(pdx)


def test_errors_come_before_any_launch(mc):
    import torch
    from mccnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n, c, world = 300, 8, 2
    x, y = torch.randn(n, c, device=dev), torch.empty(n, c, device=dev)
    parts = torch.zeros(world, 3 * c, device=dev)
    v = [torch.ones(c, device=dev) for _ in range(6)]
    saved, meta = torch.zeros(2, c, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mccnn_bn_act_workspace_bytes(n, c), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = _lib.stream_handle()

    def stats(x_=x, xb=0, n_=n, rank=0, world_=world, parts_=parts, ws_=ws, wsn=None):
        return lib.mccnn_bn_sync_stats(P(x_), xb, n_, c, rank, world_, P(parts_), P(ws_), ws.numel() if wsn is None else wsn, st)

    def apply(rank=0, world_=world, parts_=parts, yb=0, meta_=meta, thr=1 << 32):
        return lib.mccnn_bn_sync_apply(P(x), 0, n, c, rank, world_, P(parts_), P(v[0]), P(v[1]), P(v[2]), P(v[3]), 0.99, 1e-3, 1, thr,
                                       1.0, SEED, P(y), yb, P(saved), P(meta_), st)

    def sums(rank=0, world_=world, meta_=meta, wsn=None, db=2):
        return lib.mccnn_bn_sync_bwd_sums(P(x), 0, P(y), db - 2, n, c, rank, world_, P(v[0]), P(v[1]), P(saved), P(meta_), 1, 1 << 32,
                                          1.0, SEED, P(parts), P(v[4]), P(v[5]), P(ws), ws.numel() if wsn is None else wsn, st)

    def dx(rank=0, world_=world, dx_=y, dg=v[4], n_=n):
        return lib.mccnn_bn_sync_bwd_dx(P(x), 0, P(y), 0, n_, c, rank, world_, P(v[0]), P(v[1]), P(parts), P(saved), P(meta), 1,
                                        1 << 32, 1.0, SEED, P(dx_), P(dg), st)

    before = lib.mccnn_debug_launch_count()
    for f in (stats, apply, sums, dx):
        assert f(rank=world) == -1 and f(rank=-1) == -1 and f(world_=0) == -1            # MCCNN_E_BADARG
    assert stats(n_=(1 << 24) + 1) == -3 and dx(n_=(1 << 24) + 1) == -3                  # MCCNN_E_TOOLARGE
    assert stats(x_=None) == -1 and stats(parts_=None) == -1 and apply(parts_=None) == -1 and apply(meta_=None) == -1
    assert sums(meta_=None) == -1 and dx(dx_=None, dg=None) == -1
    assert stats(xb=2) == -1 and apply(yb=2) == -1 and sums(db=4) == -1                  # a type flag outside {0, 1}
    assert apply(thr=0) == -1 and apply(thr=(1 << 32) + 1) == -1
    assert stats(wsn=ws.numel() - 1) == -4 and stats(ws_=None) == -4 and sums(wsn=8) == -4   # MCCNN_E_WORKSPACE
    assert lib.mccnn_debug_launch_count() == before
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the op entries
def _through_autograd(op, d, xb, yb, keepProb, want_dx=True):
    import torch
    x = _dev(d["x"], xb).requires_grad_(want_dx)
    g, b = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    mm, mv = _dev(d["mov_mean"]), _dev(d["mov_var"])
    y = op(x, g, b, mm, mv, True, keepProb, SEED, outDtype=torch.bfloat16 if yb else torch.float32)
    y.backward(_dev(d["dy"], yb))
    torch.cuda.synchronize()
    return [_bits(t) for t in (y, x.grad if want_dx else torch.zeros(1), g.grad, b.grad, mm, mv)], y, x


@pytest.mark.parametrize("combo", [(False, False), (True, True), (False, True)], ids=["f32-f32", "bf16-bf16", "f32-bf16"])
@pytest.mark.parametrize("shape", [(257, 64), (1000, 130)], ids=lambda s: "%dx%d" % s)
def test_op_is_reproducible_and_extension_equals_ctypes(mc, shape, combo):
    """Without a process group the op runs as the one rank of a group of one: both forms, two runs, the same bytes -- and for
    f32 rows the bytes of the plain op."""
    import torch
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    xb, yb = combo
    d = rows.case(shape[0], shape[1], xb, yb)
    before = lib.mccnn_debug_launch_count()
    a, y, x = _through_autograd(M.bn_relu_dropout_sync, d, xb, yb, 0.7)
    small = shape[0] <= 256
    assert lib.mccnn_debug_launch_count() - before == (4 if small else 6)
    assert y.dtype == (torch.bfloat16 if yb else torch.float32) and x.grad.dtype == x.dtype
    assert _through_autograd(M.bn_relu_dropout_sync, d, xb, yb, 0.7)[0] == a
    assert native._EXT is not None, "the torch extension did not load"
    assert _through_autograd(native.bn_relu_drop_sync, d, xb, yb, 0.7)[0] == a
    nodx = _through_autograd(native.bn_relu_drop_sync, d, xb, yb, 0.7, want_dx=False)[0]
    assert nodx[2:] == a[2:]
    plain = lambda x_, g, b, mm, mv, relu, kp, seed, outDtype: M.bn_relu_dropout(x_, g, b, mm, mv, True, relu, kp, seed,  # noqa: E731
                                                                                   outDtype=outDtype)
    assert _through_autograd(plain, d, xb, yb, 0.7)[0] == a
    # the plain op's checks and texts; once differentiable
    with pytest.raises(M.InvalidArgumentError, match="keepProb"):
        M.bn_relu_dropout_sync(x, _dev(d["gamma"]), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"]), keepProb=1.5)
    with pytest.raises(M.InvalidArgumentError, match="group"):
        native.bn_relu_drop_sync(x, _dev(d["gamma"]), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"]), group="world")
    xx = _dev(d["x"], xb).requires_grad_(True)
    yy = M.bn_relu_dropout_sync(xx, _dev(d["gamma"]), _dev(d["beta"]), _dev(d["mov_mean"]), _dev(d["mov_var"]))
    (gx,) = torch.autograd.grad(yy.float().sum(), xx, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.float().sum().backward()


# ------------------------------------------------------------------------------------------------- two ranks
SHAPE2, CUT, KEEP = (1000, 130), 391, 0.7
H1, H2, NOUT = 32, 16, 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _network(x_np, dy_np, fusedSync, fused=True, rank_rows=None):
    """One glue block and an MLP_2_hidden over the rows x_np; the backward is a fixed linear functional of both outputs.
    -> dict of NumPy results and launch counts. rank_rows: (row0, row1) of these rows in the whole batch."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    d = ref.case(*SHAPE2)
    c = SHAPE2[1]
    r0, r1 = rank_rows or (0, SHAPE2[0])
    st = U.VariableStore(dev, fused=fused, fusedLinear=fused, fusedSync=fusedSync)
    st.dropSeed_ = SEED
    st.load_state_dict({"L_BN/gamma": torch.from_numpy(d["gamma"].copy()).to(dev), "L_BN/beta": torch.from_numpy(d["beta"].copy()).to(dev),
                        "L_BN/moving_mean": torch.from_numpy(d["mov_mean"].copy()).to(dev),
                        "L_BN/moving_variance": torch.from_numpy(d["mov_var"].copy()).to(dev)}, strict=False)
    x = torch.from_numpy(x_np.copy()).to(dev).requires_grad_(True)
    dy = torch.from_numpy(dy_np.copy()).to(dev)
    l0 = lib.mccnn_debug_launch_count()
    y = U.batch_norm_RELU_drop_out("L", x, True, True, KEEP, st)
    l1 = lib.mccnn_debug_launch_count()
    (y * dy).sum().backward()
    l2 = lib.mccnn_debug_launch_count()
    torch.manual_seed(7)                                        # the same MLP weights in every process
    x2 = torch.from_numpy(x_np.copy()).to(dev).requires_grad_(True)
    out = U.MLP_2_hidden(x2, c, H1, H2, NOUT, "M", KEEP, True, useDropOut=True, store=st)
    l3 = lib.mccnn_debug_launch_count()
    lin = torch.linspace(-1.0, 1.0, NOUT, device=dev) * torch.from_numpy(dy_np[:, :1].copy()).to(dev)
    (out * lin).sum().backward()
    l4 = lib.mccnn_debug_launch_count()
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    return dict(rows=(r0, r1), y=cpu(y), dx=cpu(x.grad), out=cpu(out), dx2=cpu(x2.grad),
                grads={k: cpu(p.grad) for k, p in st.named_parameters()}, params={k: cpu(p) for k, p in st.named_parameters()},
                buffers={k: cpu(b) for k, b in st.named_buffers()}, keys=list(st.state_dict().keys()), dropCalls=st.dropCalls_,
                launches=(l1 - l0, l2 - l1, l3 - l2, l4 - l3))


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        d = ref.case(*SHAPE2)
        r0, r1 = (0, CUT) if rank == 0 else (CUT, SHAPE2[0])
        on = _network(d["x"][r0:r1], d["dy"][r0:r1], True, rank_rows=(r0, r1))
        # the glue took library launches, forward and backward: stats (2: more than 256 rows) + apply, sums (2) + dx
        assert on["launches"][0] == 3 and on["launches"][1] == 3, on["launches"]
        assert on["launches"][2] == 9 and on["launches"][3] == 9, on["launches"]       # three blocks of the MLP likewise
        # fusedSync off: the torch sync path of today -- the bytes of a store that fuses nothing, and no library launch
        res = []
        for kw in (dict(fusedSync=False, fused=True), dict(fusedSync=False, fused=False)):
            torch.manual_seed(11)
            res.append(_network(d["x"][r0:r1], d["dy"][r0:r1], rank_rows=(r0, r1), **kw))
        off_same = all(res[0][k].tobytes() == res[1][k].tobytes() for k in ("y", "dx", "out", "dx2")) and \
            all(res[0]["grads"][k].tobytes() == res[1]["grads"][k].tobytes() for k in res[1]["grads"]) and \
            all(res[0]["buffers"][k].tobytes() == res[1]["buffers"][k].tobytes() for k in res[1]["buffers"])
        off_launches = (res[0]["launches"], res[0]["dropCalls"], res[0]["keys"] == on["keys"])
        q.put((rank, on, off_same, off_launches))
    finally:
        dist.destroy_process_group()


def _mlp_float64(x, lin, p, masks, scale):
    """MLP_2_hidden in float64 over the whole batch: forward, and the gradients of sum(out * lin) -> (out, dx, grads, moving,
    scales). scales: of the results that are cancelling sums whose true value is about 0 -- the gradient of a bias in front
    of a batch norm (sum_i dz[i, :]: held to the sum of the magnitudes, as tests/test_gpu_linear_bn.py holds db; the beta of
    the block in front of the first linear layer sums the same dz through w1) and the
    moving mean of a layer behind one (the mean of z: held to the spread of z, times 1 - momentum)."""
    f = {k: np.asarray(v, np.float64) for k, v in p.items()}
    z = np.zeros
    b0 = ref.forward(x, f["M_BN_Init/gamma"], f["M_BN_Init/beta"], z(x.shape[1]), np.ones(x.shape[1]), True, relu=False)
    z1 = b0["y"] @ f["M_weights1"] + f["M_biases1"]
    b1 = ref.forward(z1, f["M_BN_h1/gamma"], f["M_BN_h1/beta"], z(H1), np.ones(H1), True, True, masks[0], scale)
    z2 = b1["y"] @ f["M_weights2"] + f["M_biases2"]
    b2 = ref.forward(z2, f["M_BN_h2/gamma"], f["M_BN_h2/beta"], z(H2), np.ones(H2), True, True, masks[1], scale)
    out = b2["y"] @ f["M_weights3"] + f["M_biases3"]
    g = {}
    dout = np.asarray(lin, np.float64)
    g["M_weights3"], g["M_biases3"] = b2["y"].T @ dout, dout.sum(0)
    dz2, g["M_BN_h2/gamma"], g["M_BN_h2/beta"] = ref.backward(z2, dout @ f["M_weights3"].T, f["M_BN_h2/gamma"], f["M_BN_h2/beta"],
                                                              b2["mean"], b2["rstd"], True, masks[1], scale)
    g["M_weights2"], g["M_biases2"] = b1["y"].T @ dz2, dz2.sum(0)
    dz1, g["M_BN_h1/gamma"], g["M_BN_h1/beta"] = ref.backward(z1, dz2 @ f["M_weights2"].T, f["M_BN_h1/gamma"], f["M_BN_h1/beta"],
                                                              b1["mean"], b1["rstd"], True, masks[0], scale)
    g["M_weights1"], g["M_biases1"] = b0["y"].T @ dz1, dz1.sum(0)
    dx, g["M_BN_Init/gamma"], g["M_BN_Init/beta"] = ref.backward(x, dz1 @ f["M_weights1"].T, f["M_BN_Init/gamma"], f["M_BN_Init/beta"],
                                                                 b0["mean"], b0["rstd"], False)
    moving = {"M_BN_Init": b0, "M_BN_h1": b1, "M_BN_h2": b2}
    scales = {"M_biases1": np.abs(dz1).sum(0).max(), "M_biases2": np.abs(dz2).sum(0).max(),
              "M_BN_Init/beta": np.abs(dz1 @ f["M_weights1"].T).sum(0).max(),   # (sum_i of dz1 w1^T: dz1 sums to 0 over the rows)
              "M_BN_h1/moving_mean": 0.01 * np.sqrt(b1["var"]).max(), "M_BN_h2/moving_mean": 0.01 * np.sqrt(b2["var"]).max()}
    return out, dx, g, {k + "/moving_mean": v["mov_mean"] for k, v in moving.items()} | \
        {k + "/moving_variance": v["mov_var"] for k, v in moving.items()}, scales


def _close(got, want, what, scales):
    """assert_float_close, or for a cancelling sum (scales of _mlp_float64) |got - want| <= 1e-4 of its scale."""
    key = what.split(" ")[0]
    if key in scales:
        err = float(np.abs(np.asarray(got, np.float64) - want).max())
        assert err <= 1e-4 * scales[key], "%s: max |diff| %.3e > 1e-4 * %.3e" % (what, err, scales[key])
    else:
        helpers.assert_float_close(got, want, what=what)


def test_two_ranks_through_the_helpers_equal_the_whole_batch(mc):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    d = ref.case(*SHAPE2)
    n, c = SHAPE2
    single = _network(d["x"], d["dy"], False)                   # one process, fused=True: the plain library ops
    assert single["launches"][0] == 2 and single["dropCalls"] == 3
    on = [r[1] for r in res]
    # ---- fusedSync off: today's torch path, byte for byte, and not one library launch
    for rank, _, off_same, (launches, drop_calls, same_keys) in res:
        assert off_same and launches == (0, 0, 0, 0) and drop_calls == 0 and same_keys, rank
    # ---- the block against float64 over the whole batch and against the single process
    T, scale = ref.threshold(KEEP), float(np.float32(1.0) / np.float32(KEEP))
    mask = ref.keep_mask(SEED, n, c, T)
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, True, mask, scale)
    y = np.concatenate([o["y"] for o in on])
    dx = np.concatenate([o["dx"] for o in on])
    assert [o["rows"] for o in on] == [(0, CUT), (CUT, n)] and all(o["dropCalls"] == 3 and o["keys"] == single["keys"] for o in on)
    gates = np.where(mask, y > 0.0, out["pre"] > 0.0)
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], True, mask, scale, gate=gates)
    summed = {k: on[0]["grads"][k].astype(np.float64) + on[1]["grads"][k] for k in on[0]["grads"]}
    for want_y, want_dx, want_dg, want_db, mm, mv, tag in (
            (out["y"], rdx, rdg, rdb, out["mov_mean"], out["mov_var"], "float64"),
            (single["y"], single["dx"], single["grads"]["L_BN/gamma"], single["grads"]["L_BN/beta"],
             single["buffers"]["L_BN/moving_mean"], single["buffers"]["L_BN/moving_variance"], "single process")):
        helpers.assert_float_close(y, want_y, what="y vs " + tag)
        helpers.assert_float_close(dx, want_dx, what="dx vs " + tag)
        for o in on:
            r0, r1 = o["rows"]
            helpers.assert_float_close(o["y"], want_y[r0:r1], what="y slice vs " + tag)
            helpers.assert_float_close(o["dx"], want_dx[r0:r1], what="dx slice vs " + tag)
            helpers.assert_float_close(o["buffers"]["L_BN/moving_mean"], mm, what="moving mean vs " + tag)
            helpers.assert_float_close(o["buffers"]["L_BN/moving_variance"], mv, what="moving variance vs " + tag)
        helpers.assert_float_close(summed["L_BN/gamma"], want_dg, what="dgamma vs " + tag)
        helpers.assert_float_close(summed["L_BN/beta"], want_db, what="dbeta vs " + tag)
    assert not y[~mask].any() and not single["y"][~mask].any()  # the shards drop what the single process drops
    for k in on[0]["buffers"]:                                  # every moving statistic: the same bytes on both ranks
        assert on[0]["buffers"][k].tobytes() == on[1]["buffers"][k].tobytes(), k
    # ---- the MLP: fusedLinear leaves the synchronised case to the matmul + the sync op
    for k in on[0]["params"]:
        assert on[0]["params"][k].tobytes() == single["params"][k].tobytes() == on[1]["params"][k].tobytes(), k
    lin = np.linspace(-1.0, 1.0, NOUT, dtype=np.float32)[None, :] * d["dy"][:, :1]
    masks = [ref.keep_mask(SEED + 1, n, H1, T), ref.keep_mask(SEED + 2, n, H2, T)]
    fout, fdx, fg, fmoving, scales = _mlp_float64(d["x"], lin, single["params"], masks, scale)
    o2 = np.concatenate([o["out"] for o in on])
    dx2 = np.concatenate([o["dx2"] for o in on])
    names = [k for k in summed if k.startswith("M_")]
    assert len(names) == 12
    for want_out, want_dx, want_g, want_m, tag in ((fout, fdx, fg, fmoving, "float64"),
                                                   (single["out"], single["dx2"], single["grads"], single["buffers"], "single process")):
        helpers.assert_float_close(o2, want_out, what="MLP out vs " + tag)
        helpers.assert_float_close(dx2, want_dx, what="MLP dx vs " + tag)
        for o in on:
            r0, r1 = o["rows"]
            helpers.assert_float_close(o["out"], want_out[r0:r1], what="MLP out slice vs " + tag)
            helpers.assert_float_close(o["dx2"], want_dx[r0:r1], what="MLP dx slice vs " + tag)
            for k in want_m:
                if k.startswith("M_"):
                    _close(o["buffers"][k], want_m[k], k + " vs " + tag, scales)
        for k in names:
            _close(summed[k], want_g[k], k + " gradient vs " + tag, scales)
