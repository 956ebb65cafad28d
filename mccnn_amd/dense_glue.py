"""The dense glue between two MC convolutions as library ops (extensions; csrc/bn_act.hip, csrc/linear_bn.hip,
csrc/linear_xent.hip; include/mccnn.h "THE DENSE GLUE AS ONE OP" and the two sections behind it): y = drop(act(bn(x))) with the moving
statistics updated in place -- on its own (bn_relu_dropout), over a column-wise concatenation that is never materialised
(bn_relu_dropout_cat), with the batch statistics across the ranks of a process group (bn_relu_dropout_sync) and behind a
linear layer (linear_bn_relu_dropout). The dropout mask is counter-based
(csrc/bn_drop.h): reproducible from the seed, NOT torch's random stream. And what closes the dense path: the last linear
layer with the softmax cross-entropy, the predictions and the count of correct rows behind it (linear_softmax_xent,
csrc/linear_xent.hip), the cosine-distance loss of normal estimation (cosine_distance_loss, csrc/cosine_loss.hip), the
counts behind the IoU of segmentation (segmentation_counts, csrc/seg_counts.hip) and those behind ScanNet's voxel accuracy
(voxel_counts, csrc/voxel_acc.hip).

MCConvModule imports these names back: mccnn_amd.MCConvModule.bn_relu_dropout is this module's.
mccnn_amd.native has the forms that go through the torch extension.
"""
import numpy as _np
import torch

from . import _lib
from ._lib import check, ptr, stream_handle

BN_DROP_ALL = 1 << 32   # keep threshold of "no dropout"


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


# The checks the ops repeat, written once; (dtypes, their name in the messages):
_F32, _I32, _I64 = ((torch.float32,), "a float32"), ((torch.int32,), "an int32"), ((torch.int64,), "an int64")
_INT = ((torch.int32, torch.int64), "an int32 (or int64)")


def _typed(op, t, name, kind):
    _req(isinstance(t, torch.Tensor) and t.dtype in kind[0], "%s: %s must be %s tensor" % (op, name, kind[1]))


def _rows(op, t, name, kind, n, first, whose):
    """A row tensor: n elements of `kind` as (n,) or (n, 1), contiguous on the device of the op's first tensor (`whose` in the
    message) -> t as the library reads it, detached [n] (a view: nothing is launched)."""
    _typed(op, t, name, kind)
    _req(tuple(t.shape) in ((n,), (n, 1)), "%s: %s must have shape (n,) or (n, 1)" % (op, name))
    _req(t.device == first.device and t.is_contiguous(), "%s: %s must be contiguous on %s device" % (op, name, whose))
    return t.detach().reshape(n)


def _opt_rows(op, t, name, kind, n, first, whose):
    """An optional row tensor: None, or _rows."""
    return None if t is None else _rows(op, t, name, kind, n, first, whose)


def _shaped(op, t, name, kind, shape, text, first, whose):
    """A tensor of one given shape (`text` in the message) -- an `out`, a box: contiguous on the first tensor's device."""
    _typed(op, t, name, kind)
    _req(tuple(t.shape) == shape, "%s: %s must have shape %s" % (op, name, text))
    _req(t.device == first.device and t.is_contiguous(), "%s: %s must be contiguous on %s device" % (op, name, whose))


def _pos_int(op, v, name):
    _req(_is_int(v) and v >= 1, "%s expects %s >= 1" % (op, name))


def _ignore_label(op, v):
    """-> ignoreLabel as the library reads it: every negative value is -1, none."""
    _req(_is_int(v) and -(1 << 31) <= v < (1 << 31), "%s expects an integer ignoreLabel (< 0: none)" % op)
    return max(v, -1)


def _int32(t):
    """A checked int32 or int64 tensor as int32: the cast of an int64 one is one torch launch, so it comes behind the checks."""
    return t if t.dtype == torch.int32 else t.to(torch.int32)


def _linear_args(op, x, w, b, c):
    """The checks of x (n, cin), w (cin, c) and b (c,) that the two ops behind a linear layer share (c: the width's name in
    the messages)."""
    _typed(op, x, "x", _F32)
    _typed(op, w, "w", _F32)
    _req(x.dim() == 2 and w.dim() == 2 and x.shape[0] >= 1 and x.shape[1] >= 1 and w.shape[1] >= 1 and w.shape[0] == x.shape[1],
         "%s expects x (n, cin) and w (cin, %s), n, cin, %s >= 1" % (op, c, c))
    _req(x.is_contiguous() and w.is_contiguous(), "%s: x and w must be contiguous" % op)
    _req(w.device == x.device, "%s: w is on another device than x" % op)
    _req(isinstance(b, torch.Tensor) and b.dtype == torch.float32 and b.is_contiguous() and b.dim() == 1
         and b.shape[0] == w.shape[1] and b.device == x.device, "%s: b must be a float32 (%s,) tensor on x's device" % (op, c))
    _req(max(x.shape[0], x.shape[1], w.shape[1]) < (1 << 31), "%s: x too large" % op)


def _drop_args(op, keepProb, seed, outDtype):
    """The checks of keepProb, seed and outDtype that the ops share (op: the name in the messages) -> (keep threshold, keep
    scale). A threshold of 0 (a keepProb that keeps nothing) is the caller's to refuse, behind its other checks."""
    _req(keepProb is None or (isinstance(keepProb, (int, float)) and not isinstance(keepProb, bool) and 0.0 < keepProb <= 1.0),
         "%s expects keepProb in (0, 1] (or None)" % op)
    _req(_is_int(seed) and 0 <= seed < (1 << 32), "%s expects a seed in [0, 2^32)" % op)
    _req(outDtype is None or outDtype in (torch.float32, torch.bfloat16),
         "%s: outDtype must be None, torch.float32 or torch.bfloat16" % op)
    if keepProb is None:
        return BN_DROP_ALL, 1.0
    kp = float(keepProb)
    thr = int(kp * 4294967296.0)   # floor(keepProb * 2^32) in double
    return thr, float(_np.float32(1.0) / _np.float32(kp)) if thr >= 1 else 0.0   # 1.0f / (float) keepProb


def _bn_act_args(x, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype=None, *, training=True, sync=False, group=None):
    """Checks of bn_relu_dropout (nothing is launched before they pass) -> (keep threshold, keep scale). x: float32 or
    bfloat16 rows; outDtype: None (x's type), torch.float32 or torch.bfloat16; everything per column is float32. training=False
    adds the eval form's check, sync=True those of bn_relu_dropout_sync (its group, its rows), behind all the others."""
    thr, scale = _drop_args("bn_relu_dropout", keepProb, seed, outDtype)
    _req(isinstance(x, torch.Tensor) and x.dtype in (torch.float32, torch.bfloat16),
         "bn_relu_dropout: x must be a float32 (or bfloat16 storage) tensor")
    for t, name in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (movingMean, "moving_mean"), (movingVar, "moving_variance")):
        _req(isinstance(t, torch.Tensor) and (t is x or t.dtype == torch.float32),
             "bn_relu_dropout: %s must be a float32 tensor" % name)
        _req(t.is_contiguous(), "bn_relu_dropout: %s must be contiguous" % name)
    _req(x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] >= 1, "bn_relu_dropout expects x with dimensions (n, c), n, c >= 1")
    _req(x.shape[0] * x.shape[1] < (1 << 62) and max(x.shape) < (1 << 31), "bn_relu_dropout: x too large")
    _req(x.shape[1] % 2 == 0 or (x.dtype == torch.float32 and outDtype in (None, torch.float32)),
         "bn_relu_dropout: bfloat16 rows need an even number of columns")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (movingMean, "moving_mean"), (movingVar, "moving_variance")):
        _req(t.dim() == 1 and t.shape[0] == x.shape[1], "bn_relu_dropout: %s must have shape (c,)" % name)
        _req(t.device == x.device, "bn_relu_dropout: %s is on another device than x" % name)
    _req(x.is_cuda, "bn_relu_dropout: x must be a CUDA tensor")
    _req(thr >= 1, "bn_relu_dropout: keepProb keeps nothing")
    if not training:
        _req(not (torch.is_grad_enabled() and (x.requires_grad or gamma.requires_grad or beta.requires_grad)),
             "bn_relu_dropout: the eval form has no gradients")
    if sync:
        if group is not None:
            import torch.distributed as dist
            _req(dist.is_available() and isinstance(group, dist.ProcessGroup), "bn_relu_dropout_sync: group must be a process group (or None)")
        _req(x.shape[0] <= (1 << 24), "bn_relu_dropout: x too large")   # counts travel as float32
    return thr, scale


def _bn_act_fwd(lib, x, gamma, beta, movingMean, movingVar, momentum, epsilon, training, relu, thr, scale, seed, y, saved, ws):
    """The forward library call: the typed entry, whatever the types (the float32 entry is that one with both flags zero)."""
    check(lib.mccnn_bn_act_fwd_rows(ptr(x), int(x.dtype == torch.bfloat16), x.shape[0], x.shape[1], ptr(gamma), ptr(beta),
                                    ptr(movingMean), ptr(movingVar), momentum, epsilon, training, relu, thr, scale, seed,
                                    ptr(y), int(y.dtype == torch.bfloat16), ptr(saved), ptr(ws), 0 if ws is None else ws.numel(),
                                    stream_handle()), "bn_relu_dropout")


class _BnReluDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, movingMean, movingVar, relu, thr, scale, seed, momentum, epsilon, outDtype=None):
        lib = _lib.load()
        n, c = x.shape
        xd, gd, bd = _bf16_rows_aligned(x.detach()), gamma.detach(), beta.detach()
        y = torch.empty((n, c), dtype=outDtype or x.dtype, device=x.device)
        saved = torch.empty((2, c), dtype=torch.float32, device=x.device)
        ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
        _bn_act_fwd(lib, xd, gd, bd, movingMean, movingVar, momentum, epsilon, 1, int(relu), thr, scale, seed, y, saved, ws)
        ctx.save_for_backward(xd, gd, bd, saved)
        ctx.attrs = (int(relu), thr, scale, seed, y.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, gamma, beta, saved = ctx.saved_tensors
        relu, thr, scale, seed, ydt = ctx.attrs
        lib = _lib.load()
        n, c = x.shape
        gy = _bf16_rows_aligned(gy.to(ydt).contiguous())   # (dy has y's type; .to is a no-op when autograd hands that over)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dgb = torch.empty((2, c), dtype=torch.float32, device=x.device)
        ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
        check(lib.mccnn_bn_act_bwd_rows(ptr(x), int(x.dtype == torch.bfloat16), ptr(gy), int(ydt == torch.bfloat16), n, c,
                                        ptr(gamma), ptr(beta), ptr(saved), relu, thr, scale, seed, ptr(dx), ptr(dgb[0]),
                                        ptr(dgb[1]), ptr(ws), ws.numel(), stream_handle()), "bn_relu_dropout_grad")
        return (dx, dgb[0] if ctx.needs_input_grad[1] else None, dgb[1] if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None, None, None, None)


def bn_relu_dropout(x, gamma, beta, movingMean, movingVar, training, relu=True, keepProb=None, seed=0, momentum=0.99,
                    epsilon=1e-3, outDtype=None):
    """y = drop(act(bn(x))) over an [n, c] float32 contiguous tensor in one library op; differentiable (once) with respect
    to x, gamma and beta. training: batch statistics (biased variance), movingMean / movingVar updated in place as
    moving * momentum + stat * (1 - momentum), dropout with keep probability keepProb (None: none) from the counter-based
    mask of `seed`. Eval: the moving statistics, no dropout, and no gradients -- an input that requires one raises.
    x may also be bfloat16 rows (an even c), and outDtype names y's type (None: x's; torch.float32; torch.bfloat16), so the
    op is also the cast between layers that keep different row types: bf16 is widened exactly, the statistics and all
    arithmetic are float32 as for float32 rows, a bf16 y is rounded to nearest even at the store. x.grad has x's type,
    gamma.grad and beta.grad are float32."""
    return _bn_act_run(x, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype,
                       *_bn_act_args(x, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, training=training))


def _bn_act_run(x, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale):
    """bn_relu_dropout behind its checks: the arguments as given and what _bn_act_args made of keepProb."""
    if training:
        return _BnReluDropout.apply(x, gamma, beta, movingMean, movingVar, bool(relu), thr, scale, seed, float(momentum),
                                    float(epsilon), outDtype)
    lib = _lib.load()
    y = torch.empty(x.shape, dtype=outDtype or x.dtype, device=x.device)
    _bn_act_fwd(lib, _bf16_rows_aligned(x.detach()), gamma, beta, movingMean, movingVar, float(momentum), float(epsilon), 0,
                int(bool(relu)), BN_DROP_ALL, 1.0, seed, y, None, None)
    return y


# ---------------------------------------------------------------------------------------------
# ... over a column-wise concatenation that is never materialised (include/mccnn.h "... OVER A CONCATENATION"): up to 8
# segments [n, c_s], each float32 or bfloat16; y, and everything per column, at width C = sum c_s.
BN_CAT_MAX = 8


def _bn_cat_out_dtype(dtypes, outDtype=None):
    """y's type over segments of the types `dtypes`: outDtype where it is given, else what torch.cat of them would return --
    bfloat16 iff every segment is bfloat16, float32 otherwise."""
    if outDtype is not None:
        return outDtype
    return torch.bfloat16 if all(d == torch.bfloat16 for d in dtypes) else torch.float32


def _bn_cat_args(xs, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype=None, *, training=True):
    """Checks of bn_relu_dropout_cat (nothing is launched before they pass) -> (keep threshold, keep scale). xs: a list or
    tuple of 1 .. 8 contiguous (n, c_s) tensors on one device, each float32 or bfloat16; outDtype: None (_bn_cat_out_dtype:
    bfloat16 iff every segment is), torch.float32 or torch.bfloat16; everything per column is float32 (C,). training=False
    adds the eval form's check, behind all the others."""
    op = "bn_relu_dropout_cat"
    thr, scale = _drop_args(op, keepProb, seed, outDtype)
    _req(isinstance(xs, (list, tuple)) and 1 <= len(xs) <= BN_CAT_MAX, "%s expects a list of 1 to %d segments" % (op, BN_CAT_MAX))
    for x in xs:
        _req(isinstance(x, torch.Tensor) and x.dtype in (torch.float32, torch.bfloat16),
             "%s: every segment must be a float32 (or bfloat16 storage) tensor" % op)
        _req(x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] >= 1, "%s expects segments with dimensions (n, c_s), n, c_s >= 1" % op)
        _req(x.shape[0] == xs[0].shape[0], "%s: the segments must have the same number of rows" % op)
        _req(x.is_contiguous(), "%s: every segment must be contiguous" % op)
        _req(x.device == xs[0].device, "%s: the segments must be on one device" % op)
    n, c = xs[0].shape[0], sum(x.shape[1] for x in xs)
    _req(n < (1 << 31) and c < (1 << 31), "%s: x too large" % op)
    _req(c % 2 == 0 or _bn_cat_out_dtype([x.dtype for x in xs], outDtype) == torch.float32,
         "%s: bfloat16 rows need an even number of columns" % op)
    for t, name in ((gamma, "gamma"), (beta, "beta"), (movingMean, "moving_mean"), (movingVar, "moving_variance")):
        _req(isinstance(t, torch.Tensor) and t.dtype == torch.float32, "%s: %s must be a float32 tensor" % (op, name))
        _req(t.is_contiguous(), "%s: %s must be contiguous" % (op, name))
        _req(t.dim() == 1 and t.shape[0] == c, "%s: %s must have shape (C,), C the sum of the segments' widths" % (op, name))
        _req(t.device == xs[0].device, "%s: %s is on another device than the segments" % (op, name))
    _req(xs[0].is_cuda, "%s: the segments must be CUDA tensors" % op)
    _req(thr >= 1, "%s: keepProb keeps nothing" % op)
    if not training:
        _req(not (torch.is_grad_enabled() and any(t.requires_grad for t in tuple(xs) + (gamma, beta))),
             "%s: the eval form has no gradients" % op)
    return thr, scale


def _cat_table(ts):
    """The host arrays of a call: (pointers, bf16 flags, widths) of the tensors ts (None: a NULL pointer, flag and width 0)."""
    import ctypes as C
    return ((C.c_void_p * len(ts))(*[ptr(t) for t in ts]),
            (C.c_int * len(ts))(*[int(t is not None and t.dtype == torch.bfloat16) for t in ts]),
            (C.c_int * len(ts))(*[0 if t is None else t.shape[1] for t in ts]))


def _bn_cat_fwd(lib, xs, gamma, beta, movingMean, movingVar, momentum, epsilon, training, relu, thr, scale, seed, y, saved, ws):
    px, bf, cs = _cat_table(xs)
    check(lib.mccnn_bn_act_cat_fwd_rows(px, bf, cs, len(xs), xs[0].shape[0], ptr(gamma), ptr(beta), ptr(movingMean), ptr(movingVar),
                                        momentum, epsilon, training, relu, thr, scale, seed, ptr(y), int(y.dtype == torch.bfloat16),
                                        ptr(saved), ptr(ws), 0 if ws is None else ws.numel(), stream_handle()), "bn_relu_dropout_cat")


class _BnReluDropoutCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gamma, beta, movingMean, movingVar, relu, thr, scale, seed, momentum, epsilon, outDtype, *xs):
        lib = _lib.load()
        n, c = xs[0].shape[0], gamma.shape[0]
        xd, gd, bd = tuple(x.detach() for x in xs), gamma.detach(), beta.detach()
        y = torch.empty((n, c), dtype=_bn_cat_out_dtype([x.dtype for x in xs], outDtype), device=gamma.device)
        saved = torch.empty((2, c), dtype=torch.float32, device=gamma.device)
        ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), gamma.device)
        _bn_cat_fwd(lib, xd, gd, bd, movingMean, movingVar, momentum, epsilon, 1, int(relu), thr, scale, seed, y, saved, ws)
        ctx.save_for_backward(gd, bd, saved, *xd)
        ctx.attrs = (int(relu), thr, scale, seed, y.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        gamma, beta, saved = ctx.saved_tensors[:3]
        xs = ctx.saved_tensors[3:]
        relu, thr, scale, seed, ydt = ctx.attrs
        lib = _lib.load()
        n, c = xs[0].shape[0], gamma.shape[0]
        gy = _bf16_rows_aligned(gy.to(ydt).contiguous())
        need = ctx.needs_input_grad
        dxs = tuple(torch.empty_like(x) if need[11 + k] else None for k, x in enumerate(xs))
        dgb = torch.empty((2, c), dtype=torch.float32, device=gamma.device)
        ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), gamma.device)
        px, bf, cs = _cat_table(xs)
        pdx = _cat_table(dxs)[0] if any(d is not None for d in dxs) else None   # (dx_s is empty_like(x_s): x_s's type)
        check(lib.mccnn_bn_act_cat_bwd_rows(px, bf, cs, len(xs), ptr(gy), int(ydt == torch.bfloat16), n, ptr(gamma), ptr(beta),
                                            ptr(saved), relu, thr, scale, seed, pdx, ptr(dgb[0]), ptr(dgb[1]), ptr(ws), ws.numel(),
                                            stream_handle()), "bn_relu_dropout_cat_grad")
        return (dgb[0] if need[0] else None, dgb[1] if need[1] else None) + (None,) * 9 + dxs


def bn_relu_dropout_cat(xs, gamma, beta, movingMean, movingVar, training, relu=True, keepProb=None, seed=0, momentum=0.99,
                        epsilon=1e-3, outDtype=None):
    """bn_relu_dropout over torch.cat(xs, 1) in one library op, without the concatenation: xs a list or tuple of 1 .. 8
    contiguous (n, c_s) tensors, each float32 or bfloat16 on its own, gamma, beta and the moving statistics (C,), C = sum c_s;
    y is (n, C) of type outDtype -- None: what torch.cat(xs, 1) has, bfloat16 iff every segment is bfloat16 and float32
    otherwise; a bfloat16 y needs an even C. A bfloat16 segment is widened exactly on load, the statistics and all
    arithmetic are float32, and its gradient is bfloat16, rounded to nearest even at the store. The definition, the moving statistics, the mask -- element (row, column
    of the concatenation) -- and the eval form are bn_relu_dropout's; differentiable (once) with respect to every segment,
    gamma and beta: each segment that requires a gradient gets a contiguous one of its own, the others None. The launches
    are those of bn_relu_dropout on the concatenated float32 tensor, and wherever the library takes the same plan for both
    (C % 4 != 0, or every c_s % 4 == 0 and every tensor on a 16-byte boundary -- 8 bytes do for a bfloat16 segment) so are the
    bytes, a bfloat16 segment's gradient being that op's slice rounded to bfloat16."""
    return _bn_cat_run(xs, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype,
                       *_bn_cat_args(xs, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, training=training))


def _bn_cat_run(xs, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale):
    """bn_relu_dropout_cat behind its checks: the arguments as given and what _bn_cat_args made of keepProb."""
    if training:
        return _BnReluDropoutCat.apply(gamma, beta, movingMean, movingVar, bool(relu), thr, scale, seed, float(momentum),
                                       float(epsilon), outDtype, *xs)
    lib = _lib.load()
    y = torch.empty((xs[0].shape[0], gamma.shape[0]), dtype=_bn_cat_out_dtype([x.dtype for x in xs], outDtype), device=gamma.device)
    _bn_cat_fwd(lib, tuple(x.detach() for x in xs), gamma.detach(), beta.detach(), movingMean, movingVar, float(momentum),
                float(epsilon), 0, int(bool(relu)), BN_DROP_ALL, 1.0, seed, y, None, None)
    return y


# ---------------------------------------------------------------------------------------------
# ... with batch statistics across the ranks of a process group (include/mccnn.h "... WITH BATCH STATISTICS ACROSS RANKS"):
# the library op cut in two where the collective goes -- stats, gather, apply forward; sums, gather, dx backward. The
# collective is torch.distributed's (mccnn_amd.dist.gather_rows), so the autograd node is Python's, over four stage calls:
# the ctypes ones below, or the extension's (native.bn_relu_drop_sync) -- the same library calls, so the same bytes.
def _bn_sync_stats(x, rank, world, parts):
    lib = _lib.load()
    n, c = x.shape
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    check(lib.mccnn_bn_sync_stats(ptr(x), int(x.dtype == torch.bfloat16), n, c, rank, world, ptr(parts), ptr(ws), ws.numel(),
                                  stream_handle()), "bn_relu_dropout_sync")


def _bn_sync_apply(x, rank, world, parts, gamma, beta, movingMean, movingVar, momentum, epsilon, relu, thr, scale, seed, y, saved,
                   meta):
    lib = _lib.load()
    check(lib.mccnn_bn_sync_apply(ptr(x), int(x.dtype == torch.bfloat16), x.shape[0], x.shape[1], rank, world, ptr(parts), ptr(gamma),
                                  ptr(beta), ptr(movingMean), ptr(movingVar), momentum, epsilon, int(relu), thr, scale, seed, ptr(y),
                                  int(y.dtype == torch.bfloat16), ptr(saved), ptr(meta), stream_handle()), "bn_relu_dropout_sync")


def _bn_sync_bwd_sums(x, gy, rank, world, gamma, beta, saved, meta, relu, thr, scale, seed, partsB, dgb):
    lib = _lib.load()
    n, c = x.shape
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), x.device)
    check(lib.mccnn_bn_sync_bwd_sums(ptr(x), int(x.dtype == torch.bfloat16), ptr(gy), int(gy.dtype == torch.bfloat16), n, c, rank,
                                     world, ptr(gamma), ptr(beta), ptr(saved), ptr(meta), int(relu), thr, scale, seed, ptr(partsB),
                                     ptr(dgb[0]), ptr(dgb[1]), ptr(ws), ws.numel(), stream_handle()), "bn_relu_dropout_sync_grad")


def _bn_sync_bwd_dx(x, gy, rank, world, gamma, beta, partsB, saved, meta, relu, thr, scale, seed, dx, dgb):
    lib = _lib.load()
    check(lib.mccnn_bn_sync_bwd_dx(ptr(x), int(x.dtype == torch.bfloat16), ptr(gy), int(gy.dtype == torch.bfloat16), x.shape[0],
                                   x.shape[1], rank, world, ptr(gamma), ptr(beta), ptr(partsB), ptr(saved), ptr(meta), int(relu), thr,
                                   scale, seed, ptr(dx), ptr(dgb[0]), stream_handle()), "bn_relu_dropout_sync_grad")


_BN_SYNC_STAGES = (_bn_sync_stats, _bn_sync_apply, _bn_sync_bwd_sums, _bn_sync_bwd_dx)


def _bn_sync_place(group):
    """(rank, world) of this process in `group` (None: the default group); (0, 1) without a process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


class _BnReluDropoutSync(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, movingMean, movingVar, relu, thr, scale, seed, momentum, epsilon, outDtype, group, stages):
        from .dist import gather_rows
        rank, world = _bn_sync_place(group)
        n, c = x.shape
        xd, gd, bd = _bf16_rows_aligned(x.detach()), gamma.detach(), beta.detach()
        parts = torch.empty((world, 3 * c), dtype=torch.float32, device=x.device)
        stages[0](xd, rank, world, parts)
        parts = gather_rows(parts, group)
        y = torch.empty((n, c), dtype=outDtype or x.dtype, device=x.device)
        saved = torch.empty((2, c), dtype=torch.float32, device=x.device)
        meta = torch.empty((2,), dtype=torch.int32, device=x.device)
        stages[1](xd, rank, world, parts, gd, bd, movingMean, movingVar, momentum, epsilon, relu, thr, scale, seed, y, saved, meta)
        ctx.save_for_backward(xd, gd, bd, saved, meta)
        ctx.attrs = (relu, thr, scale, seed, y.dtype, group, stages, rank, world)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from .dist import gather_rows
        x, gamma, beta, saved, meta = ctx.saved_tensors
        relu, thr, scale, seed, ydt, group, stages, rank, world = ctx.attrs
        c = x.shape[1]
        gy = _bf16_rows_aligned(gy.to(ydt).contiguous())
        partsB = torch.empty((world, 3 * c), dtype=torch.float32, device=x.device)
        dgb = torch.empty((2, c), dtype=torch.float32, device=x.device)
        stages[2](x, gy, rank, world, gamma, beta, saved, meta, relu, thr, scale, seed, partsB, dgb)
        partsB = gather_rows(partsB, group)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        stages[3](x, gy, rank, world, gamma, beta, partsB, saved, meta, relu, thr, scale, seed, dx, dgb)
        return (dx, dgb[0] if ctx.needs_input_grad[1] else None, dgb[1] if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None, None, None, None, None, None)


def _bn_relu_dropout_sync(stages, x, gamma, beta, movingMean, movingVar, relu, keepProb, seed, momentum, epsilon, outDtype, group):
    return _bn_sync_run(x, gamma, beta, movingMean, movingVar, relu, seed, momentum, epsilon, outDtype, group,
                        *_bn_act_args(x, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, sync=True, group=group),
                        stages=stages)


def _bn_sync_run(x, gamma, beta, movingMean, movingVar, relu, seed, momentum, epsilon, outDtype, group, thr, scale,
                 stages=_BN_SYNC_STAGES):
    """bn_relu_dropout_sync behind its checks, over the four stage calls `stages` (the ctypes ones, or the extension's)."""
    return _BnReluDropoutSync.apply(x, gamma, beta, movingMean, movingVar, bool(relu), thr, scale, seed, float(momentum),
                                    float(epsilon), outDtype, group, stages)


def bn_relu_dropout_sync(x, gamma, beta, movingMean, movingVar, relu=True, keepProb=None, seed=0, momentum=0.99, epsilon=1e-3,
                         outDtype=None, group=None):
    """The training form of bn_relu_dropout (its definition, types, checks and errors) with the batch statistics over the
    rows of ALL ranks of `group` (None: the default process group; without one, this process alone): n, mean and var are
    those of the ranks' rows concatenated in rank order, and the dropout mask of a row is the mask of its global index, so
    with the same seed on every rank the shards reproduce the unsharded batch. Every rank of the group calls it, with at
    least one row; row counts may differ. Two collectives of 3c floats per rank, one forward and one backward
    (mccnn_amd.dist.gather_rows). movingMean / movingVar get the same bytes on every rank. x.grad is the gradient of the
    SUM of the ranks' losses; gamma.grad and beta.grad are this rank's share, to be added up by the caller's gradient
    all-reduce as for every other parameter. Differentiable once."""
    return _bn_relu_dropout_sync(_BN_SYNC_STAGES, x, gamma, beta, movingMean, movingVar, relu, keepProb, seed, momentum, epsilon,
                                 outDtype, group)


# ---------------------------------------------------------------------------------------------
# A linear layer and the dense glue behind it as one op (csrc/linear_bn.hip, include/mccnn.h "A LINEAR LAYER AND THE DENSE
# GLUE BEHIND IT AS ONE OP"): z = x @ w + b, y = drop(act(bn(z))).
def _linear_bn_args(x, w, b, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype=None, *, training=True):
    """Checks of linear_bn_relu_dropout (nothing is launched before they pass) -> (keep threshold, keep scale).
    training=False adds the eval form's check, behind all the others."""
    _linear_args("linear_bn_relu_dropout", x, w, b, "cout")
    thr, scale = _drop_args("linear_bn_relu_dropout", keepProb, seed, outDtype)
    _req(outDtype != torch.bfloat16 or w.shape[1] % 2 == 0, "linear_bn_relu_dropout: bfloat16 rows need an even number of columns")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (movingMean, "moving_mean"), (movingVar, "moving_variance")):
        _req(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1
             and t.shape[0] == w.shape[1] and t.device == x.device,
             "linear_bn_relu_dropout: %s must be a contiguous float32 (cout,) tensor on x's device" % name)
    _req(x.is_cuda, "linear_bn_relu_dropout: x must be a CUDA tensor")
    _req(thr >= 1, "linear_bn_relu_dropout: keepProb keeps nothing")
    if not training:
        _req(not (torch.is_grad_enabled() and any(t.requires_grad for t in (x, w, b, gamma, beta))),
             "linear_bn_relu_dropout: the eval form has no gradients")
    return thr, scale


class _LinearBnReluDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, movingMean, movingVar, relu, thr, scale, seed, momentum, epsilon, outDtype=None):
        lib = _lib.load()
        n, cin = x.shape
        cout = w.shape[1]
        xd, wd, bd, gd, bed = x.detach(), w.detach(), b.detach(), gamma.detach(), beta.detach()
        z = torch.empty((n, cout), dtype=torch.float32, device=x.device)
        y = torch.empty((n, cout), dtype=outDtype or torch.float32, device=x.device)
        saved = torch.empty((3, cout), dtype=torch.float32, device=x.device)
        ws = _ws(lib.mccnn_linear_bn_act_workspace_bytes(n, cin, cout), x.device)
        check(lib.mccnn_linear_bn_act_fwd(ptr(xd), ptr(wd), ptr(bd), n, cin, cout, ptr(gd), ptr(bed), ptr(movingMean), ptr(movingVar),
                                          momentum, epsilon, 1, int(relu), thr, scale, seed, ptr(z), ptr(y),
                                          int(y.dtype == torch.bfloat16), ptr(saved), ptr(ws), ws.numel(), stream_handle()),
              "linear_bn_relu_dropout")
        ctx.save_for_backward(xd, wd, gd, bed, z, saved)
        ctx.attrs = (int(relu), thr, scale, seed, y.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w, gamma, beta, z, saved = ctx.saved_tensors
        relu, thr, scale, seed, ydt = ctx.attrs
        lib = _lib.load()
        n, cin = x.shape
        cout = w.shape[1]
        gy = gy.to(ydt).contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        dv = torch.empty((3, cout), dtype=torch.float32, device=x.device)   # db, dgamma, dbeta
        ws = _ws(lib.mccnn_linear_bn_act_workspace_bytes(n, cin, cout), x.device)
        check(lib.mccnn_linear_bn_act_bwd(ptr(x), ptr(w), ptr(z), ptr(gy), int(ydt == torch.bfloat16), n, cin, cout, ptr(gamma),
                                          ptr(beta), ptr(saved), relu, thr, scale, seed, ptr(dx), ptr(dw), ptr(dv[0]), ptr(dv[1]),
                                          ptr(dv[2]), ptr(ws), ws.numel(), stream_handle()), "linear_bn_relu_dropout_grad")
        need = ctx.needs_input_grad
        return (dx, dw if need[1] else None, dv[0] if need[2] else None, dv[1] if need[3] else None,
                dv[2] if need[4] else None) + (None,) * 9


def linear_bn_relu_dropout(x, w, b, gamma, beta, movingMean, movingVar, training, relu=True, keepProb=None, seed=0,
                           momentum=0.99, epsilon=1e-3, outDtype=None):
    """y = drop(act(bn(x @ w + b))) in one library op: x (n, cin) and w (cin, cout) float32 contiguous, everything per
    column float32 (cout,). bn, act and drop are bn_relu_dropout's, applied to z = x @ w + b (batch statistics and the
    moving ones updated in place when training; the counter-based mask of `seed`); differentiable (once) with respect to
    x, w, b, gamma and beta. outDtype: y's type, None / torch.float32 or torch.bfloat16 (an even cout). Eval: the moving
    statistics, no dropout, and no gradients -- an input that requires one raises."""
    return _linear_bn_run(x, w, b, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype,
                          *_linear_bn_args(x, w, b, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, training=training))


def _linear_bn_run(x, w, b, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale):
    """linear_bn_relu_dropout behind its checks: the arguments as given and what _linear_bn_args made of keepProb."""
    if training:
        return _LinearBnReluDropout.apply(x, w, b, gamma, beta, movingMean, movingVar, bool(relu), thr, scale, seed,
                                          float(momentum), float(epsilon), outDtype)
    lib = _lib.load()
    n, cin = x.shape
    cout = w.shape[1]
    y = torch.empty((n, cout), dtype=outDtype or torch.float32, device=x.device)
    check(lib.mccnn_linear_bn_act_fwd(ptr(x.detach()), ptr(w.detach()), ptr(b.detach()), n, cin, cout, ptr(gamma.detach()),
                                      ptr(beta.detach()), ptr(movingMean), ptr(movingVar), float(momentum), float(epsilon), 0,
                                      int(bool(relu)), BN_DROP_ALL, 1.0, seed, None, ptr(y), int(y.dtype == torch.bfloat16), None,
                                      None, 0, stream_handle()), "linear_bn_relu_dropout")
    return y


# ---------------------------------------------------------------------------------------------
# The last linear layer and the softmax cross-entropy behind it as one op (csrc/linear_xent.hip, include/mccnn.h "THE LAST
# LINEAR LAYER AND THE SOFTMAX CROSS-ENTROPY BEHIND IT AS ONE OP"): x -> (loss, predictions, count of correct rows).
def _linear_xent_args(x, w, b, labels, weights=None, wantLogits=False):
    """Checks of linear_softmax_xent (nothing is launched before they pass) -> what _linear_xent_run takes: (x, w, b, labels,
    weights, wantLogits) with labels and weights as the library reads them: int32 [n] -- an int64 tensor is cast here, behind
    the checks, which is one torch launch -- and float32 [n] or None."""
    op = "linear_softmax_xent"
    _linear_args(op, x, w, b, "c")
    n = x.shape[0]
    labels = _rows(op, labels, "labels", _INT, n, x, "x's")
    rw = _opt_rows(op, weights, "weights", _F32, n, x, "x's")
    _req(rw is None or not (torch.is_grad_enabled() and weights.requires_grad), "%s: no gradient with respect to weights" % op)
    _req(x.is_cuda, "%s: x must be a CUDA tensor" % op)
    return x, w, b, _int32(labels), rw, bool(wantLogits)


class _LinearSoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, labels, weights, wantLogits):
        lib = _lib.load()
        n, cin = x.shape
        c = w.shape[1]
        xd, wd, bd = x.detach(), w.detach(), b.detach()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        lse = torch.empty((n,), dtype=torch.float32, device=x.device)
        pred = torch.empty((n,), dtype=torch.int32, device=x.device)
        meta = torch.empty((2,), dtype=torch.int32, device=x.device)
        logits = torch.empty((n, c), dtype=torch.float32, device=x.device) if wantLogits else None
        ws = _ws(lib.mccnn_linear_xent_workspace_bytes(n, cin, c), x.device)
        check(lib.mccnn_linear_xent_fwd(ptr(xd), ptr(wd), ptr(bd), n, cin, c, ptr(labels), ptr(weights), ptr(loss), ptr(lse), ptr(meta),
                                        ptr(pred), ptr(logits), ptr(ws), ws.numel(), stream_handle()), "linear_softmax_xent")
        ctx.save_for_backward(xd, wd, bd, labels, lse, meta)
        ctx.weights = weights
        if wantLogits:
            ctx.mark_non_differentiable(pred, meta, logits)
            return loss, pred, meta, logits
        ctx.mark_non_differentiable(pred, meta)
        return loss, pred, meta

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gl, *unused):
        x, w, b, labels, lse, meta = ctx.saved_tensors
        lib = _lib.load()
        n, cin = x.shape
        c = w.shape[1]
        gl = gl.to(torch.float32).contiguous()   # (one word on the device, read by the kernel: no read-back)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty_like(b)
        ws = _ws(lib.mccnn_linear_xent_workspace_bytes(n, cin, c), x.device)
        check(lib.mccnn_linear_xent_bwd(ptr(x), ptr(w), ptr(b), n, cin, c, ptr(labels), ptr(ctx.weights), ptr(lse), ptr(meta), ptr(gl),
                                        ptr(dx), ptr(dw), ptr(db), ptr(ws), ws.numel(), stream_handle()), "linear_softmax_xent_grad")
        need = ctx.needs_input_grad
        return dx, dw if need[1] else None, db if need[2] else None, None, None, None


def linear_softmax_xent(x, w, b, labels, weights=None, wantLogits=False):
    """The sparse softmax cross-entropy of z = x @ w + b in one library op -> (loss, pred, meta, logits or None). x (n, cin),
    w (cin, c), b (c,) float32 contiguous; labels (n,) or (n, 1), int32 taken as it is, int64 cast to int32 (one torch
    launch); weights: float32 (n,) row weights, None: all 1. A row is live iff 0 <= label < c and its weight is not 0 -- a label
    outside [0, c) makes a weight-0 row, never an error. loss (0-dim float32) = sum over live rows of weight * (logsumexp(z_i)
    - z[i, label_i]) / D with D = max(number of live rows, 1): the mean without weights, TF's SUM_BY_NONZERO_WEIGHTS with
    them; +0 and zero gradients when no row is live. pred (int32 (n,)): the lowest arg-max of every row; meta (int32 (2,)):
    D and the number of live rows with pred == label. loss is differentiable (once) with respect to x, w and b, all three
    gradients from one autograd node whose upstream gradient stays on the device. pred, meta and logits are NOT
    differentiable: whoever needs gradients through the logits uses the unfused path (x @ w + b and torch's loss)."""
    return _linear_xent_run(*_linear_xent_args(x, w, b, labels, weights, wantLogits))


def _linear_xent_run(x, w, b, labels, weights, wantLogits):
    """linear_softmax_xent behind its checks, over what _linear_xent_args returns."""
    out = _LinearSoftmaxXent.apply(x, w, b, labels, weights, wantLogits)
    return out if wantLogits else out + (None,)


# ---------------------------------------------------------------------------------------------
# The cosine-distance loss of normal estimation as one op (csrc/cosine_loss.hip, include/mccnn.h "THE COSINE-DISTANCE LOSS OF
# NORMAL ESTIMATION AS ONE OP"): (pred, target) -> (loss, sums, meta).
def _cosine_loss_args(pred, target, weights=None):
    """Checks of cosine_distance_loss (nothing is launched before they pass) -> what _cosine_loss_run takes: (pred, target,
    weights) with the weights as the library reads them: float32 [n] or None."""
    _typed("cosine_distance_loss", pred, "pred", _F32)
    _typed("cosine_distance_loss", target, "target", _F32)
    _req(pred.dim() == 2 and pred.shape[0] >= 1 and pred.shape[1] >= 1 and tuple(target.shape) == tuple(pred.shape),
         "cosine_distance_loss expects pred (n, c) and target (n, c), n, c >= 1")
    _req(pred.is_contiguous() and target.is_contiguous(), "cosine_distance_loss: pred and target must be contiguous")
    _req(target.device == pred.device, "cosine_distance_loss: target is on another device than pred")
    _req(pred.shape[0] * pred.shape[1] < (1 << 31), "cosine_distance_loss: pred too large")
    _req(not (torch.is_grad_enabled() and target.requires_grad), "cosine_distance_loss: no gradient with respect to target")
    rw = _opt_rows("cosine_distance_loss", weights, "weights", _F32, pred.shape[0], pred, "pred's")
    _req(rw is None or not (torch.is_grad_enabled() and weights.requires_grad), "cosine_distance_loss: no gradient with respect to weights")
    _req(pred.is_cuda, "cosine_distance_loss: pred must be a CUDA tensor")
    return pred, target, rw


class _CosineDistanceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weights):
        lib = _lib.load()
        n, c = pred.shape
        pd, td = pred.detach(), target.detach()
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        sums = torch.empty((2,), dtype=torch.float32, device=pred.device)
        meta = torch.empty((1,), dtype=torch.int32, device=pred.device)
        ws = _ws(lib.mccnn_cosine_loss_workspace_bytes(n, c), pred.device)
        check(lib.mccnn_cosine_loss_fwd(ptr(pd), ptr(td), n, c, ptr(weights), ptr(loss), ptr(sums), ptr(meta), ptr(ws), ws.numel(),
                                        stream_handle()), "cosine_distance_loss")
        ctx.save_for_backward(pd, td, meta)
        ctx.weights = weights
        ctx.mark_non_differentiable(sums, meta)
        return loss, sums, meta

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gl, *unused):
        pred, target, meta = ctx.saved_tensors
        lib = _lib.load()
        n, c = pred.shape
        gl = gl.to(torch.float32).contiguous()   # (one word on the device, read by the kernel: no read-back)
        dpred = torch.empty_like(pred)
        check(lib.mccnn_cosine_loss_bwd(ptr(pred), ptr(target), n, c, ptr(ctx.weights), ptr(meta), ptr(gl), ptr(dpred),
                                        stream_handle()), "cosine_distance_loss_grad")
        return dpred, None, None


def cosine_distance_loss(pred, target, weights=None):
    """The cosine-distance loss of normal estimation in one library op -> (loss, sums, meta). pred, target (n, c) float32
    contiguous (no alignment rule: a view that starts anywhere in its buffer is fine); weights: float32 (n,) or (n, 1) row
    weights, None: all 1. Both rows are normalised as tf.nn.l2_normalize does (x / sqrt(max(sum x^2, 1e-12))), cos_i is
    their dot product. A row is live iff its weight is not 0. loss (0-dim float32) = sum over live rows of weight * (1 - cos_i)
    / D with D = max(number of live rows, 1): the mean without weights, TF's SUM_BY_NONZERO_WEIGHTS with them; +0 and zero
    gradients when no row is live. sums (float32 (2,)): the sum over live rows of cos_i and of the angle between the two
    unit rows in radians, 2 atan2(|u - v|, |u + v|); meta (int32 (1,)): D. loss is differentiable (once) with respect to pred,
    the upstream gradient stays on the device; there is no gradient with respect to target or weights (asking for one
    raises), and sums and meta are NOT differentiable."""
    return _cosine_loss_run(*_cosine_loss_args(pred, target, weights))


def _cosine_loss_run(pred, target, weights):
    """cosine_distance_loss behind its checks, over what _cosine_loss_args returns."""
    return _CosineDistanceLoss.apply(pred, target, weights)


# ---------------------------------------------------------------------------------------------
# Segmentation scores on the device (csrc/seg_counts.hip, include/mccnn.h "SEGMENTATION SCORES ON THE DEVICE: PER-CLOUD,
# PER-CLASS COUNTS"): (pred, labels) -> int64 [numClouds, numClasses, 3] counts of intersection, union and ground truth.
def _seg_counts_args(pred, labels, numClasses, batchIds=None, numClouds=1, weights=None, ignoreLabel=-1, out=None):
    """Checks of segmentation_counts (nothing is launched before they pass) -> what _seg_counts_run takes: its own arguments
    with pred, labels, batchIds and weights as the library reads them -- int32 [n] (an int64 pred or labels is cast here,
    behind the checks, one torch launch each), int32 [n] or None, float32 [n] or None -- and every negative ignoreLabel as -1."""
    op = "segmentation_counts"
    _pos_int(op, numClasses, "numClasses")
    _pos_int(op, numClouds, "numClouds")
    _req(numClouds * numClasses * 3 < (1 << 31), "%s: numClouds * numClasses too large" % op)
    ignoreLabel = _ignore_label(op, ignoreLabel)
    _typed(op, pred, "pred", _INT)
    _req(pred.dim() in (1, 2) and (pred.dim() == 1 or pred.shape[1] == 1), "%s: pred must have shape (n,) or (n, 1)" % op)
    n = pred.shape[0]
    _req(n < (1 << 31), "%s: pred too large" % op)
    _req(pred.is_contiguous(), "%s: pred must be contiguous" % op)
    labels = _rows(op, labels, "labels", _INT, n, pred, "pred's")
    batchIds = _opt_rows(op, batchIds, "batchIds", _I32, n, pred, "pred's")
    rw = _opt_rows(op, weights, "weights", _F32, n, pred, "pred's")
    _req(rw is None or not weights.requires_grad, "%s: no gradient with respect to weights" % op)
    if out is not None:
        _shaped(op, out, "out", _I64, (numClouds, numClasses, 3), "(numClouds, numClasses, 3)", pred, "pred's")
    _req(pred.is_cuda, "%s: pred must be a CUDA tensor" % op)
    return _int32(pred.detach().reshape(n)), _int32(labels), numClasses, batchIds, numClouds, rw, ignoreLabel, out


def segmentation_counts(pred, labels, numClasses, batchIds=None, numClouds=1, weights=None, ignoreLabel=-1, out=None):
    """The counts behind the IoU of segmentation in one library launch -> counts, int64 (numClouds, numClasses, 3) on pred's
    device: per cloud and class the intersection I, the union U and the ground truth G. pred, labels: (n,) or (n, 1), int32
    taken as it is, int64 cast to int32 (one torch launch each); batchIds: int32 (n,) or (n, 1), None: every row is cloud 0;
    weights: float32 (n,) or (n, 1), None: all 1. A row is live iff 0 <= label < numClasses, label != ignoreLabel (< 0:
    none), its weight is not 0 and 0 <= batch id < numClouds -- a bad batch id makes a dead row, it is never counted for
    another cloud. A live row adds 1 to G of its label; a hit adds 1 to I and U of it; a miss adds 1 to U of the label and to
    U of the prediction where that is a class (a prediction outside [0, numClasses) is a miss and nothing else). out: None
    makes a zeroed tensor; a given one is ADDED to and returned, so a caller accumulates over as many batches as it likes.
    Integer atomics only: the same inputs give the same bytes. Nothing is differentiable and nothing is read back."""
    return _seg_counts_run(*_seg_counts_args(pred, labels, numClasses, batchIds, numClouds, weights, ignoreLabel, out))


def _seg_counts_run(pred, labels, numClasses, batchIds, numClouds, weights, ignoreLabel, out):
    """segmentation_counts behind its checks, over what _seg_counts_args returns."""
    lib = _lib.load()
    if out is None:
        out = torch.zeros((numClouds, numClasses, 3), dtype=torch.int64, device=pred.device)
    check(lib.mccnn_seg_counts_add(ptr(pred), ptr(labels), ptr(weights), ptr(batchIds), pred.shape[0], numClouds, numClasses,
                                   ignoreLabel, ptr(out), stream_handle()), "segmentation_counts")
    return out


# ---------------------------------------------------------------------------------------------
# Voxel accuracy on the device (csrc/voxel_acc.hip, include/mccnn.h "VOXEL ACCURACY ON THE DEVICE: PER-VOXEL MAJORITY VOTES"):
# (points, pred, labels, box minimum) -> int64 [numClouds, numClasses, 2] counts of valid voxels whose votes agree (V) and of
# all valid voxels (G), per cloud and majority label.
_VOXEL_WS = {}   # (device index, raw stream, cap_rec, numClasses) -> the hash table: all zero between calls
_VOXEL_WS_MAX = 8


def voxel_cap_rec(n):
    """The recommended slots of the table for n rows: the smallest power of two >= max(2 n, 64)."""
    cap = 64
    while cap < 2 * n:
        cap <<= 1
    return cap


def _voxel_ws(n, numClasses, device):
    """The op's hash table: a torch.zeros tensor of mccnn_voxel_acc_workspace_bytes(n, C) bytes kept per (device, stream,
    cap_rec, C). Zeroed ONCE: every call leaves what it used all zero again, so it is handed over with ws_clean = 1. Calls on
    one stream are ordered; another stream gets a table of its own."""
    cap = voxel_cap_rec(n)
    key = (device.index, stream_handle(), cap, numClasses)
    ws = _VOXEL_WS.get(key)
    if ws is None:
        while len(_VOXEL_WS) >= _VOXEL_WS_MAX:
            _VOXEL_WS.pop(next(iter(_VOXEL_WS)))
        ws = _VOXEL_WS[key] = torch.zeros(cap * (8 + 8 * numClasses), dtype=torch.uint8, device=device)
    return ws


def _voxel_counts_args(points, pred, labels, numClasses, batchIds=None, numClouds=1, aabbMin=None, resolution=0.05,
                       ignoreLabel=-1, maxIgnoreShare=0.3, out=None, dropped=None):
    """Checks of voxel_counts (nothing is launched before they pass) -> what _voxel_counts_run takes: its own arguments with
    points, pred, labels, batchIds, aabbMin, resolution and maxIgnoreShare as the library reads them -- float32 [n, 3], int32
    [n] (an int64 pred or labels is cast here, behind the checks, one torch launch each), int32 [n] or None, float32
    [numClouds, 3], the float32 value of resolution as a float, a float -- and every negative ignoreLabel as -1."""
    op = "voxel_counts"
    _pos_int(op, numClasses, "numClasses")
    _pos_int(op, numClouds, "numClouds")
    _req(numClouds <= 32768 and numClouds * numClasses * 2 < (1 << 31), "%s: numClouds (<= 32768) * numClasses too large" % op)
    ignoreLabel = _ignore_label(op, ignoreLabel)
    _req(isinstance(resolution, (int, float, _np.floating)) and not isinstance(resolution, bool), "%s expects a number as resolution" % op)
    with _np.errstate(over="ignore"):
        res = float(_np.float32(resolution))
    _req(res > 0.0 and res != float("inf"), "%s expects a finite resolution > 0 (as float32)" % op)
    _req(isinstance(maxIgnoreShare, (int, float, _np.floating)) and not isinstance(maxIgnoreShare, bool),
         "%s expects a number as maxIgnoreShare" % op)
    _typed(op, points, "points", _F32)
    _req(points.dim() == 2 and points.shape[1] == 3, "%s: points must have shape (n, 3)" % op)
    n = points.shape[0]
    _req(n < (1 << 30), "%s: points too large" % op)
    _req(points.is_contiguous(), "%s: points must be contiguous" % op)
    pred = _rows(op, pred, "pred", _INT, n, points, "points'")
    labels = _rows(op, labels, "labels", _INT, n, points, "points'")
    batchIds = _opt_rows(op, batchIds, "batchIds", _I32, n, points, "points'")
    _shaped(op, aabbMin, "aabbMin", _F32, (numClouds, 3), "(numClouds, 3)", points, "points'")
    if out is not None:
        _shaped(op, out, "out", _I64, (numClouds, numClasses, 2), "(numClouds, numClasses, 2)", points, "points'")
    if dropped is not None:
        _typed(op, dropped, "dropped", _I32)
        _req(dropped.numel() == 1 and dropped.device == points.device, "%s: dropped must have one element on points' device" % op)
    _req(points.is_cuda, "%s: points must be a CUDA tensor" % op)
    return (points.detach(), _int32(pred), _int32(labels), numClasses, batchIds, numClouds, aabbMin.detach(), res, ignoreLabel,
            float(maxIgnoreShare), out, dropped)


def voxel_counts(points, pred, labels, numClasses, batchIds=None, numClouds=1, aabbMin=None, resolution=0.05, ignoreLabel=-1,
                 maxIgnoreShare=0.3, out=None, dropped=None):
    """The counts behind ScanNet's voxel accuracy in two library launches -> counts, int64 (numClouds, numClasses, 2) on
    points' device: per cloud b and class c, [b, c, 1] = G, the valid voxels whose most frequent label is c, and [b, c, 0] =
    V, those of them whose most frequent prediction is c too. points: float32 (n, 3); pred, labels: (n,) or (n, 1), int32
    taken as it is, int64 cast to int32 (one torch launch each); batchIds: int32 (n,) or (n, 1), None: every row is cloud 0;
    aabbMin: float32 (numClouds, 3), the corner the grid of every cloud starts at (required here; the helper of
    MCNetworkUtils computes it). A row's voxel is (b, ceilf((p - aabbMin[b]) / resolution)) per axis in float32; a row is dead
    iff its label is outside [0, numClasses), its batch id outside [0, numClouds) -- never counted for another cloud -- or a
    coordinate is not finite, below 0 or above 65535 (dropped, optional int32 device word, is incremented by the number of
    such rows; it is never read here). A row with label ignoreLabel (< 0: none) is live. Ties go to the lowest class; a
    prediction outside [0, numClasses) votes for nothing. A voxel is valid iff the share of ignoreLabel among its labels is
    below maxIgnoreShare (in double) and its majority label is not ignoreLabel. out: None makes a zeroed tensor; a given one
    is ADDED to and returned. The table lives in a zeroed tensor kept per (device, stream, capacity, numClasses), 8 + 8
    numClasses bytes for each of the >= 2 n slots; the op leaves it zeroed. Integer atomics only: the same inputs give the
    same bytes. Nothing is differentiable and nothing is read back."""
    return _voxel_counts_run(*_voxel_counts_args(points, pred, labels, numClasses, batchIds, numClouds, aabbMin, resolution,
                                                 ignoreLabel, maxIgnoreShare, out, dropped))


def _voxel_counts_run(points, pred, labels, numClasses, batchIds, numClouds, aabbMin, res, ignoreLabel, share, out, dropped):
    """voxel_counts behind its checks, over what _voxel_counts_args returns."""
    lib = _lib.load()
    if out is None:
        out = torch.zeros((numClouds, numClasses, 2), dtype=torch.int64, device=points.device)
    n = points.shape[0]
    if n == 0:
        return out
    ws = _voxel_ws(n, numClasses, points.device)
    check(lib.mccnn_voxel_acc_add(ptr(points), ptr(pred), ptr(labels), ptr(batchIds), ptr(aabbMin), n, numClouds, numClasses,
                                  ignoreLabel, res, share, ptr(out), ptr(dropped), ptr(ws), ws.numel(), 1, stream_handle()),
          "voxel_counts")
    return out


# At the end on purpose: MCConvModule imports this module back at ITS end, and with both imports last each module finds the
# other one's names defined whichever of the two is imported first.
from .MCConvModule import _bf16_rows_aligned, _req, _ws  # noqa: E402
