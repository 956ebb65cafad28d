"""Dense helper layers used between the MC convolutions: the counterpart of the reference's
utils/MCNetworkUtils.py with the same function names, argument orders, variable names and initialisers, on torch.

The reference creates variables through TF's global variable scope (tf.get_variable); here they live in a
VariableStore (the ConvolutionBuilder keeps its own in the same way). Batch normalisation follows
tf.layers.batch_normalization's defaults (momentum 0.99, epsilon 1e-3, gamma/beta) and -- because the batch is sharded
cloud-per-GPU while the reference normalises over the WHOLE batch (utils/MCNetworkUtils.py:140) -- synchronises its
statistics across ranks with one small all-reduce when torch.distributed is initialised (point counts differ per rank,
so sums and counts are reduced, not means).

VariableStore(fused=True) (extension, opt-in): batch norm + ReLU + dropout of a block run as ONE library op
(dense_glue.bn_relu_dropout, csrc/bn_act.hip) where its conditions hold (_fused_glue); everywhere else, and always
with fused off, the code below is what runs. Names, shapes, initialisers and state_dict are the same either way; the
dropout mask of the fused op is counter-based (seed dropSeed_ + dropCalls_), not torch's random stream.

VariableStore(fused=True, fusedSync=True) (extension, opt-in): the one case `fused` leaves to the torch code below -- training
statistics synchronised across the ranks of a process group -- runs as a library op too (dense_glue.bn_relu_dropout_sync:
the op cut in two around one gather of 3c floats per rank, forward and backward). Same names, shapes and state_dict; the
mask of a row is that of its index in the whole batch, so with one dropSeed_ on all ranks the shards drop what a single
process would. fusedLinear leaves that case to the matmul followed by this op.

VariableStore(fused=True, fusedCat=True) (extension, opt-in): batch_norm_RELU_drop_out also takes a list or tuple of 2-D
tensors, meaning their concatenation along axis 1. With both switches on the block reads the segments where they are
(dense_glue.bn_relu_dropout_cat, csrc/bn_act.hip: one op, no torch.cat, one contiguous gradient per segment) where its
conditions hold (_fused_cat: 1 .. 8 float32 contiguous segments on one HIP device, statistics of this process alone);
everywhere else -- the switch off, CPU, bfloat16 segments, statistics across ranks -- the list is torch.cat'ed and takes
the path of a single tensor. Names, shapes, initialisers, state_dict and the dropSeed_ / dropCalls_ counting are the same.

VariableStore(fusedLinear=True) (extension, opt-in): a linear layer with such a block behind it -- conv_1x1 followed by
batch_norm_RELU_drop_out (conv_1x1_batch_norm_RELU_drop_out) and the hidden layers of the MLPs -- runs as ONE library op
(dense_glue.linear_bn_relu_dropout, csrc/linear_bn.hip) where its conditions hold (_fused_linear); everywhere else the
matmul and the block run as before. Names, shapes, initialisers, creation order and state_dict are the same either way,
and a call that drops takes its seed from dropSeed_ / dropCalls_ as the fused glue does: with `fused` on as well, the
masks of a network do not depend on this switch.

VariableStore(fusedLoss=True) (extension, opt-in): the LAST linear of a network and the sparse softmax cross-entropy behind
it -- conv_1x1_softmax_cross_entropy, and the MLPs called with labels -- run as ONE library op
(dense_glue.linear_softmax_xent, csrc/linear_xent.hip) where its conditions hold (_fused_loss): x -> LossHead(loss, pred,
correct, denom, logits), the gradients of x, the weights and the biases from one autograd node. Everywhere else, and always
with the switch off, torch code computes the same definition (_loss_head). Names, shapes, initialisers, creation order and
state_dict are the same either way; without labels every helper returns the logits as before.
The same switch covers the loss of the third task, normal estimation: cosine_distance_loss(pred, target) -> NormalHead(loss,
cosSum, angleSum, denom) runs as ONE library op (dense_glue.cosine_distance_loss, csrc/cosine_loss.hip) where its conditions
hold (_fused_cosine), as torch code of the same definition (_normal_head) everywhere else. And the figure of the second task,
segmentation: segmentation_counts(pred or LossHead, labels, ...) -> int64 [B, C, 3] counts of intersection, union and ground
truth per cloud and class runs as ONE library launch (dense_glue.segmentation_counts, csrc/seg_counts.hip) under the same
switch, as torch code of the same definition (_seg_counts_torch) everywhere else; segmentation_scores and part_iou form the
reference's two IoU figures from the counts. ScanNet's third figure, the voxel accuracy, likewise: voxel_counts(points, pred or
LossHead, labels, ...) -> int64 [B, C, 2] counts of valid voxels whose majority label and majority prediction agree, and of
all valid voxels, as one library op (dense_glue.voxel_counts, csrc/voxel_acc.hip: a device hash table, two launches) under
the same switch, as torch code of the same definition (_voxel_counts_torch) everywhere else; voxel_scores forms the figure.
"""
import collections
import math

import numpy as np
import torch
import torch.distributed as dist

from . import dense_glue
from .MCConvModule import InvalidArgumentError


class VariableStore(torch.nn.Module):
    """name -> torch.nn.Parameter / buffer; tf.get_variable + tf.add_to_collection semantics on a torch.nn.Module, so
    that `parameters()`, `state_dict()`, `.to()`, optimisers and DDP wrappers see the variables under the reference's
    names (`Reduce_1_weights`, `Final_Logits_BN_h1/gamma`, ...). Variables are created on first use (tf.get_variable),
    so load_state_dict() also accepts names that do not exist yet."""

    def __init__(self, device=None, fused=False, fusedLinear=False, fusedSync=False, fusedLoss=False, fusedCat=False):
        super().__init__()
        self.device = device
        self.collections_ = {}
        self.fused_ = bool(fused)   # the dense glue as one library op where it applies (may be reassigned at any time)
        self.fusedLinear_ = bool(fusedLinear)   # linear layer + glue as one library op where it applies (reassignable too)
        self.fusedSync_ = bool(fusedSync)   # with fused_: the glue stays a library op when statistics cross ranks (reassignable)
        self.fusedLoss_ = bool(fusedLoss)   # last linear + softmax cross-entropy as one library op where it applies (reassignable)
        self.fusedCat_ = bool(fusedCat)   # with fused_: the glue over a list of segments reads them in place (reassignable)
        self.syncGroup_ = None      # the process group of those statistics (None: the default group)
        self.dropSeed_ = 0          # a fused call that drops uses the seed (dropSeed_ + dropCalls_) mod 2^32 ...
        self.dropCalls_ = 0         # ... and increments this counter

    @property
    def variables_(self):
        return self._parameters

    @property
    def buffers_(self):
        return self._buffers

    def get_variable(self, name, shape, init, device=None):
        p = self._parameters.get(name)
        if p is None:
            p = torch.nn.Parameter(init(torch.empty(shape, dtype=torch.float32, device=device or self.device)))
            self.register_parameter(name, p)
        elif tuple(p.shape) != tuple(shape):
            raise RuntimeError("variable %s exists with shape %s, requested %s" % (name, tuple(p.shape), shape))
        return p

    def get_buffer(self, name, shape, fill, device=None):
        b = self._buffers.get(name)
        if b is None:
            b = torch.full(shape, float(fill), dtype=torch.float32, device=device or self.device)
            self.register_buffer(name, b)
        return b

    def add_to_collection(self, coll, p):
        lst = self.collections_.setdefault(coll, [])
        if not any(q is p for q in lst):
            lst.append(p)

    def get_collection(self, coll):
        return list(self.collections_.get(coll, []))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # lazily created variables: adopt what is not there yet (also when a parent module's load_state_dict() recurses
        # into this one -- variable names hold no '.', so every key below `prefix` without one is this module's own)
        for k, v in state_dict.items():
            name = k[len(prefix):] if k.startswith(prefix) else None
            if name and "." not in name and name not in self._parameters and name not in self._buffers:
                if name.endswith("/moving_mean") or name.endswith("/moving_variance"):
                    self.register_buffer(name, v.detach().clone())
                else:
                    self.register_parameter(name, torch.nn.Parameter(v.detach().clone()))
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


_DEFAULT_STORE = VariableStore()


def get_default_store():
    return _DEFAULT_STORE


def reset_default_store(device=None):
    global _DEFAULT_STORE
    _DEFAULT_STORE = VariableStore(device)
    return _DEFAULT_STORE


def _fan_avg_uniform(fan_in, fan_out):
    limit = math.sqrt(3.0 / ((fan_in + fan_out) / 2.0))  # variance_scaling_initializer(1.0, 'FAN_AVG', uniform=True)

    def init(t):
        with torch.no_grad():
            t.uniform_(-limit, limit)
        return t
    return init


def _glorot_uniform(fan_in, fan_out):
    # tf.get_variable's default initializer (used for ..._weights2 in MLP_2_hidden, MCNetworkUtils.py:55)
    limit = math.sqrt(6.0 / (fan_in + fan_out))

    def init(t):
        with torch.no_grad():
            t.uniform_(-limit, limit)
        return t
    return init


def _zeros(t):
    with torch.no_grad():
        t.zero_()
    return t


def _ones(t):
    with torch.no_grad():
        t.fill_(1.0)
    return t


def _bn_block(st, name, c, dev):
    """The four variables of a batch-norm block -> (gamma, beta, moving_mean, moving_variance), created on first use in that
    order (the order of the store's state_dict keys)."""
    return (st.get_variable(name + "/gamma", (c,), _ones, dev), st.get_variable(name + "/beta", (c,), _zeros, dev),
            st.get_buffer(name + "/moving_mean", (c,), 0.0, dev), st.get_buffer(name + "/moving_variance", (c,), 1.0, dev))


def _stats_cross_ranks(training, sync):
    """The batch statistics of this call run over the rows of more than one rank."""
    return bool(training and sync and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


def batch_normalization(inputs, training, name, store=None, momentum=0.99, epsilon=1e-3, sync=True):
    """tf.layers.batch_normalization(inputs, training=..., name=...) over axis 0 of an [n, c] tensor."""
    st = store or _DEFAULT_STORE
    c = inputs.shape[1]
    dev = inputs.device
    gamma, beta, mov_mean, mov_var = _bn_block(st, name, c, dev)
    distributed = _stats_cross_ranks(training, sync)
    if training and not distributed and inputs.shape[0] > 1:
        # single process: the fused batch-norm kernels (one forward, one backward launch instead of ~30 element-wise
        # ones; the network is host-bound). Same arithmetic: biased batch variance for the normalisation AND for the
        # moving average, as tf.layers.batch_normalization does (torch's own running_var update would be unbiased).
        with torch.no_grad():
            var, mean = torch.var_mean(inputs, 0, unbiased=False)
            mov_mean.mul_(momentum).add_(mean, alpha=1.0 - momentum)
            mov_var.mul_(momentum).add_(var, alpha=1.0 - momentum)
        return torch.nn.functional.batch_norm(inputs, None, None, gamma, beta, True, 0.0, epsilon)
    if training:
        n = torch.tensor([float(inputs.shape[0])], dtype=torch.float32, device=dev)
        s1 = inputs.sum(0)
        s2 = (inputs * inputs).sum(0)
        if distributed:
            import torch.distributed.nn.functional as dfn
            packed = dfn.all_reduce(torch.cat([s1, s2, n]), op=dist.ReduceOp.SUM)
            s1, s2, n = packed[:c], packed[c:2 * c], packed[2 * c:]
        mean = s1 / n
        var = (s2 / n - mean * mean).clamp_min(0.0)
        with torch.no_grad():
            mov_mean.mul_(momentum).add_(mean.detach(), alpha=1.0 - momentum)
            mov_var.mul_(momentum).add_(var.detach(), alpha=1.0 - momentum)
    else:
        mean, var = mov_mean, mov_var
    return (inputs - mean) * torch.rsqrt(var + epsilon) * gamma + beta


_NATIVE = False   # mccnn_amd.native once the library has loaded; None when it does not


def _fused_native():
    """mccnn_amd.native, whose _X_run functions the gates below hand their checked arguments to -- once the library has
    loaded; None when it does not. Cached."""
    global _NATIVE
    if _NATIVE is False:
        try:
            from . import _lib, native
            _lib.load()
            _NATIVE = native
        except (ImportError, OSError, AttributeError, RuntimeError):
            _NATIVE = None
    return _NATIVE


def _draw_drop_seed(st, keepProb):
    """The seed of a library call that is going to happen -- every decline lies behind it: a call that drops (keepProb: its keep
    probability, None: none, as for every eval call) takes the store's next seed and counts as one of its dropCalls_."""
    if keepProb is None:
        return 0
    seed = (int(st.dropSeed_) + int(st.dropCalls_)) % (1 << 32)
    st.dropCalls_ += 1
    return seed


def _fused_glue(st, inputs, training, name, relu, keepProb=None, momentum=0.99, epsilon=1e-3, sync=True, outDtype=None):
    """drop(act(batch_normalization(inputs))) as one library op, or None where the fused form does not apply (the caller
    then runs the torch code): the store's switch is off, the input is not a contiguous float32 (or bfloat16 with an even
    c) [n, c] tensor on a HIP device, the library does not load, training statistics are synchronised across ranks and
    the store's fusedSync_ is off (with it on, that case takes the op whose statistics run over the rows of all ranks of
    the store's syncGroup_: native.bn_relu_drop_sync), or an eval call wants gradients -- whatever the op's own rule
    (dense_glue._bn_act_args), asked once, refuses. keepProb: the keep probability of a dropout that applies (None: none).
    outDtype: the result's type (None: the input's; torch.float32; torch.bfloat16, which needs an even c as well)."""
    if not getattr(st, "fused_", False):
        return None
    synced = _stats_cross_ranks(training, sync)
    if synced and not getattr(st, "fusedSync_", False):
        return None
    native = _fused_native()
    if native is None or not torch.is_tensor(inputs) or inputs.dim() != 2:   # (the block below is as wide as inputs.shape[1])
        return None
    # residual: the rule is never shown the keepProb of an eval call; this gate has always declined a bad one there too
    if keepProb is not None and not 0.0 < keepProb <= 1.0:
        return None
    gamma, beta, mov_mean, mov_var = _bn_block(st, name, inputs.shape[1], inputs.device)
    group = getattr(st, "syncGroup_", None) if synced else None
    keep = keepProb if training else None
    try:   # (the seed is drawn behind the checks: they see 0 in its place)
        checked = dense_glue._bn_act_args(inputs, gamma, beta, mov_mean, mov_var, keep, 0, outDtype, training=training,
                                          sync=synced, group=group)
    except InvalidArgumentError:
        return None
    seed = _draw_drop_seed(st, keep)
    if synced:
        return native._bn_sync_run(inputs, gamma, beta, mov_mean, mov_var, relu, seed, momentum, epsilon, outDtype, group, *checked)
    return native._bn_act_run(inputs, gamma, beta, mov_mean, mov_var, training, relu, seed, momentum, epsilon, outDtype, *checked)


def _fused_cat(st, segments, training, name, relu, keepProb=None, momentum=0.99, epsilon=1e-3, sync=True, outDtype=None):
    """drop(act(batch_normalization(torch.cat(segments, 1)))) as one library op that reads the segments where they are, or
    None where that form does not apply (the caller then concatenates and goes on as for a single tensor): fused_ or
    fusedCat_ is off, training statistics are synchronised across ranks, the library does not load, or whatever the op's own
    rule (dense_glue._bn_cat_args), asked once, refuses -- more than 8 segments, one that is not a contiguous float32 or bfloat16 2-D
    tensor on a HIP device (the types may differ from segment to segment; the result has torch.cat's: bfloat16 iff every
    segment is), an eval call that wants gradients. The block's variables and the seed of a call that drops are those of
    _fused_glue on the concatenated tensor."""
    if not (getattr(st, "fused_", False) and getattr(st, "fusedCat_", False)) or _stats_cross_ranks(training, sync):
        return None
    native = _fused_native()
    if native is None or not all(torch.is_tensor(x) and x.dim() == 2 for x in segments):
        return None
    # residual: as in _fused_glue
    if keepProb is not None and not 0.0 < keepProb <= 1.0:
        return None
    gamma, beta, mov_mean, mov_var = _bn_block(st, name, sum(x.shape[1] for x in segments), segments[0].device)
    keep = keepProb if training else None
    try:   # (the seed is drawn behind the checks: they see 0 in its place)
        checked = dense_glue._bn_cat_args(segments, gamma, beta, mov_mean, mov_var, keep, 0, outDtype, training=training)
    except InvalidArgumentError:
        return None
    seed = _draw_drop_seed(st, keep)
    return native._bn_cat_run(segments, gamma, beta, mov_mean, mov_var, training, relu, seed, momentum, epsilon, outDtype, *checked)


def _keep_prob(useDropOut, keepProb):
    """The keep probability of a block's dropout as a float, None when the block has none."""
    if not useDropOut or keepProb is None or keepProb is False:
        return None
    return float(keepProb)


def _bn_relu_drop(st, inputs, training, name, useDropOut, keepProb, outDtype=None):
    """relu(batch_normalization(inputs)) [+ dropout]: the fused op where it applies, the torch code otherwise (followed by
    a cast where another type than its result's was asked for)."""
    if getattr(st, "fused_", False):
        y = _fused_glue(st, inputs, training, name, True, _keep_prob(useDropOut, keepProb), outDtype=outDtype)
        if y is not None:
            return y
    y = torch.relu(batch_normalization(inputs, training, name, st))
    if useDropOut:
        y = _dropout(y, keepProb, training)
    if outDtype is not None and y.dtype != outDtype:
        y = y.to(outDtype)
    return y


def _fused_linear(st, inputs, w, b, training, name, keepProb=None, momentum=0.99, epsilon=1e-3, sync=True, outDtype=None):
    """drop(relu(batch_normalization(inputs @ w + b))) as one library op, or None where that form does not apply (the
    caller then runs the matmul and the block as before): the store's switch is off, inputs is not a contiguous float32
    [n, cin] tensor on a HIP device (w and b likewise), the library does not load, training statistics are synchronised
    across ranks, or an eval call wants gradients -- whatever the op's own rule (dense_glue._linear_bn_args), asked once,
    refuses. The variables of the block are created as batch_normalization creates them, and a call that drops takes its seed
    as _fused_glue does."""
    if not getattr(st, "fusedLinear_", False) or _stats_cross_ranks(training, sync):
        return None
    native = _fused_native()
    if native is None or not torch.is_tensor(inputs) or w.dim() != 2:   # (the block below is as wide as w.shape[1])
        return None
    # residual: the rule is never shown the keepProb of an eval call; this gate has always declined a bad one there too
    if keepProb is not None and not 0.0 < keepProb <= 1.0:
        return None
    gamma, beta, mov_mean, mov_var = _bn_block(st, name, w.shape[1], inputs.device)
    keep = keepProb if training else None
    try:   # (the seed is drawn behind the checks: they see 0 in its place)
        checked = dense_glue._linear_bn_args(inputs, w, b, gamma, beta, mov_mean, mov_var, keep, 0, outDtype, training=training)
    except InvalidArgumentError:
        return None
    seed = _draw_drop_seed(st, keep)
    return native._linear_bn_run(inputs, w, b, gamma, beta, mov_mean, mov_var, training, True, seed, momentum, epsilon, outDtype,
                                 *checked)


def _linear_bn_relu_drop(st, inputs, w, b, training, name, useDropOut, keepProb, outDtype=None):
    """_bn_relu_drop(inputs @ w + b): as one library op where the store's fusedLinear_ says so and it applies, the matmul
    and the block otherwise."""
    if getattr(st, "fusedLinear_", False):
        y = _fused_linear(st, inputs, w, b, training, name, _keep_prob(useDropOut, keepProb), outDtype=outDtype)
        if y is not None:
            return y
    return _bn_relu_drop(st, inputs @ w + b, training, name, useDropOut, keepProb, outDtype)


def _dropout(x, keepProb, training=True):
    if keepProb is None or keepProb is False:
        return x
    return torch.nn.functional.dropout(x, p=1.0 - float(keepProb), training=training)


#: What a helper called with labels returns. loss: 0-dim float32, differentiable with respect to the helper's input and the
#: variables of its last linear; pred: int32 [n], the lowest arg-max of every row; correct, denom: 0-dim int32 tensors on
#: the device (no read-back) -- the live rows whose prediction is their label, and D = max(number of live rows, 1), so
#: correct / denom is the accuracy over the live rows; logits: [n, C] without gradient history when asked for, else None.
LossHead = collections.namedtuple("LossHead", "loss pred correct denom logits")


def _fused_loss(st, inputs, w, b, labels, labelWeights, wantLogits):
    """The LossHead of _loss_head as one library op, or None where that form does not apply (the caller then runs the torch
    code): the store's switch is off, inputs is not a contiguous float32 [n, cin] tensor on a HIP device (w and b
    likewise), labels / labelWeights are not contiguous int32 or int64 / float32 tensors of n elements on that device, or the
    library does not load -- whatever the op's own rule (dense_glue._linear_xent_args), asked once, refuses. The op is
    differentiable once: a caller that needs a double backward switches fusedLoss_ off."""
    if not getattr(st, "fusedLoss_", False):
        return None
    native = _fused_native()
    # residual: the rule takes row weights that want a gradient while grad mode is off; this gate never has
    if native is None or getattr(labelWeights, "requires_grad", False):
        return None
    try:
        checked = dense_glue._linear_xent_args(inputs, w, b, labels, labelWeights, wantLogits)
    except InvalidArgumentError:
        return None
    loss, pred, meta, logits = native._linear_xent_run(*checked)
    return LossHead(loss, pred, meta[1], meta[0], logits)


def _loss_head(st, inputs, w, b, labels, labelWeights=None, wantLogits=False):
    """The sparse softmax cross-entropy over z = inputs @ w + b -> LossHead. A row is live iff 0 <= label < C and its weight
    (labelWeights, None: all 1) is not 0; loss = sum over live rows of weight * (logsumexp(z_i) - z[i, label_i]) / D with
    D = max(number of live rows, 1) -- the mean of the reference's ModelNet.py:35-36 without weights, the
    SUM_BY_NONZERO_WEIGHTS of its ScanNet.py:35-37 with them; pred = the lowest arg-max of a row, correct = the live rows
    with pred == label. One library op where the store's fusedLoss_ says so and it applies (_fused_loss), this torch code
    otherwise."""
    if getattr(st, "fusedLoss_", False):
        head = _fused_loss(st, inputs, w, b, labels, labelWeights, wantLogits)
        if head is not None:
            return head
    z = inputs @ w + b
    C = z.shape[1]
    y = labels.reshape(-1).to(torch.int64)
    live = (y >= 0) & (y < C)
    logp = torch.log_softmax(z, 1)
    rows = -logp.gather(1, y.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    if labelWeights is not None:
        rw = labelWeights.reshape(-1).to(z.dtype)
        live = live & (rw != 0)
        rows = rows * rw
    denom = live.sum().clamp_min(1)
    loss = torch.where(live, rows, torch.zeros_like(rows)).sum() / denom
    pred = z.detach().argmax(1)
    correct = (live & (pred == y)).sum()
    return LossHead(loss, pred.to(torch.int32), correct.to(torch.int32), denom.to(torch.int32), z.detach() if wantLogits else None)


#: What cosine_distance_loss returns. loss: 0-dim float32, differentiable with respect to the prediction; cosSum, angleSum:
#: 0-dim float32 tensors, the sums over the live rows of cos_i and of the angle between prediction and target in radians;
#: denom: 0-dim int32, D = max(number of live rows, 1). All on the prediction's device: no read-back until printed. The last
#: three are metrics without gradient history (mean_angle, reference_angle).
NormalHead = collections.namedtuple("NormalHead", "loss cosSum angleSum denom")

_L2_EPS = 1e-12   # tf.nn.l2_normalize's epsilon


def _fused_cosine(st, pred, target, weights):
    """The NormalHead of _normal_head as one library op, or None where that form does not apply (the caller then runs the
    torch code): the store's fusedLoss_ switch is off, pred and target are not float32 [n, c] tensors on one HIP device laid
    out as .contiguous() would leave them (a view that starts anywhere in its buffer is fine), target or the weights want
    a gradient, the weights are not a contiguous float32 [n] / [n, 1] tensor on that device, or the library does not load --
    whatever the op's own rule (dense_glue._cosine_loss_args), asked once, refuses. The op is differentiable once: a caller
    that needs a double backward switches fusedLoss_ off."""
    if not getattr(st, "fusedLoss_", False):
        return None
    native = _fused_native()
    # residual: the rule takes row weights that want a gradient while grad mode is off; this gate never has
    if native is None or getattr(weights, "requires_grad", False):
        return None
    try:
        checked = dense_glue._cosine_loss_args(pred, target, weights)
    except InvalidArgumentError:
        return None
    loss, sums, meta = native._cosine_loss_run(*checked)
    return NormalHead(loss, sums[0], sums[1], meta[0])


def _normal_head(pred, target, weights=None):
    """The cosine-distance loss in torch code -> NormalHead: both rows normalised as tf.nn.l2_normalize does (x / sqrt(max(sum
    x^2, 1e-12)): below the clamp the unit row is LINEAR in x, which is also what its gradient says), cos_i their dot product,
    a row live iff its weight is not 0, loss = sum over live rows of weight * (1 - cos_i) / D with D = max(number of live rows,
    1), and the angle of a row as 2 atan2(|u - v|, |u + v|) (pi / 2 where both lengths are 0)."""
    u = pred / torch.sqrt((pred * pred).sum(1, keepdim=True).clamp_min(_L2_EPS))
    v = target / torch.sqrt((target * target).sum(1, keepdim=True).clamp_min(_L2_EPS))
    cos = (u * v).sum(1)
    rows = 1.0 - cos
    if weights is not None:
        rw = weights.reshape(-1).to(pred.dtype)
        live = rw != 0
        rows = rows * rw
    else:
        live = torch.ones_like(cos, dtype=torch.bool)
    denom = live.sum().clamp_min(1)
    loss = torch.where(live, rows, torch.zeros_like(rows)).sum() / denom
    with torch.no_grad():
        ud, vd = u.detach(), v.detach()
        far = ((ud - vd) ** 2).sum(1).sqrt()
        near = ((ud + vd) ** 2).sum(1).sqrt()
        ang = torch.where((far == 0) & (near == 0), torch.full_like(far, math.pi / 2), 2.0 * torch.atan2(far, near))
        zero = torch.zeros_like(ang)
        cosSum = torch.where(live, cos.detach(), zero).sum()
        angleSum = torch.where(live, ang, zero).sum()
    return NormalHead(loss, cosSum, angleSum, denom.to(torch.int32))


def cosine_distance_loss(pred, target, weights=None, store=None):
    """The loss of normal estimation (the reference's ModelNetNormals.py:34-44: tf.losses.cosine_distance over the two
    l2_normalize'd [n, c] tensors, with its default SUM_BY_NONZERO_WEIGHTS) -> NormalHead(loss, cosSum, angleSum, denom).
    weights: [n] or [n, 1] row weights, None: all 1; a row with weight 0 takes no part, neither in the loss nor in the two
    sums. One library op where the store's fusedLoss_ says so and it applies (_fused_cosine), torch code of the same definition
    (_normal_head) otherwise."""
    st = store or _DEFAULT_STORE
    if getattr(st, "fusedLoss_", False):
        head = _fused_cosine(st, pred, target, weights)
        if head is not None:
            return head
    return _normal_head(pred, target, weights)


def mean_angle(head):
    """The mean over the live rows of the angle between prediction and target, in radians (a 0-dim tensor)."""
    return head.angleSum / head.denom


def reference_angle(head, c):
    """The figure the reference prints as its angle (ModelNetNormals.py): acos of the mean of u * v over all ELEMENTS, i.e.
    acos(cosSum / (c * D)) for rows of c columns -- not the angle of any row; kept for comparing with its logs."""
    return torch.acos(head.cosSum / (c * head.denom))


#: What segmentation_scores returns, the figures of the reference's ScanNet.py:346-386. iou, acc: float64 [C], per class
#: I / U and I / G (1.0 where the denominator is 0); meanIoU, meanAcc: 0-dim float64, their means over the classes other than
#: ignoreLabel; totalAcc: 0-dim float64, sum I / sum G over those classes (1.0 when sum G is 0). All on the counts' device.
SegScores = collections.namedtuple("SegScores", "iou acc meanIoU meanAcc totalAcc")


def _fused_seg_counts(st, pred, labels, numClasses, batchIds, numClouds, weights, ignoreLabel, out):
    """segmentation_counts as one library launch, or None where that form does not apply (the caller then runs the torch
    code): the store's fusedLoss_ switch is off, pred and labels are not contiguous int32 or int64 tensors of n elements on
    one HIP device, batchIds / weights / out are not what dense_glue.segmentation_counts takes, or the library does not
    load -- whatever the op's own rule (dense_glue._seg_counts_args), asked once, refuses."""
    if not getattr(st, "fusedLoss_", False):
        return None
    native = _fused_native()
    # residual: the rule takes ignoreLabel = -2^31; this gate never has
    if native is None or ignoreLabel == -(1 << 31):
        return None
    try:
        checked = dense_glue._seg_counts_args(pred, labels, numClasses, batchIds, numClouds, weights, ignoreLabel, out)
    except InvalidArgumentError:
        return None
    return native._seg_counts_run(*checked)


def _seg_counts_torch(pred, labels, numClasses, batchIds=None, numClouds=1, weights=None, ignoreLabel=-1, out=None):
    """segmentation_counts in torch code, on any device: the flat index of every (cloud, class, count) a row adds to, dead
    rows and absent adds sent to one extra slot behind the table, and ONE integer scatter_add_ over all of them -- no
    boolean indexing and no bincount, which would read a size back. Exact: integer adds in any order."""
    B, C = int(numClouds), int(numClasses)
    if B < 1 or C < 1:
        raise ValueError("segmentation_counts expects numClouds, numClasses >= 1")
    p = pred.detach().reshape(-1).to(torch.int64)
    l = labels.detach().reshape(-1).to(torch.int64)
    n = p.shape[0]
    if l.shape[0] != n:
        raise ValueError("segmentation_counts: labels must have pred's n elements")
    live = (l >= 0) & (l < C)
    if ignoreLabel >= 0:
        live = live & (l != ignoreLabel)
    if weights is not None:
        if weights.numel() != n:
            raise ValueError("segmentation_counts: weights must have pred's n elements")
        live = live & (weights.detach().reshape(-1) != 0)   # (-0.0 is 0; a NaN is not)
    if batchIds is not None:
        if batchIds.numel() != n:
            raise ValueError("segmentation_counts: batchIds must have pred's n elements")
        b = batchIds.detach().reshape(-1).to(torch.int64)
        live = live & (b >= 0) & (b < B)
        row = b * C
    else:
        row = torch.zeros_like(l)
    words = B * C * 3
    if out is None:
        out = torch.zeros((B, C, 3), dtype=torch.int64, device=p.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.int64 and tuple(out.shape) == (B, C, 3) and out.device == p.device):
        raise ValueError("segmentation_counts: out must be an int64 (numClouds, numClasses, 3) tensor on pred's device")
    hit = live & (p == l)
    other = live & ~hit & (p >= 0) & (p < C)
    at = (row + l) * 3
    dump = torch.full_like(l, words)
    idx = torch.cat((torch.where(hit, at, dump), torch.where(live, at + 1, dump), torch.where(live, at + 2, dump),
                     torch.where(other, (row + p) * 3 + 1, dump)))
    flat = torch.zeros(words + 1, dtype=torch.int64, device=p.device)
    flat.scatter_add_(0, idx, torch.ones_like(idx))
    out += flat[:words].view(B, C, 3)
    return out


def segmentation_counts(pred, labels, numClasses, batchIds=None, numClouds=1, weights=None, ignoreLabel=-1, out=None, store=None):
    """The counts behind every IoU of segmentation -> counts, int64 [numClouds, numClasses, 3] on pred's device: per cloud b
    and class c the intersection I (rows with label c and prediction c), the union U (label c or prediction c) and the ground
    truth G (label c), over the live rows. pred: [n] or [n, 1] integer predictions, or a LossHead, whose .pred is taken;
    labels likewise; batchIds: [n] or [n, 1] int32, None: every row is cloud 0; weights: [n] or [n, 1] row weights, None:
    all 1. A row is live iff 0 <= label < numClasses, label != ignoreLabel (< 0: none), its weight is not 0 and 0 <= batch
    id < numClouds (a bad batch id makes a dead row; it is never counted for another cloud). A prediction outside [0,
    numClasses) on a live row is a miss of its label and nothing else. out: None makes a zeroed tensor; a given one is ADDED
    to and returned, so an evaluation accumulates over its batches (ShapeNet.py:291-308 at full batch size, ScanNet.py:306-315
    with ignoreLabel = 0) and reads nothing back until it prints (segmentation_scores, part_iou). One library launch where
    the store's fusedLoss_ says so and it applies (_fused_seg_counts, csrc/seg_counts.hip), torch code of the same definition
    (_seg_counts_torch) otherwise, CPU tensors included; exact either way."""
    if isinstance(pred, LossHead):
        pred = pred.pred
    st = store or _DEFAULT_STORE
    if getattr(st, "fusedLoss_", False):
        counts = _fused_seg_counts(st, pred, labels, numClasses, batchIds, numClouds, weights, ignoreLabel, out)
        if counts is not None:
            return counts
    return _seg_counts_torch(pred, labels, numClasses, batchIds, numClouds, weights, ignoreLabel, out)


def _ratio_or_one(num, den):
    """num / den in float64, 1.0 where den is 0 (the reference's rule for a class nobody has and nobody predicts)."""
    return torch.where(den > 0, num / den.clamp_min(1.0), torch.ones_like(num))


def segmentation_scores(counts, ignoreLabel=-1):
    """The ScanNet rule (ScanNet.py:346-386) over counts [B, C, 3] of segmentation_counts -> SegScores(iou, acc, meanIoU,
    meanAcc, totalAcc). The counts are summed over the clouds, in float64 (exact below 2^53); per class iou = I / U and acc =
    I / G, each 1.0 where its denominator is 0; the means run over the classes other than ignoreLabel (< 0 or >= C: all of
    them; 1.0 when none is left); totalAcc = sum I / sum G over those classes, 1.0 when sum G is 0. Torch ops on the counts'
    device, nothing is read back."""
    c = counts.to(torch.float64).sum(0)
    I, U, G = c[:, 0], c[:, 1], c[:, 2]
    iou, acc = _ratio_or_one(I, U), _ratio_or_one(I, G)
    keep = (torch.arange(c.shape[0], device=c.device) != ignoreLabel).to(torch.float64)
    k = keep.sum()
    meanIoU = _ratio_or_one((iou * keep).sum(), k)
    meanAcc = _ratio_or_one((acc * keep).sum(), k)
    totalAcc = _ratio_or_one((I * keep).sum(), (G * keep).sum())
    return SegScores(iou, acc, meanIoU, meanAcc, totalAcc)


def part_iou(counts, classMask):
    """The ShapeNet rule (ShapeNet.py:294-307) over counts [B, C, 3] of segmentation_counts -> float64 [B]: per cloud the mean
    over its masked classes of I / U, 1.0 where U is 0. classMask: bool [B, C], row b marks the parts of cloud b's category;
    a cloud whose mask is empty gives 1.0. The dataset figure of the reference is the plain mean of this over all models
    (its per-category figure the mean over the models of a category). Torch ops on the counts' device, nothing is read
    back."""
    if tuple(classMask.shape) != tuple(counts.shape[:2]):
        raise ValueError("part_iou: classMask must have shape (numClouds, numClasses)")
    c = counts.to(torch.float64)
    m = classMask.to(device=c.device, dtype=torch.float64)
    return _ratio_or_one((_ratio_or_one(c[:, :, 0], c[:, :, 1]) * m).sum(1), m.sum(1))


#: What voxel_scores returns, ScanNet's voxel accuracy (ScanNet.py:367-384). acc: float64 [C], per class V / G (1.0 where G is
#: 0); meanAcc: 0-dim float64, its mean over the classes other than ignoreLabel. On the counts' device.
VoxelScores = collections.namedtuple("VoxelScores", "acc meanAcc")


def _voxel_res(resolution):
    """resolution as the float32 the definition divides by, as a Python float; None where it is not a finite positive one."""
    try:
        with np.errstate(over="ignore"):
            res = float(np.float32(resolution))
    except (TypeError, ValueError):
        return None
    return res if 0.0 < res < float("inf") else None


def _fused_voxel_counts(st, points, pred, labels, numClasses, batchIds, numClouds, aabbMin, resolution, ignoreLabel, maxIgnoreShare,
                        out, dropped):
    """voxel_counts as one library op, or None where that form does not apply (the caller then runs the torch code): the
    store's fusedLoss_ switch is off, points is not a contiguous float32 [n, 3] tensor on a HIP device, pred and labels are not
    contiguous int32 or int64 tensors of n elements on it, batchIds / aabbMin / out / dropped are not what
    dense_glue.voxel_counts takes, or the library does not load -- whatever the op's own rule (dense_glue._voxel_counts_args),
    asked once, refuses."""
    if not getattr(st, "fusedLoss_", False):
        return None
    native = _fused_native()
    # residual: the rule takes ignoreLabel = -2^31; this gate never has
    if native is None or ignoreLabel == -(1 << 31):
        return None
    try:
        checked = dense_glue._voxel_counts_args(points, pred, labels, numClasses, batchIds, numClouds, aabbMin, resolution,
                                                ignoreLabel, maxIgnoreShare, out, dropped)
    except InvalidArgumentError:
        return None
    return native._voxel_counts_run(*checked)


def _lowest_argmax(h):
    """Per row of the integer table h [m, C] the LOWEST column attaining the row's maximum (0 for an all-zero row)."""
    C = h.shape[1]
    cols = torch.arange(C, device=h.device, dtype=torch.int64).expand_as(h)
    return torch.where(h == h.max(1, keepdim=True).values, cols, torch.full_like(cols, C)).min(1).values


def _voxel_counts_torch(points, pred, labels, numClasses, batchIds=None, numClouds=1, aabbMin=None, resolution=0.05,
                        ignoreLabel=-1, maxIgnoreShare=0.3, out=None, dropped=None):
    """voxel_counts in torch code, on any device, exact: the voxel coordinates as the float32 ceil of a correctly rounded
    float32 quotient (formed in float64 and rounded once more: 53 >= 2 * 24 + 2 bits, so the double rounding is the single
    one), the tuples packed into int64 keys, torch.unique over the keys, integer scatter_add_ histograms, the lowest class of
    every tie and the double quotient of the rule. torch.unique returns a size: this path SYNCHRONISES with the device. It is
    an evaluation path."""
    B, C = int(numClouds), int(numClasses)
    if B < 1 or C < 1 or B > 32768:
        raise ValueError("voxel_counts expects numClasses >= 1 and 1 <= numClouds <= 32768")
    res = _voxel_res(resolution)
    if res is None:
        raise ValueError("voxel_counts expects a finite resolution > 0 (as float32)")
    if not (torch.is_tensor(points) and points.dim() == 2 and points.shape[1] == 3 and points.dtype == torch.float32):
        raise ValueError("voxel_counts: points must be a float32 (n, 3) tensor")
    dev = points.device
    n = points.shape[0]
    pts = points.detach()
    p = pred.detach().reshape(-1).to(torch.int64)
    l = labels.detach().reshape(-1).to(torch.int64)
    if p.shape[0] != n or l.shape[0] != n:
        raise ValueError("voxel_counts: pred and labels must have points' n elements")
    if not (torch.is_tensor(aabbMin) and tuple(aabbMin.shape) == (B, 3) and aabbMin.dtype == torch.float32 and aabbMin.device == dev):
        raise ValueError("voxel_counts: aabbMin must be a float32 (numClouds, 3) tensor on points' device")
    if out is None:
        out = torch.zeros((B, C, 2), dtype=torch.int64, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.int64 and tuple(out.shape) == (B, C, 2) and out.device == dev):
        raise ValueError("voxel_counts: out must be an int64 (numClouds, numClasses, 2) tensor on points' device")
    if dropped is not None and not (torch.is_tensor(dropped) and dropped.dtype == torch.int32 and dropped.numel() == 1
                                    and dropped.device == dev):
        raise ValueError("voxel_counts: dropped must be an int32 tensor of one element on points' device")
    if n == 0:
        return out
    live = (l >= 0) & (l < C)
    if batchIds is not None:
        if batchIds.numel() != n:
            raise ValueError("voxel_counts: batchIds must have points' n elements")
        b = batchIds.detach().reshape(-1).to(torch.int64)
        live = live & (b >= 0) & (b < B)
        b = b.clamp(0, B - 1)                      # (dead rows read some box; they are dead)
    else:
        b = torch.zeros_like(l)
    d = pts - aabbMin.detach()[b]                  # float32, correctly rounded everywhere
    v = torch.ceil((d.to(torch.float64) / res).to(torch.float32))
    inside = ((v >= 0) & (v <= 65535)).all(1)      # (a NaN fails both)
    if dropped is not None:
        dropped += (live & ~inside).sum().to(torch.int32).reshape(dropped.shape)
    live = live & inside
    vi = torch.where(inside.unsqueeze(1), v, torch.zeros_like(v)).to(torch.int64)
    key = torch.where(live, (b << 48) | (vi[:, 0] << 32) | (vi[:, 1] << 16) | vi[:, 2], torch.full_like(b, -1))
    ukey, slot = torch.unique(key, return_inverse=True)     # (sorted: the dead rows' -1, when there is one, is slot 0)
    m = ukey.shape[0]
    dump = torch.full_like(slot, m * C)
    hl = torch.zeros(m * C + 1, dtype=torch.int64, device=dev)
    hp = torch.zeros(m * C + 1, dtype=torch.int64, device=dev)
    one = torch.ones_like(slot)
    hl.scatter_add_(0, torch.where(live, slot * C + l, dump), one)
    hp.scatter_add_(0, torch.where(live & (p >= 0) & (p < C), slot * C + p.clamp(0, C - 1), dump), one)
    hl, hp = hl[:m * C].view(m, C), hp[:m * C].view(m, C)
    s = hl.sum(1)
    ul, up = _lowest_argmax(hl), _lowest_argmax(hp)
    g = hl[:, ignoreLabel] if 0 <= ignoreLabel < C else torch.zeros_like(s)
    valid = (ukey >= 0) & (s > 0) & (g.to(torch.float64) / s.clamp_min(1).to(torch.float64) < float(maxIgnoreShare)) & (ul != ignoreLabel)
    at = (((ukey >> 48) & 0x7fff).clamp(0, B - 1) * C + ul) * 2
    words = B * C * 2
    flat = torch.zeros(words + 1, dtype=torch.int64, device=dev)
    idx = torch.cat((torch.where(valid, at + 1, torch.full_like(at, words)), torch.where(valid & (ul == up), at, torch.full_like(at, words))))
    flat.scatter_add_(0, idx, torch.ones_like(idx))
    out += flat[:words].view(B, C, 2)
    return out


def _box_min(points, batchIds, numClouds):
    """The per-cloud minimum corner the voxel grid starts at. On a HIP device the library's compute_aabb (scaleInv=False:
    bit-exact to the per-cloud minimum); elsewhere torch's amin per cloud. Either way bad batch ids are CLAMPED here."""
    n = points.shape[0]
    if batchIds is None:
        bids = torch.zeros((n, 1), dtype=torch.int32, device=points.device)
    else:
        bids = batchIds.detach().reshape(n, 1).to(torch.int32)
    if points.is_cuda:
        try:
            from . import MCConvModule as M
            return M.compute_aabb(points.detach().contiguous(), bids.contiguous(), int(numClouds), False)[0]
        except (ImportError, OSError, AttributeError):
            pass
    idx = bids.reshape(-1).to(torch.int64).clamp(0, int(numClouds) - 1).unsqueeze(1).expand(n, 3)
    mn = torch.full((int(numClouds), 3), float("inf"), dtype=torch.float32, device=points.device)
    return mn.scatter_reduce(0, idx, points.detach(), "amin", include_self=True)


def voxel_counts(points, pred, labels, numClasses, batchIds=None, numClouds=1, aabbMin=None, resolution=0.05, ignoreLabel=-1,
                 maxIgnoreShare=0.3, out=None, dropped=None, store=None):
    """The counts behind ScanNet's voxel accuracy (ScanNet.py:321-339) -> counts, int64 [numClouds, numClasses, 2] on points'
    device: [b, c, 1] = G, the valid voxels of cloud b whose most frequent label is c; [b, c, 0] = V, those of them whose most
    frequent prediction is c as well. points: float32 [n, 3]; pred: [n] or [n, 1] integer predictions, or a LossHead, whose
    .pred is taken; labels likewise; batchIds: [n] or [n, 1] int32, None: every row is cloud 0. The voxel of a row is the
    integer tuple (b, ceil((p - aabbMin[b]) / resolution)) with float32 arithmetic per axis (resolution is taken as float32;
    the default is the reference's 5 cm). aabbMin: float32 [numClouds, 3]; None takes the per-cloud minimum of the points
    (compute_aabb with scaleInv=False on a HIP device) -- compute_aabb CLAMPS bad batch ids into a cloud's box, so a caller
    whose batch ids may be out of range passes its own box. A row is dead iff its label is outside [0, numClasses), its batch
    id outside [0, numClouds) or one of its coordinates is not finite, below 0 or above 65535 (dropped: optional int32 [1]
    tensor on the device, incremented by the number of rows dropped for their coordinates). A row labelled ignoreLabel (< 0:
    none) is live: it votes and counts in the share. Per voxel the lowest class wins a tie, a prediction outside [0,
    numClasses) votes for nothing, and the voxel is valid iff the share of ignoreLabel among its rows is below maxIgnoreShare
    (in double, the reference's 0.3) and its majority label is not ignoreLabel. Two departures from the reference: it flattens
    the triple in float32 with strides nVoxels, which merges (0, y, z) with (nVoxels_x, y - 1, z) and loses exactness above
    2^24; the tuple here does neither. out: None makes a zeroed tensor; a given one is ADDED to and returned, so an evaluation
    accumulates over its rooms and reads nothing back until it prints (voxel_scores). One library op (two launches) where the
    store's fusedLoss_ says so and it applies (_fused_voxel_counts, csrc/voxel_acc.hip), torch code of the same definition
    (_voxel_counts_torch) otherwise, CPU tensors included; exact either way. The torch code uses torch.unique and therefore
    synchronises with the device."""
    if isinstance(pred, LossHead):
        pred = pred.pred
    st = store or _DEFAULT_STORE
    if aabbMin is None:
        aabbMin = _box_min(points, batchIds, numClouds)
    if getattr(st, "fusedLoss_", False):
        counts = _fused_voxel_counts(st, points, pred, labels, numClasses, batchIds, numClouds, aabbMin, resolution, ignoreLabel,
                                     maxIgnoreShare, out, dropped)
        if counts is not None:
            return counts
    return _voxel_counts_torch(points, pred, labels, numClasses, batchIds, numClouds, aabbMin, resolution, ignoreLabel,
                               maxIgnoreShare, out, dropped)


def voxel_scores(counts, ignoreLabel=-1):
    """ScanNet's voxel accuracy (ScanNet.py:367-384) over counts [B, C, 2] of voxel_counts -> VoxelScores(acc, meanAcc). The
    counts are summed over the clouds, in float64 (exact below 2^53); per class acc = V / G, 1.0 where G is 0; meanAcc is the
    mean over the classes other than ignoreLabel (< 0 or >= C: all of them; 1.0 when none is left). Torch ops on the counts'
    device, nothing is read back."""
    c = counts.to(torch.float64).sum(0)
    acc = _ratio_or_one(c[:, 0], c[:, 1])
    keep = (torch.arange(c.shape[0], device=c.device) != ignoreLabel).to(torch.float64)
    return VoxelScores(acc, _ratio_or_one((acc * keep).sum(), keep.sum()))


def MLP_2_hidden(features, numInputFeatures, hidden1_units, hidden2_units, numOutFeatures, layerName, keepProb,
                 isTraining, useDropOut=False, useInitBN=True, store=None, labels=None, labelWeights=None, wantLogits=False):
    """utils/MCNetworkUtils.py:20-69. labels (extension; None: the logits, as ever): the result is the LossHead of the sparse
    softmax cross-entropy over the last linear (_loss_head; labelWeights: row weights, wantLogits: keep the logits in it)."""
    st = store or _DEFAULT_STORE
    dev = features.device
    if useInitBN:
        y = _fused_glue(st, features, isTraining, layerName + "_BN_Init", False)
        features = y if y is not None else batch_normalization(features, isTraining, layerName + "_BN_Init", st)
    w = st.get_variable(layerName + '_weights1', (numInputFeatures, hidden1_units),
                        _fan_avg_uniform(numInputFeatures, hidden1_units), dev)
    st.add_to_collection('weight_decay_loss', w)
    b = st.get_variable(layerName + '_biases1', (hidden1_units,), _zeros, dev)
    hidden1 = _linear_bn_relu_drop(st, features, w, b, isTraining, layerName + "_BN_h1", useDropOut, keepProb)
    w = st.get_variable(layerName + '_weights2', (hidden1_units, hidden2_units),
                        _glorot_uniform(hidden1_units, hidden2_units), dev)
    st.add_to_collection('weight_decay_loss', w)
    b = st.get_variable(layerName + '_biases2', (hidden2_units,), _zeros, dev)
    hidden2 = _linear_bn_relu_drop(st, hidden1, w, b, isTraining, layerName + "_BN_h2", useDropOut, keepProb)
    w = st.get_variable(layerName + '_weights3', (hidden2_units, numOutFeatures),
                        _fan_avg_uniform(hidden2_units, numOutFeatures), dev)
    st.add_to_collection('weight_decay_loss', w)
    b = st.get_variable(layerName + '_biases3', (numOutFeatures,), _zeros, dev)
    if labels is not None:
        return _loss_head(st, hidden2, w, b, labels, labelWeights, wantLogits)
    return hidden2 @ w + b


def MLP_1_hidden(features, numInputFeatures, hidden_units, numOutFeatures, layerName, keepProb, isTraining,
                 useDropOut=False, store=None, labels=None, labelWeights=None, wantLogits=False):
    """utils/MCNetworkUtils.py:72-106. labels, labelWeights, wantLogits (extension): as in MLP_2_hidden."""
    st = store or _DEFAULT_STORE
    dev = features.device
    w = st.get_variable(layerName + '_weights1', (numInputFeatures, hidden_units),
                        _fan_avg_uniform(numInputFeatures, hidden_units), dev)
    st.add_to_collection('weight_decay_loss', w)
    b = st.get_variable(layerName + '_biases1', (hidden_units,), _zeros, dev)
    hidden = _linear_bn_relu_drop(st, features, w, b, isTraining, layerName + "_BN_h", useDropOut, keepProb)
    w = st.get_variable(layerName + '_weights2', (hidden_units, numOutFeatures),
                        _fan_avg_uniform(hidden_units, numOutFeatures), dev)
    st.add_to_collection('weight_decay_loss', w)
    b = st.get_variable(layerName + '_biases2', (numOutFeatures,), _zeros, dev)
    if labels is not None:
        return _loss_head(st, hidden, w, b, labels, labelWeights, wantLogits)
    return hidden @ w + b


def conv_1x1(layerName, inputs, numInputs, numOutFeatures, store=None):
    """utils/MCNetworkUtils.py:109-126."""
    st = store or _DEFAULT_STORE
    dev = inputs.device
    w = st.get_variable(layerName + '_weights', (numInputs, numOutFeatures), _fan_avg_uniform(numInputs, numOutFeatures), dev)
    st.add_to_collection('weight_decay_loss', w)
    b = st.get_variable(layerName + '_biases', (numOutFeatures,), _zeros, dev)
    return inputs @ w + b


def conv_1x1_softmax_cross_entropy(layerName, inputs, numInputs, numOutFeatures, labels, labelWeights=None, wantLogits=False,
                                   store=None):
    """The sparse softmax cross-entropy (_loss_head) over conv_1x1(layerName, inputs, numInputs, numOutFeatures) (extension)
    -> LossHead: the same variables, created in the same order from the same initialisers; one library op where the store's
    fusedLoss_ is set and the op applies, torch code otherwise."""
    st = store or _DEFAULT_STORE
    dev = inputs.device
    w = st.get_variable(layerName + '_weights', (numInputs, numOutFeatures), _fan_avg_uniform(numInputs, numOutFeatures), dev)
    st.add_to_collection('weight_decay_loss', w)
    b = st.get_variable(layerName + '_biases', (numOutFeatures,), _zeros, dev)
    return _loss_head(st, inputs, w, b, labels, labelWeights, wantLogits)


def batch_norm_RELU_drop_out(layerName, inFeatures, isTraining, usedDropOut, keepProb, store=None, outDtype=None):
    """utils/MCNetworkUtils.py:129-144. outDtype (extension): the result's type, torch.float32 or torch.bfloat16 (None: as
    computed) -- with a fused store the one library op reads float32 or bfloat16 rows and writes either, so the block is
    also the cast between layers that keep different row types. inFeatures (extension): also a list or tuple of 2-D tensors,
    meaning torch.cat(inFeatures, 1) -- one library op over the segments where the store's fused_ and fusedCat_ say so and it
    applies (_fused_cat), the concatenation followed by the path of a single tensor otherwise."""
    st = store or _DEFAULT_STORE
    if isinstance(inFeatures, (list, tuple)):
        if len(inFeatures) >= 1:
            y = _fused_cat(st, inFeatures, isTraining, layerName + "_BN", True, _keep_prob(usedDropOut, keepProb), outDtype=outDtype)
            if y is not None:
                return y
        inFeatures = torch.cat(list(inFeatures), 1)
    return _bn_relu_drop(st, inFeatures, isTraining, layerName + "_BN", usedDropOut, keepProb, outDtype)


def conv_1x1_batch_norm_RELU_drop_out(layerName, bnLayerName, inputs, numInputs, numOutFeatures, isTraining, usedDropOut,
                                      keepProb, store=None, outDtype=None):
    """batch_norm_RELU_drop_out(bnLayerName, conv_1x1(layerName, inputs, numInputs, numOutFeatures), isTraining,
    usedDropOut, keepProb, outDtype=outDtype) (extension): the same variables, created in the same order from the same
    initialisers; one library op where the store's fusedLinear_ is set and the op applies, the two helpers otherwise."""
    st = store or _DEFAULT_STORE
    if getattr(st, "fusedLinear_", False):
        dev = inputs.device
        w = st.get_variable(layerName + '_weights', (numInputs, numOutFeatures), _fan_avg_uniform(numInputs, numOutFeatures), dev)
        st.add_to_collection('weight_decay_loss', w)
        b = st.get_variable(layerName + '_biases', (numOutFeatures,), _zeros, dev)
        y = _fused_linear(st, inputs, w, b, isTraining, bnLayerName + "_BN", _keep_prob(usedDropOut, keepProb), outDtype=outDtype)
        if y is not None:
            return y
    return batch_norm_RELU_drop_out(bnLayerName, conv_1x1(layerName, inputs, numInputs, numOutFeatures, st), isTraining,
                                    usedDropOut, keepProb, st, outDtype)
