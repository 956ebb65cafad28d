"""The optimiser step as one library op: FusedAdam, Adam with L2 weight decay over all parameters of a network in
ceil(tensors / mccnn_adam_max_tensors()) launches of csrc/adam.hip (C-ABI mccnn_adam_step, include/mccnn.h).

Per element, in float32 (the definition of include/mccnn.h):

    g   = grad_scale * grad                      (skipped when grad_scale == 1)
    g   = weight_decay * p + g                   (skipped when weight_decay == 0; L2 in the gradient, not AdamW)
    m'  = m + (1 - beta1) * (g - m)
    v'  = beta2 * v + ((1 - beta2) * g) * g
    den = sqrt(v') / bc2_sqrt + eps
    p'  = p - step_size * (m' / den)

with the per-tensor scalars computed here, in double, from the tensor's own step count t >= 1 and the betas rounded to float32
(the values the kernel multiplies with), and rounded once to float32:

    form 'torch' (torch.optim.Adam's arithmetic)         step_size = lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t)
    form 'tf'    (tf.train.AdamOptimizer's, the reference's: epsilon outside the bias correction)
                                                         step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t),  bc2_sqrt = 1

With maxGradNorm or skipNonFinite set, one reduction stands in front (mccnn_grad_norm, the same file), with gs = float32(gradScale)
and the live tensors of ALL param groups in record order:

    S       = sum over live tensors and elements of (gs * grad)^2       (float32 products and chunk sums, float64 across chunks)
    norm    = float32(sqrt(S))
    coef    = 1 if max_norm == 0 or norm is not finite, else min(1.0f, max_norm / (norm + 1e-6f))   (clip_grad_norm_'s formula)
    skipped = 1 if skipNonFinite and norm is not finite, else 0;   skips += skipped

and the step runs with grad_scale' = float32(gs * coef) in place of grad_scale, or not at all when skipped == 1. The four values
are a 16-byte record on the device, which the step kernel reads; nothing is read back.

The host side is the point of the op: one persistent array of records (the C struct's layout as a NumPy structured array) for
all parameters, handed to the library by address. A step writes the parameter and gradient pointers, the live flags where
they changed, and the two step scalars as array operations; no ctypes object is built per tensor.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from .MCConvModule import InvalidArgumentError

# mccnn_adam_tensor (include/mccnn.h)
RECORD = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("step_size", "<f4"), ("bc2_sqrt", "<f4"),
                   ("weight_decay", "<f4")])
assert RECORD.itemsize == 48
CHUNK = 4096   # elements one workgroup of the kernel takes (csrc/adam.hip: kAdamChunk)
FORMS = ("torch", "tf")
# mccnn_grad_record (include/mccnn.h) as 0-dim views of its 16 bytes: float32 norm and coef, int32 skipped and skips
GradRecord = collections.namedtuple("GradRecord", ["norm", "coef", "skipped", "skips"])


def _f32(x):
    return float(np.float32(x))


def step_scalars(form, lr, beta1, beta2, t):
    """-> (step_size, bc2_sqrt) of step count(s) t >= 1 in double (NumPy broadcasts over t); the caller rounds to float32.
    beta1, beta2: the values the kernel multiplies with (float32-rounded for the op)."""
    if form not in FORMS:
        raise InvalidArgumentError("FusedAdam: form must be 'torch' or 'tf', got %r" % (form,))
    if type(t) is int:   # (all tensors of a step at the same count: plain floats)
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        return (lr / bc1, math.sqrt(bc2)) if form == "torch" else (lr * math.sqrt(bc2) / bc1, 1.0)
    t = np.asarray(t, dtype=np.float64)
    bc1 = 1.0 - np.power(float(beta1), t)
    bc2 = 1.0 - np.power(float(beta2), t)
    if form == "torch":
        return lr / bc1, np.sqrt(bc2)
    return lr * np.sqrt(bc2) / bc1, np.ones_like(bc2)


def _adam_torch(p, g, m, v, step_size, bc2_sqrt, weight_decay, beta1, beta2, eps, grad_scale):
    """The definition on torch tensors (float32, in place on p, m, v): the CPU route of FusedAdam. Every scalar is a Python
    float holding a float32 value."""
    if grad_scale != 1.0:
        g = g * grad_scale
    if weight_decay != 0.0:
        g = (p * weight_decay).add_(g)
    omb1, omb2 = _f32(np.float32(1.0) - np.float32(beta1)), _f32(np.float32(1.0) - np.float32(beta2))
    m.add_((g - m).mul_(omb1))
    v.mul_(beta2).add_((g * omb2).mul_(g))
    den = v.sqrt().div_(bc2_sqrt).add_(eps)
    p.sub_((m / den).mul_(step_size))


def _grad_norm_host(grads, gs):
    """The norm's definition on the CPU -> float32 norm: float32 products, squares and per-chunk sums, float64 across the chunks
    (a square or a chunk sum beyond float32 is inf, as in the kernel)."""
    total = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for g in grads:
            x = g.detach().reshape(-1).numpy() * np.float32(gs)
            x = x * x
            for a in range(0, len(x), CHUNK):
                total += float(x[a:a + CHUNK].sum(dtype=np.float32))
    return np.float32(math.sqrt(total))   # (inf and NaN pass through)


def clip_coef(norm, max_norm):
    """csrc/grad_clip.h in NumPy float32: norm, max_norm float32 -> float32 coef."""
    norm, max_norm = np.float32(norm), np.float32(max_norm)
    if max_norm == 0 or not np.isfinite(norm):
        return np.float32(1.0)
    with np.errstate(over="ignore"):   # (max_norm / 1e-6 beyond float32 is inf, and the min 1)
        return min(np.float32(1.0), max_norm / (norm + np.float32(1e-6)))


class _Plan:
    """What a step reuses: the flat parameter list, the record array and its address, the step counts."""
    __slots__ = ("params", "slices", "device", "rec", "addr", "numel", "decays", "t", "step_buf", "step_np", "has_state", "all_state",
                 "same_t", "live", "checked", "group_wd", "ws_bytes")


class FusedAdam(torch.optim.Optimizer):
    """Adam with L2 weight decay, one library op per step (see the module's docstring for the arithmetic).

        FusedAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weightDecay=0.0, decayParams=None, form='torch', gradScale=1.0,
                  maxGradNorm=None, skipNonFinite=False)

    params       tensors or param groups. lr, betas, eps, weight_decay and form live in param_groups: a scheduler, or the
                 reference's staircase decay with a floor, assigns group['lr']. lr is a Python float; a tensor raises. Groups
                 with different betas or eps go out as separate library calls, groups that share them share launches.
    decayParams  None: every parameter of a group gets the group's weight_decay (torch's rule). An iterable of parameters:
                 only those do, the others get 0 -- the reference's collection,
                 net.store.get_collection('weight_decay_loss') + net.convBuilder.get_collection('weight_decay_loss'). With
                 weightDecay = c that is the gradient of the reference's l2_regularizer(scale=c) term, c sum(w^2) / 2.
    form         'torch' (default) or 'tf': where epsilon stands relative to the bias correction.
    gradScale    multiplies every gradient as it is loaded (1 / world after GradBucket.allreduce(average=False)).
    maxGradNorm  None, or a finite Python number > 0: the gradients, gradScale included, are scaled so that their norm over ALL
                 param groups is at most this (torch.nn.utils.clip_grad_norm_'s formula), inside the op.
    skipNonFinite  True: a step whose gradient norm is inf or NaN changes nothing of p, exp_avg, exp_avg_sq.

    gradScale, maxGradNorm and skipNonFinite are plain attributes and may be assigned between steps; pickle and deepcopy keep
    them; they stay out of param_groups and state_dict(). With maxGradNorm None and skipNonFinite False a step is the library
    call it was without them. With either set, one mccnn_grad_norm over the whole record array runs first (one norm, whatever
    the groups), then mccnn_adam_step_clipped per group of shared betas and eps: ceil(tensors / 76) + 1 launches more. The
    optimiser owns the partials buffer (it grows when needed) and the 16-byte record (zeroed when created, not pickled).
    grad_record is None before the first such step, afterwards GradRecord(norm, coef, skipped, skips): 0-dim float32 and int32
    views of the record on the parameters' device, rewritten by every such step. The class never reads them back; a training
    loop stacks norm into the read-back it already does for its progress line. skips counts the skipped steps. A gradient with
    |gradScale * grad| above about 1.8e19 overflows its float32 square and reads as non-finite.
    Step counts live on the host and nothing is read back, so a SKIPPED STEP IS STILL COUNTED: state[p]['step'] and the bias
    corrections then run ahead by the number of skips (one skip at t = 100 with beta2 = 0.999 changes sqrt(1 - beta2^t) by
    0.5 %; after a few thousand steps it changes nothing). There is no collective: the norm is that of the gradients this
    optimiser sees. After GradBucket.allreduce those of the all-reduced tensors agree across ranks; ranks whose other gradients
    differ clip differently.

    state[p] holds step (a 0-dim float32 CPU tensor; the steps of all parameters are views of one buffer, so that a step
    counts them with one operation), exp_avg and exp_avg_sq under torch.optim.Adam's names; state_dict()
    and load_state_dict() exchange with torch.optim.Adam in both directions. exp_avg and exp_avg_sq of the parameters that
    meet their first gradient in one step are views of one zeroed buffer each (two launches, once), every view on a 16-byte
    boundary. A parameter whose grad is None is skipped: no state, no step counted. A non-contiguous gradient is made
    contiguous first: one torch launch for that tensor. A sparse gradient, a non-float32 or non-contiguous parameter, a
    non-float32 gradient, or parameters on more than one device raise InvalidArgumentError before anything is launched.

    CUDA parameters go through mccnn_adam_step on torch's current stream, CPU parameters through the same definition in
    torch (_adam_torch). Not covered: AMSGrad, maximize, decoupled decay (AdamW), bf16 parameters, capturable / graph
    capture, device step counts (GradScaler-style exactness of a skipped step)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weightDecay=0.0, decayParams=None, form="torch",
                 gradScale=1.0, maxGradNorm=None, skipNonFinite=False):
        if isinstance(lr, torch.Tensor):
            raise InvalidArgumentError("FusedAdam: lr must be a Python float, not a tensor")
        if not (isinstance(gradScale, (int, float)) and math.isfinite(gradScale)):
            raise InvalidArgumentError("FusedAdam: gradScale must be a finite Python number, got %r" % (gradScale,))
        # (the keys torch.optim.Adam's groups carry, at their off values: a state_dict of this class loads there as it is)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weightDecay, form=form, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        self._check_group(defaults)
        self._check_clip(maxGradNorm, skipNonFinite)
        self._plan = None
        self._decay_ids = None
        self._clip_rec = self._clip_ws = self.grad_record = None
        super().__init__(params, defaults)
        self.gradScale = float(gradScale)
        self.maxGradNorm = maxGradNorm
        self.skipNonFinite = skipNonFinite
        if decayParams is not None:
            decay = list(decayParams)
            own = {id(p) for g in self.param_groups for p in g["params"]}
            if not all(isinstance(p, torch.Tensor) and id(p) in own for p in decay):
                raise InvalidArgumentError("FusedAdam: decayParams holds something that is not among params")
            self._decay_ids = {id(p) for p in decay}

    @staticmethod
    def _check_clip(max_norm, skip):
        """-> the float32 max_norm the library is handed (0: no clipping)."""
        if type(skip) is not bool:
            raise InvalidArgumentError("FusedAdam: skipNonFinite must be a bool, got %r" % (skip,))
        if max_norm is None:
            return 0.0
        ok = isinstance(max_norm, (int, float)) and not isinstance(max_norm, bool) and math.isfinite(max_norm)
        with np.errstate(over="ignore"):
            ok = ok and math.isfinite(_f32(max_norm)) and _f32(max_norm) > 0.0
        if not ok:
            raise InvalidArgumentError("FusedAdam: maxGradNorm must be None or a finite Python number > 0 (in float32), got %r" % (max_norm,))
        return _f32(max_norm)

    @staticmethod
    def _check_group(g):
        lr, eps, wd = g["lr"], g["eps"], g["weight_decay"]
        if isinstance(lr, torch.Tensor):
            raise InvalidArgumentError("FusedAdam: lr must be a Python float, not a tensor")
        b = g["betas"]
        if not (math.isfinite(lr) and lr >= 0.0):
            raise InvalidArgumentError("FusedAdam: invalid lr %r" % (lr,))
        if not (len(b) == 2 and all(isinstance(x, (int, float)) and 0.0 <= x < 1.0 for x in b)):
            raise InvalidArgumentError("FusedAdam: betas must be two numbers in [0, 1), got %r" % (b,))
        if not (math.isfinite(eps) and eps >= 0.0):
            raise InvalidArgumentError("FusedAdam: invalid eps %r" % (eps,))
        if not (math.isfinite(wd) and wd >= 0.0):
            raise InvalidArgumentError("FusedAdam: invalid weight_decay %r" % (wd,))
        if g.get("form", "torch") not in FORMS:
            raise InvalidArgumentError("FusedAdam: form must be 'torch' or 'tf', got %r" % (g.get("form"),))
        if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
            raise InvalidArgumentError("FusedAdam: amsgrad, maximize and decoupled weight decay are not covered")

    def __getstate__(self):
        d = dict(super().__getstate__())
        flat = [p for g in self.param_groups for p in g["params"]]
        d["gradScale"] = self.gradScale
        d["maxGradNorm"] = self.maxGradNorm
        d["skipNonFinite"] = self.skipNonFinite
        d["_decay_index"] = None if self._decay_ids is None else [i for i, p in enumerate(flat) if id(p) in self._decay_ids]
        return d

    def __setstate__(self, state):
        state = dict(state)
        known = "_decay_index" in state   # (load_state_dict comes through here too, with state and param_groups only)
        index = state.pop("_decay_index", None)
        super().__setstate__(state)
        if known:
            flat = [p for g in self.param_groups for p in g["params"]]
            self._decay_ids = None if index is None else {id(flat[i]) for i in index}
        self._plan = None   # (the record array holds addresses and aliases the step counts: rebuilt at the next step)
        for k, v in (("maxGradNorm", None), ("skipNonFinite", False), ("_clip_rec", None), ("_clip_ws", None), ("grad_record", None)):
            self.__dict__.setdefault(k, v)   # (a copy starts with a fresh record; load_state_dict keeps what is there)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def load_state_dict(self, state_dict):
        """Takes a state_dict of this class or of torch.optim.Adam (keys this class adds take their defaults; step counts
        come to the CPU as float32 copies, wherever the other optimiser kept them)."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            self._check_group(g)
        for st in self.state.values():
            if "step" in st:
                s = st["step"]
                st["step"] = (s.detach().to("cpu", torch.float32).reshape(()).clone() if isinstance(s, torch.Tensor)
                              else torch.tensor(float(s), dtype=torch.float32))
        self._plan = None

    # ------------------------------------------------------------------------------------------------------------ the plan
    def _build_plan(self):
        pl = _Plan()
        pl.params, pl.slices = [], []
        for g in self.param_groups:
            a = len(pl.params)
            pl.params.extend(g["params"])
            pl.slices.append(slice(a, len(pl.params)))
        devs = {p.device for p in pl.params}
        if len(devs) > 1:
            raise InvalidArgumentError("FusedAdam: parameters on more than one device (%s)" % ", ".join(sorted(map(str, devs))))
        pl.device = devs.pop() if devs else torch.device("cpu")
        if pl.device.type not in ("cpu", "cuda"):
            raise InvalidArgumentError("FusedAdam: parameters must be CPU or CUDA tensors, got %s" % pl.device)
        for p in pl.params:
            if p.dtype is not torch.float32 or p.layout is not torch.strided:
                raise InvalidArgumentError("FusedAdam: parameters must be dense float32 tensors, got %s" % p.dtype)
            if not p.is_contiguous():
                raise InvalidArgumentError("FusedAdam: parameters must be contiguous")
            if p.numel() >= 1 << 31:
                raise InvalidArgumentError("FusedAdam: a parameter of 2^31 elements or more")
        n = len(pl.params)
        pl.rec = np.zeros(n, dtype=RECORD)
        pl.addr = pl.rec.ctypes.data
        pl.numel = np.array([p.numel() for p in pl.params], dtype=np.int32)
        # the partials of mccnn_grad_norm, 8 bytes per chunk: of ALL tensors, what any set of live ones needs at most
        pl.ws_bytes = 8 * int((-(-pl.numel.astype(np.int64) // CHUNK)).sum())
        ids = self._decay_ids
        pl.decays = np.array([1.0 if ids is None or id(p) in ids else 0.0 for p in pl.params], dtype=np.float64)
        pl.t = np.zeros(n, dtype=np.int64)
        # the step counts of state[p]['step'] are views of ONE CPU buffer: a step adds 1 to all of them with one NumPy
        # operation (torch._foreach_add_ over 44 separate 0-dim CPU tensors costs more than the rest of the host path)
        pl.step_buf = torch.zeros(n, dtype=torch.float32)
        pl.step_np = pl.step_buf.numpy()
        pl.has_state = [False] * n
        for i, p in enumerate(pl.params):
            st = self.state.get(p)
            if st:
                pl.t[i] = int(round(float(st["step"])))
                pl.step_np[i] = pl.t[i]
                st["step"] = pl.step_buf[i]
                pl.has_state[i] = True
                pl.rec["m"][i] = st["exp_avg"].data_ptr()
                pl.rec["v"][i] = st["exp_avg_sq"].data_ptr()
                for k in ("exp_avg", "exp_avg_sq"):
                    if st[k].dtype is not torch.float32 or not st[k].is_contiguous() or st[k].device != p.device:
                        raise InvalidArgumentError("FusedAdam: state %s must be a contiguous float32 tensor on the parameter's device" % k)
        pl.all_state = all(pl.has_state)
        pl.same_t = bool((pl.t == pl.t[0]).all()) if n else True
        pl.live = False          # the previous step's live records (None: all of them; False: no step yet): n is rewritten on a change
        pl.checked = [None] * len(self.param_groups)   # per group: the hyper-parameters last validated, and what follows from them
        pl.group_wd = [None] * len(self.param_groups)
        self._plan = pl
        return pl

    def _new_state(self, pl, fresh):
        """exp_avg and exp_avg_sq of the parameters that meet their first gradient: views of one zeroed buffer each, every
        view on a 16-byte boundary."""
        offs, total = [], 0
        for i in fresh:
            offs.append(total)
            total += (int(pl.numel[i]) + 3) & ~3
        bufs = torch.zeros((2, max(total, 1)), dtype=torch.float32, device=pl.device)
        for i, off in zip(fresh, offs):
            p = pl.params[i]
            k = int(pl.numel[i])
            st = self.state[p]
            st["step"] = pl.step_buf[i]
            st["exp_avg"] = bufs[0, off:off + k].view(p.shape)
            st["exp_avg_sq"] = bufs[1, off:off + k].view(p.shape)
            pl.has_state[i] = True
            pl.rec["m"][i] = st["exp_avg"].data_ptr()
            pl.rec["v"][i] = st["exp_avg_sq"].data_ptr()
        pl.all_state = all(pl.has_state)

    def _group_key(self, pl, k, g):
        """The float32 betas and eps of group k, validated once per set of values."""
        lr = g["lr"]
        now = (lr, g["betas"], g["eps"], g["weight_decay"], g.get("form"), g.get("amsgrad"), g.get("maximize"),
               g.get("decoupled_weight_decay"))
        c = pl.checked[k]
        if type(lr) is not float or c is None or c[0] != now:
            self._check_group(g)
            c = pl.checked[k] = (now, (_f32(g["betas"][0]), _f32(g["betas"][1]), _f32(g["eps"])))
        return c[1]

    # ------------------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        pl = self._plan or self._build_plan()
        params = pl.params
        n = len(params)
        if n == 0:
            return loss
        clip = None   # (max_norm as float32 with 0 for none, skip) when the norm pass runs
        if self.maxGradNorm is not None or self.skipNonFinite is not False:
            clip = (self._check_clip(self.maxGradNorm, self.skipNonFinite), self.skipNonFinite)
        f32, strided = torch.float32, torch.strided
        grads = [p.grad for p in params]
        keep = None
        if not [1 for g in grads if g is None or g.dtype is not f32 or g.layout is not strided or not g.is_contiguous()]:
            live = None   # every parameter has a dense contiguous float32 gradient: no per-tensor Python beyond the pointers
            gp = [g.data_ptr() for g in grads]
        else:
            gp, live, keep = [0] * n, [], {}
            for i, g in enumerate(grads):
                if g is None:
                    continue
                if g.layout is not strided:
                    raise InvalidArgumentError("FusedAdam: sparse gradients are not supported")
                if g.dtype is not f32:
                    raise InvalidArgumentError("FusedAdam: gradients must be float32, got %s" % g.dtype)
                if not g.is_contiguous():
                    g = keep[i] = g.contiguous()
                gp[i] = g.data_ptr()
                live.append(i)
            if not live:
                return loss
            if len(live) == n:
                live = None
        groups = self.param_groups
        keys = [self._group_key(pl, k, g) for k, g in enumerate(groups)]
        if not pl.all_state:
            fresh = [i for i in (range(n) if live is None else live) if not pl.has_state[i]]
            if fresh:
                self._new_state(pl, fresh)
        rec = pl.rec
        rec["p"] = [p.data_ptr() for p in params]
        rec["g"] = gp
        live_t = None if live is None else tuple(live)
        if live_t != pl.live:
            if live is None:
                rec["n"] = pl.numel
            else:
                mask = np.zeros(n, dtype=np.int32)
                mask[live] = 1
                rec["n"] = pl.numel * mask
            pl.live = live_t
        if live is None:
            pl.t += 1
            pl.step_np += 1.0
        else:
            pl.t[live] += 1
            pl.step_np[live] += 1.0
            pl.same_t = False
        t0 = int(pl.t[0]) if pl.same_t else None
        runs = []   # (key, first record, end record): neighbouring groups with the same betas and eps are one run
        for k, (g, sl) in enumerate(zip(groups, pl.slices)):
            if sl.stop == sl.start:
                continue
            key = keys[k]
            ss, bc = step_scalars(g["form"], g["lr"], key[0], key[1], t0 if t0 is not None else np.maximum(pl.t[sl], 1))
            rec["step_size"][sl] = ss
            rec["bc2_sqrt"][sl] = bc
            if pl.group_wd[k] != g["weight_decay"]:
                rec["weight_decay"][sl] = pl.decays[sl] * float(g["weight_decay"])
                pl.group_wd[k] = g["weight_decay"]
            if runs and runs[-1][0] == key and runs[-1][2] == sl.start:
                runs[-1] = (key, runs[-1][1], sl.stop)
            else:
                runs.append((key, sl.start, sl.stop))
        if pl.device.type == "cpu":
            self._step_cpu(pl, runs, grads, keep, clip)
            return loss
        calls = {}
        for key, a, b in runs:
            calls.setdefault(key, []).append((a, b))
        lib = _lib.load()
        cur = _lib._cur_device() if _lib._cur_device is not None else torch.cuda.current_device()
        if cur != pl.device.index:
            with torch.cuda.device(pl.device):
                self._launch(lib, pl, calls, clip)
        else:
            self._launch(lib, pl, calls, clip)
        return loss

    def _record(self, device):
        """The 16-byte record on `device`, zeroed once, and its four views."""
        r = self._clip_rec
        if r is None or r.device != device:
            r = self._clip_rec = torch.zeros(4, dtype=torch.int32, device=device)
            f = r.view(torch.float32)
            self.grad_record = GradRecord(f[0], f[1], r[2], r[3])
        return r

    def _launch(self, lib, pl, calls, clip=None):
        stream = _lib.stream_handle()
        if clip is not None:   # one norm over the records of all groups, left in the record on the device
            rec = self._record(pl.device)
            ws = self._clip_ws
            if ws is None or ws.device != pl.device or ws.numel() * 8 < pl.ws_bytes:
                ws = self._clip_ws = torch.empty(max(pl.ws_bytes // 8, 1), dtype=torch.float64, device=pl.device)
            _lib.check(lib.mccnn_grad_norm(pl.addr, len(pl.rec), self.gradScale, clip[0], int(clip[1]), rec.data_ptr(), ws.data_ptr(),
                                           ws.numel() * 8, stream), "mccnn_grad_norm")
            rp = rec.data_ptr()
        for (b1, b2, eps), spans in calls.items():
            if len(spans) == 1:
                a, b = spans[0]
                addr, count = pl.addr + a * RECORD.itemsize, b - a
            else:   # (groups that share betas and eps but do not stand side by side: their records, copied together)
                tmp = np.concatenate([pl.rec[a:b] for a, b in spans])
                addr, count = tmp.ctypes.data, len(tmp)
            if clip is None:
                _lib.check(lib.mccnn_adam_step(addr, count, b1, b2, eps, self.gradScale, stream), "mccnn_adam_step")
            else:
                _lib.check(lib.mccnn_adam_step_clipped(addr, count, b1, b2, eps, self.gradScale, rp, stream), "mccnn_adam_step_clipped")

    def _step_cpu(self, pl, runs, grads, keep, clip=None):
        rec = pl.rec
        gs = _f32(self.gradScale)
        if clip is not None:   # the same definition, the record as CPU tensors
            live = [keep[i] if keep and i in keep else grads[i] for i in range(len(rec)) if rec["n"][i] > 0]
            norm = _grad_norm_host(live, gs)
            coef = clip_coef(norm, clip[0])
            skipped = int(clip[1] and not np.isfinite(norm))
            r = self._record(pl.device).numpy()
            r.view(np.float32)[:2] = (norm, coef)
            r[2] = skipped
            r[3] += skipped
            if skipped:
                return
            gs = _f32(np.float32(gs) * coef)
        for (b1, b2, eps), a, b in runs:
            for i in range(a, b):
                if rec["n"][i] == 0:
                    continue
                p = pl.params[i]
                st = self.state[p]
                g = keep[i] if keep and i in keep else grads[i]
                _adam_torch(p, g, st["exp_avg"], st["exp_avg_sq"], float(rec["step_size"][i]), float(rec["bc2_sqrt"][i]),
                            float(rec["weight_decay"][i]), b1, b2, eps, gs)
