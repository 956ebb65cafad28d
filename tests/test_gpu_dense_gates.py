"""The gates of MCNetworkUtils on the GPU, over the tables of tests/test_dense_gates_cpu.py moved to the device (n = 6 rows, c =
4, cin = 3, 4 classes, 2 clouds; bfloat16 rows at c = 6 and, refused, at c = 5): a good call through a gate is the call of
mccnn_amd.native byte for byte and launch for launch, a bad one is declined before anything is launched and the helper then
gives the torch path's result exactly, what the parent's gates declined beyond the ops' rules stays declined, and the rule of
an op runs once per fused helper call. Every declined call ends in Python."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_dense_gates_cpu as T  # noqa: E402

DEV = "cuda:0"
SEVEN = T.OPS[:1] + ("bn_sync",) + T.OPS[1:]
LEAVES = {"bn_act": ("x", "gamma", "beta"), "linear_bn": ("x", "w", "b", "gamma", "beta"), "linear_xent": ("x", "w", "b"),
          "cosine_loss": ("pred",)}
RULES = {"bn_act": "_bn_act_args", "bn_sync": "_bn_act_args"}   # (every other op: _<op>_args)


def _table(op):
    return "bn_act" if op == "bn_sync" else op


def _launches():
    from mccnn_amd import _lib
    return _lib.load().mccnn_debug_launch_count()


def _cross_ranks(monkeypatch):
    """The statistics of a training call count as crossing ranks (no process group: this process alone is the group)."""
    import mccnn_amd.MCNetworkUtils as U
    monkeypatch.setattr(U, "_stats_cross_ranks", lambda training, sync: bool(training and sync))


def _native(op, a):
    """The call of mccnn_amd.native a gate stands for, its result in the order of the gate's."""
    from mccnn_amd import native
    if op in ("bn_act", "bn_sync", "linear_bn"):
        keep = a["keepProb"] if a["training"] else None
        seed = 0 if keep is None else a["seed"]
        cols = (a["gamma"], a["beta"], a["movingMean"], a["movingVar"])
        if op == "bn_sync":
            return native.bn_relu_drop_sync(a["x"], *cols, True, keep, seed, 0.99, 1e-3, a["outDtype"], None)
        if op == "bn_act":
            return native.bn_relu_drop(a["x"], *cols, a["training"], True, keep, seed, 0.99, 1e-3, a["outDtype"])
        return native.linear_bn_relu_drop(a["x"], a["w"], a["b"], *cols, a["training"], True, keep, seed, 0.99, 1e-3, a["outDtype"])
    if op == "linear_xent":
        loss, pred, meta, logits = native.linear_softmax_xent(*a.values())
        return loss, pred, meta[1], meta[0], logits
    if op == "cosine_loss":
        loss, sums, meta = native.cosine_distance_loss(*a.values())
        return loss, sums[0], sums[1], meta[0]
    return getattr(native, {"seg_counts": "segmentation_counts"}.get(op, op))(*a.values())


def _run(op, a, via):
    """Forward (and backward where the op has one) of entry `a` through the gate or through native -> (every tensor that
    comes of it, library launches)."""
    import torch
    st, a = T.store_for(_table(op), a, fusedSync=op == "bn_sync")
    st.dropSeed_ = a.get("seed", 0)
    training = a.get("training", True)
    leaves = [a[k].requires_grad_(True) for k in LEAVES.get(_table(op), ())] if training else []
    before = _launches()
    with torch.set_grad_enabled(bool(training)):
        out = T.gate(_table(op), st, a) if via == "gate" else _native(op, a)
    assert out is not None
    outs = [out] if torch.is_tensor(out) else list(out)
    if leaves:
        y = outs[0]
        y.backward((torch.arange(y.numel(), device=y.device, dtype=torch.float32).reshape(y.shape) % 7 - 3).to(y.dtype))
    torch.cuda.synchronize()
    assert all(t.grad is not None for t in leaves)
    return outs + [t.grad for t in leaves] + list(st._buffers.values()), _launches() - before


GOOD = [(op, kind, i) for op in SEVEN for kind, i, a in T.entries(_table(op)) if kind in ("good", "fine")
        and not (op == "bn_sync" and not a["training"])]
BAD = [(op, kind, i) for op in T.OPS for kind, i, _ in T.entries(op) if kind in ("bad", "huge")]


def _pick(op, kind, i):
    return next(a for k, j, a in T.entries(_table(op), DEV) if (k, j) == (kind, i))


@pytest.mark.parametrize("op,kind,i", GOOD, ids=["%s-%s%d" % c for c in GOOD])
def test_a_good_call_through_the_gate_is_the_native_call(mc, monkeypatch, op, kind, i):
    """(a) The same bytes -- results, gradients, moving statistics -- and the same number of library launches."""
    if op == "bn_sync":
        _cross_ranks(monkeypatch)
    got, launched = _run(op, _pick(op, kind, i), "gate")
    want, launches = _run(op, _pick(op, kind, i), "native")
    print(op, kind, i, "launches", launched, launches)
    assert launched == launches > 0
    assert T.same(("ok", got), ("ok", want))


@pytest.mark.parametrize("op,kind,i", BAD, ids=["%s-%s%d" % c for c in BAD])
def test_a_bad_call_is_declined_before_any_launch(mc, op, kind, i):
    """(b) Every bad entry on the device: None, nothing launched, no seed drawn; the helper is the torch path exactly."""
    st, a = T.store_for(op, _pick(op, kind, i))
    before = _launches()
    assert T.gate(op, st, a) is None
    assert _launches() == before and st.dropCalls_ == 0
    if kind == "huge":
        return
    res = []
    for on in (False, True):
        st, a = T.store_for(op, _pick(op, kind, i), on)
        res.append((T.outcome(lambda: T.helper(op, st, a)), T.state(st), st.dropCalls_))
    assert T.same(res[0][0], res[1][0]) and T.same_state(res[0][1], res[1][1]) and res[0][2] == res[1][2] == 0


def test_what_the_parent_declined_beyond_the_rules_stays_on_the_torch_path(mc):
    """(c) Row weights that want a gradient under no_grad (the loss and the cosine gate), ignoreLabel = -2^31 (the two count
    gates): the rule takes them, the gate does not -- and takes the same call without them."""
    import torch
    import mccnn_amd.dense_glue as G
    for op, kw, nograd in (("linear_xent", dict(weights=torch.ones(6, device=DEV, requires_grad=True)), True),
                           ("cosine_loss", dict(weights=torch.ones(6, device=DEV, requires_grad=True)), True),
                           ("seg_counts", dict(ignoreLabel=-2 ** 31), False), ("voxel_counts", dict(ignoreLabel=-2 ** 31), False)):
        with torch.set_grad_enabled(not nograd):
            st, a = T.store_for(op, dict(_pick(op, "good", 0), **kw))
            before = _launches()
            assert T.gate(op, st, a) is None and _launches() == before
            assert T.rule(op, a, G) is not None                              # (the op itself would run it)
            st, a = T.store_for(op, _pick(op, "good", 0))
            assert T.gate(op, st, a) is not None and _launches() > before


@pytest.mark.parametrize("op", SEVEN)
def test_the_rule_runs_once_per_fused_helper_call(mc, monkeypatch, op):
    """(d) A counter on dense_glue._X_args: one evaluation per helper call that takes the library op."""
    import mccnn_amd.dense_glue as G
    if op == "bn_sync":
        _cross_ranks(monkeypatch)
    name = RULES.get(op, "_%s_args" % op)
    rule, calls = getattr(G, name), []
    monkeypatch.setattr(G, name, lambda *a, **k: calls.append(1) or rule(*a, **k))
    st, a = T.store_for(_table(op), _pick(op, "good", 0), fusedSync=op == "bn_sync")
    before = _launches()
    assert T.helper(_table(op), st, a) is not None
    assert _launches() > before and len(calls) == 1
