"""The gates of MCNetworkUtils (_fused_glue, _fused_linear, _fused_loss, _fused_cosine, _fused_seg_counts, _fused_voxel_counts)
without a GPU: each asks its op's own rule (dense_glue._X_args) and nothing else, so on CPU tensors, with the switch on, every
entry of the bad-argument tables of the ops' CPU tests -- and a good call -- is declined: None, no launch, no seed drawn, and
the helper gives the torch path's result exactly.

tables(dev) holds those entries at the sizes tests/test_gpu_dense_gates.py runs them at on the device (n = 6 rows, c = 4, cin =
3, 4 classes, 2 clouds; bfloat16 rows at c = 6 and, refused, at c = 5): per op (good, bad, fine, ruleOnly) -- the arguments of
the op's rule in order, the overrides the rule refuses on any device, those it refuses for the CPU tensor alone, and those that
are bad only in an argument a gate never passes on (the seed, which it draws itself). HUGE marks the one entry the torch path
would answer with a 25 GB table: it goes to the rule and the gate, not to the helper."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OPS = ("bn_act", "linear_bn", "linear_xent", "cosine_loss", "seg_counts", "voxel_counts")


def tables(dev="cpu"):
    g = torch.Generator().manual_seed(5)
    bf, f16, f64, i64 = torch.bfloat16, torch.float16, torch.float64, torch.int64
    r = lambda *s, dtype=torch.float32: (torch.randn(*s, generator=g) * 2 + 0.5).to(dtype).to(dev)  # noqa: E731
    i32 = lambda *s, hi=4: torch.randint(0, hi, s, generator=g).to(torch.int32).to(dev)  # noqa: E731
    col = lambda c: dict(gamma=r(c), beta=r(c), movingMean=r(c), movingVar=r(c).abs() + 0.5)  # noqa: E731
    cnt = lambda *s: torch.zeros(*s, dtype=i64, device=dev)  # noqa: E731
    t = {}
    # tests/test_bn_act_cpu.py, tests/test_bn_act_rows_cpu.py
    t["bn_act"] = (dict(x=r(6, 4), **col(4), training=True, keepProb=0.5, seed=1, outDtype=None),
                   [dict(x=r(6, 4, dtype=f64)), dict(x=r(4, 6).t()), dict(gamma=r(4, dtype=f64)), dict(movingVar=(r(8).abs() + 0.5)[::2]),
                    dict(keepProb=0.0), dict(keepProb=1.5), dict(keepProb=-0.1), dict(keepProb=float("nan")),
                    dict(x=r(6, 5, dtype=bf), **col(5)), dict(x=r(6, 5), **col(5), outDtype=bf), dict(outDtype=f16), dict(outDtype=f64),
                    dict(x=r(6, 4, dtype=bf), outDtype=f16), dict(x=r(6, 4, dtype=f16)), dict(x=r(6, 4, dtype=bf), gamma=r(4, dtype=bf)),
                    dict(x=r(6, 4, dtype=bf), beta=r(4, dtype=bf))],
                   [dict(), dict(x=r(6, 6, dtype=bf), **col(6), outDtype=torch.float32), dict(x=r(6, 6), **col(6), outDtype=bf),
                    dict(training=False, keepProb=None)],
                   [dict(seed=-1), dict(seed=1 << 32), dict(seed=0.5)])
    # tests/test_linear_bn_cpu.py
    t["linear_bn"] = (dict(x=r(6, 3), w=r(3, 4), b=r(4), **col(4), training=True, keepProb=0.5, seed=1, outDtype=None),
                      [dict(x=r(6, 3, dtype=f64)), dict(x=r(3, 6).t()), dict(w=r(5, 4)), dict(w=r(3, 4, dtype=f64)), dict(b=r(3)),
                       dict(gamma=r(4, dtype=f64)), dict(movingVar=(r(8).abs() + 0.5)[::2]), dict(keepProb=0.0), dict(keepProb=1.5),
                       dict(outDtype=f16), dict(x=r(6, 3, dtype=bf)), dict(w=r(3, 5), b=r(5), **col(5), outDtype=bf)],
                      [dict(), dict(w=r(3, 6), b=r(6), **col(6), outDtype=bf), dict(training=False, keepProb=None)],
                      [dict(seed=-1), dict(seed=1 << 32)])
    # tests/test_linear_xent_cpu.py
    t["linear_xent"] = (dict(x=r(6, 3), w=r(3, 4), b=r(4), labels=i32(6), weights=None, wantLogits=False),
                        [dict(x=r(6, 3, dtype=f64)), dict(w=r(3, 4, dtype=f64)), dict(x=r(3, 6).t()), dict(w=r(5, 4)), dict(x=r(6)),
                         dict(b=r(3)), dict(b=r(4, dtype=f64)), dict(labels=r(6)), dict(labels=[0] * 6), dict(labels=i32(5)),
                         dict(labels=i32(1, 6).to(i64)), dict(labels=i32(12)[::2]), dict(weights=r(6, dtype=f64)), dict(weights=r(7)),
                         dict(weights=r(12)[::2]), dict(weights=r(6).requires_grad_(True))],
                        [dict(), dict(labels=i32(6, 1).to(i64), weights=r(6), wantLogits=True)], [])
    # tests/test_cosine_loss_cpu.py
    t["cosine_loss"] = (dict(pred=r(6, 3), target=r(6, 3), weights=None),
                        [dict(pred=r(6, 3, dtype=f64)), dict(target=r(6, 3, dtype=f64)), dict(pred=[0.0] * 6), dict(pred=r(6)),
                         dict(target=r(5, 3)), dict(pred=r(0, 3), target=r(0, 3)), dict(pred=r(3, 6).t()), dict(target=r(6, 6)[:, :3]),
                         dict(target=r(6, 3).requires_grad_(True)), dict(weights=r(6, dtype=f64)), dict(weights=r(7)),
                         dict(weights=r(1, 6)), dict(weights=r(12)[::2]), dict(weights=r(6).requires_grad_(True))],
                        [dict(), dict(weights=r(6, 1))], [])
    # tests/test_seg_counts_cpu.py
    t["seg_counts"] = (dict(pred=i32(6), labels=i32(6, 1), numClasses=4, batchIds=None, numClouds=1, weights=None, ignoreLabel=-1, out=None),
                       [dict(pred=r(6)), dict(pred=[0] * 6), dict(pred=i32(6, 2)), dict(pred=i32(2, 3, 1)), dict(pred=i32(12)[::2]),
                        dict(labels=r(6)), dict(labels=i32(5)), dict(labels=i32(12)[::2]), dict(numClasses=0), dict(numClasses=4.0),
                        dict(numClouds=0), dict(numClouds=True), dict(numClouds=1 << 20, numClasses=1 << 10, HUGE=True), dict(ignoreLabel=1.5),
                        dict(ignoreLabel=1 << 31), dict(batchIds=i32(6).to(i64)), dict(batchIds=i32(7)), dict(batchIds=i32(12)[::2]),
                        dict(weights=r(6, dtype=f64)), dict(weights=r(1, 6)), dict(weights=r(12)[::2]),
                        dict(weights=r(6).requires_grad_(True)), dict(out=r(1, 4, 3)), dict(out=cnt(1, 4, 2)),
                        dict(out=cnt(1, 4, 6)[:, :, ::2]), dict(numClouds=2, out=cnt(1, 4, 3))],
                       [dict(), dict(pred=i32(6, 1).to(i64), batchIds=i32(6, 1, hi=2), weights=r(6, 1), numClouds=2, out=cnt(2, 4, 3))], [])
    # tests/test_voxel_acc_cpu.py
    pts = lambda n, k=3, dtype=torch.float32: (torch.rand(n, k, generator=g) * 0.4).to(dtype).to(dev)  # noqa: E731
    t["voxel_counts"] = (dict(points=pts(6), pred=i32(6), labels=i32(6, 1), numClasses=4, batchIds=None, numClouds=1,
                              aabbMin=torch.zeros(1, 3, device=dev), resolution=0.05, ignoreLabel=-1, maxIgnoreShare=0.3, out=None,
                              dropped=None),
                         [dict(points=pts(6, dtype=f64)), dict(points=[0.0] * 6), dict(points=pts(6, 2)), dict(points=pts(12)[::2]),
                          dict(pred=r(6)), dict(pred=i32(6, 2)), dict(pred=i32(12)[::2]), dict(labels=r(6)), dict(labels=i32(5)),
                          dict(labels=i32(12)[::2]), dict(numClasses=0), dict(numClasses=4.0), dict(numClouds=0), dict(numClouds=True),
                          dict(numClouds=32769, aabbMin=torch.zeros(32769, 3, device=dev)), dict(ignoreLabel=1.5),
                          dict(ignoreLabel=1 << 31), dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=float("nan")),
                          dict(resolution=1e39), dict(resolution="5cm"), dict(maxIgnoreShare=None), dict(batchIds=i32(6).to(i64)),
                          dict(batchIds=i32(7)), dict(batchIds=i32(12)[::2]), dict(aabbMin=None),
                          dict(aabbMin=torch.zeros(2, 3, device=dev)), dict(aabbMin=torch.zeros(1, 3, dtype=f64, device=dev)),
                          dict(out=r(1, 4, 2)), dict(out=cnt(1, 4, 3)), dict(out=cnt(1, 4, 4)[:, :, ::2]),
                          dict(dropped=cnt(1)), dict(dropped=i32(2))],
                         [dict(), dict(pred=i32(6, 1).to(i64), batchIds=i32(6, 1, hi=2), numClouds=2, aabbMin=torch.zeros(2, 3, device=dev),
                               out=cnt(2, 4, 2), dropped=torch.zeros(1, dtype=torch.int32, device=dev), resolution=np.float32(0.05))], [])
    return t


def entries(op, dev="cpu"):
    """[(kind, index, arguments)] of table `op`: the good call and every override applied to it."""
    good, bad, fine, ruleOnly = tables(dev)[op]
    out = [("good", 0, good)]
    for kind, lst in (("bad", bad), ("fine", fine), ("ruleOnly", ruleOnly)):
        out += [("huge" if kw.pop("HUGE", False) else kind, i, dict(good, **kw)) for i, kw in enumerate(lst)]
    return out


SWITCH = {"bn_act": "fused", "linear_bn": "fusedLinear"}   # (every other op: fusedLoss)
BLOCK = (("w", "R_weights"), ("b", "R_biases"), ("gamma", "R_Out_BN/gamma"), ("beta", "R_Out_BN/beta"))


def store_for(op, a, on=True, **more):
    """-> (a VariableStore with op's switch `on` that holds a's per-column tensors under the names the helpers look them up
    by, a with those tensors replaced by the store's)."""
    import mccnn_amd.MCNetworkUtils as U
    dev = next(v.device for v in a.values() if torch.is_tensor(v))
    st = U.VariableStore(dev, **dict({SWITCH.get(op, "fusedLoss"): on}, **more))
    a = dict(a)
    for key, name in BLOCK:
        if key in a:
            st.register_parameter(name, torch.nn.Parameter(a[key]))
            a[key] = st.variables_[name]
    for key, name in (("movingMean", "R_Out_BN/moving_mean"), ("movingVar", "R_Out_BN/moving_variance")):
        if key in a:
            st.register_buffer(name, a[key])
    return st, a


def rule(op, a, G=None):
    """The op's argument rule over `a`."""
    import mccnn_amd.dense_glue as G_
    G = G or G_
    if op == "bn_act":
        return G._bn_act_args(a["x"], a["gamma"], a["beta"], a["movingMean"], a["movingVar"], a["keepProb"], a["seed"], a["outDtype"],
                              training=a["training"])
    if op == "linear_bn":
        return G._linear_bn_args(a["x"], a["w"], a["b"], a["gamma"], a["beta"], a["movingMean"], a["movingVar"], a["keepProb"],
                                 a["seed"], a["outDtype"], training=a["training"])
    return getattr(G, "_%s_args" % op)(*a.values())


def gate(op, st, a, U=None):
    """The op's gate over `a` and the store `st` of store_for."""
    import mccnn_amd.MCNetworkUtils as U_
    U = U or U_
    if op == "bn_act":
        return U._fused_glue(st, a["x"], a["training"], "R_Out_BN", True, a["keepProb"], outDtype=a["outDtype"])
    if op == "linear_bn":
        return U._fused_linear(st, a["x"], a["w"], a["b"], a["training"], "R_Out_BN", a["keepProb"], outDtype=a["outDtype"])
    if op == "linear_xent":
        return U._fused_loss(st, *a.values())
    if op == "cosine_loss":
        return U._fused_cosine(st, *a.values())
    return getattr(U, "_fused_" + op)(st, *a.values())


def helper(op, st, a):
    """The public helper above the gate over `a` and the store `st` of store_for."""
    import mccnn_amd.MCNetworkUtils as U
    drop = a.get("keepProb") is not None
    if op == "bn_act":
        return U.batch_norm_RELU_drop_out("R_Out", a["x"], a["training"], drop, a["keepProb"], st, a["outDtype"])
    if op == "linear_bn":
        return U.conv_1x1_batch_norm_RELU_drop_out("R", "R_Out", a["x"], a["w"].shape[0], a["w"].shape[1], a["training"], drop,
                                                   a["keepProb"], st, a["outDtype"])
    if op == "linear_xent":
        return U.conv_1x1_softmax_cross_entropy("R", a["x"], a["w"].shape[0], a["w"].shape[1], a["labels"], a["weights"],
                                                a["wantLogits"], st)
    return getattr(U, {"cosine_loss": "cosine_distance_loss", "seg_counts": "segmentation_counts"}.get(op, op))(*a.values(), store=st)


def outcome(f):
    """("ok", the tensors f returns) or ("raised", the exception's type)."""
    torch.manual_seed(3)   # (torch's dropout)
    try:
        res = f()
    except Exception as err:   # noqa: BLE001 -- whatever the torch code makes of a bad argument, both stores must make it
        return "raised", type(err)
    return "ok", [res] if torch.is_tensor(res) else list(res)


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same(a, b):
    """Two outcomes agree: the same exception type, or the same tensors byte for byte (a NaN equals itself)."""
    if a[0] != b[0] or a[0] == "raised":
        return a == b
    return len(a[1]) == len(b[1]) and all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape
                                                                         and torch.equal(_bytes(x), _bytes(y)))
                                          for x, y in zip(a[1], b[1]))


def state(st):
    return [(k, v.detach().clone()) for k, v in st.state_dict().items()]


def same_state(s0, s1):
    return [k for k, _ in s0] == [k for k, _ in s1] and all(torch.equal(a, b) for (_, a), (_, b) in zip(s0, s1))


CASES = [(op, kind, i) for op in OPS for kind, i, _ in entries(op)]


@pytest.mark.parametrize("op,kind,i", CASES, ids=["%s-%s%d" % c for c in CASES])
def test_a_gate_declines_cpu_tensors_and_the_helper_is_the_torch_path(op, kind, i):
    """Every entry on CPU tensors with the switch on: the rule refuses it, the gate returns None without a launch or a seed, it
    creates no variable the torch path would not create, and the helper gives what it gives with the switch off."""
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib
    lib = _lib.load()
    pick = lambda: next(a for k, j, a in entries(op) if (k, j) == (kind, i))  # noqa: E731 -- (a fresh copy per use)
    before = lib.mccnn_debug_launch_count()
    with pytest.raises(M.InvalidArgumentError):
        rule(op, pick())
    if kind == "ruleOnly":
        assert lib.mccnn_debug_launch_count() == before
        return
    st, a = store_for(op, pick())
    assert gate(op, st, a) is None
    assert st.dropCalls_ == 0 and lib.mccnn_debug_launch_count() == before
    if kind == "huge":
        return
    res = []
    for on in (False, True):
        st, a = store_for(op, pick(), on)
        res.append((outcome(lambda: helper(op, st, a)), state(st), st.dropCalls_))
    assert same(res[0][0], res[1][0]) and same_state(res[0][1], res[1][1]) and res[0][2] == res[1][2] == 0
    assert lib.mccnn_debug_launch_count() == before
    if kind in ("good", "fine"):
        assert res[0][0][0] == "ok"


def test_each_gate_asks_its_ops_own_rule():
    import mccnn_amd.MCNetworkUtils as U
    import mccnn_amd.dense_glue as G
    from mccnn_amd import native
    for name, args, runs in (("_fused_glue", "_bn_act_args", ("_bn_act_run", "_bn_sync_run")), ("_fused_linear", "_linear_bn_args", ("_linear_bn_run",)),
                             ("_fused_loss", "_linear_xent_args", ("_linear_xent_run",)), ("_fused_cosine", "_cosine_loss_args", ("_cosine_loss_run",)),
                             ("_fused_seg_counts", "_seg_counts_args", ("_seg_counts_run",)),
                             ("_fused_voxel_counts", "_voxel_counts_args", ("_voxel_counts_run",))):
        src = inspect.getsource(getattr(U, name))
        assert src.count("dense_glue.%s(" % args) == 1 and "except InvalidArgumentError" in src, name
        for run in runs:
            assert "native.%s(" % run in src and callable(getattr(native, run)) and callable(getattr(G, run)), (name, run)
        assert "is_contiguous" not in src and ".dtype" not in src and ".shape[0]" not in src     # (no rule of its own)
    assert not [n for n in vars(U) if n.startswith("_FUSED_")] and not hasattr(U, "_load_fused_ops")
    assert U._fused_native() is native and U._fused_native() is native


def test_the_residual_declines_on_the_cpu_too():
    """What the parent's gates declined and the ops' rules take: declined before the rule is asked."""
    import mccnn_amd.MCNetworkUtils as U
    import mccnn_amd.dense_glue as G
    asked = []
    for op, kw in (("linear_xent", dict(weights=torch.ones(6, requires_grad=True))), ("cosine_loss", dict(weights=torch.ones(6, requires_grad=True))),
                   ("seg_counts", dict(ignoreLabel=-2 ** 31)), ("voxel_counts", dict(ignoreLabel=-2 ** 31))):
        st, a = store_for(op, dict(tables()[op][0], **kw))
        spy = type("Spy", (), {"__getattr__": lambda self, n: asked.append(n) or getattr(G, n)})()
        was, U.dense_glue = U.dense_glue, spy
        try:
            with torch.no_grad():
                assert gate(op, st, a) is None
        finally:
            U.dense_glue = was
    assert asked == []
