"""The last linear layer + softmax cross-entropy as one op (linear_softmax_xent) without a GPU: the float64 reference pinned
against torch's autograd, the ABI and the argument errors of the three C entries, the checks of the Python op, and the CPU
route of VariableStore(fusedLoss=True), MLP_2_hidden / MLP_1_hidden(labels=...) and conv_1x1_softmax_cross_entropy."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xent_ref as ref  # noqa: E402

CASES = [(s, hot, wts) for s in ref.SHAPES for hot in (False, True) for wts in (False, True)]
CASE_IDS = ["%dx%dx%d%s%s" % (s + ("-hot" if hot else "", "-weights" if wts else "")) for s, hot, wts in CASES]


@pytest.mark.parametrize("shape,hot,wts", CASES, ids=CASE_IDS)
def test_reference_equals_torch_autograd(shape, hot, wts):
    """Forward and the three gradients against float64 torch.nn.functional.cross_entropy: rows that are not live are mapped
    to ignore_index; the weighted form is spelled out (sum of weight * row loss over the live rows / their number)."""
    n, cin, C = shape
    d = ref.case(*shape, hot=hot)
    rw = d["rw"] if wts else None
    z = ref.linear(d["x"], d["w"], d["b"])
    out = ref.forward(z, d["labels"], rw)
    grads = ref.backward(d["x"], d["w"], z, d["labels"], rw, g=0.75)
    t = {k: torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("x", "w", "b")}
    zt = t["x"] @ t["w"] + t["b"]
    live = ref.live_rows(d["labels"], C, rw)
    assert out["D"] == max(int(live.sum()), 1) and np.array_equal(out["live"], live)
    y = torch.tensor(np.where(live, d["labels"], -100).astype(np.int64))
    if wts:
        rows = torch.nn.functional.cross_entropy(zt, y, ignore_index=-100, reduction="none")
        loss = (rows * torch.tensor(d["rw"], dtype=torch.float64)).sum() / out["D"]
    elif live.any():
        loss = torch.nn.functional.cross_entropy(zt, y, ignore_index=-100)
    else:
        loss = zt.sum() * 0.0
    (0.75 * loss).backward()

    def close(a, b, what):
        b = b.detach().numpy()
        assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max()), what

    close(np.float64(out["loss"]), loss, "loss")
    close(out["lse"], torch.logsumexp(zt, 1), "lse")
    close(grads["dx"], t["x"].grad, "dx")
    close(grads["dw"], t["w"].grad, "dW")
    close(grads["db"], t["b"].grad, "db")
    assert np.array_equal(out["pred"], zt.argmax(1).numpy())
    assert out["correct"] == int((live & (out["pred"] == d["labels"])).sum())
    if n >= 8:
        assert not live[3] and not live[5] and not grads["dz"][3].any() and not grads["dx"][5].any()
    if hot and C >= 3:
        assert z.max() > 89.0 and np.isfinite(out["loss"])   # (exp(89) overflows float32: a naive exp(z) does not do here)


def test_no_live_row_gives_zero_not_nan():
    d = ref.case(64, 16, 21)
    z = ref.linear(d["x"], d["w"], d["b"])
    for labels, rw in ((np.full(64, 21, np.int32), None), (np.full(64, -1, np.int32), d["rw"]), (d["labels"], np.zeros(64, np.float32))):
        out = ref.forward(z, labels, rw)
        g = ref.backward(d["x"], d["w"], z, labels, rw, g=2.0)
        assert out["loss"] == 0.0 and out["D"] == 1 and out["correct"] == 0
        assert not g["dx"].any() and not g["dw"].any() and not g["db"].any()


# ------------------------------------------------------------------------------------------------- ABI, argument errors
def test_abi_version():
    from mccnn_amd import _lib
    assert _lib.load().mccnn_abi_version() >= 23


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 0x7f0000000000   # a made-up, 16-byte aligned address: never dereferenced, every call below returns before a launch
    fwd = lambda **k: lib.mccnn_linear_xent_fwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("w", p), ("b", p), ("n", 300), ("cin", 6), ("c", 8), ("labels", p), ("rw", p), ("loss", p), ("lse", p),
        ("meta", p), ("pred", p), ("logits", p), ("ws", p), ("wsb", 1 << 24), ("stream", None))])
    bwd = lambda **k: lib.mccnn_linear_xent_bwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("w", p), ("b", p), ("n", 300), ("cin", 6), ("c", 8), ("labels", p), ("rw", p), ("lse", p), ("meta", p),
        ("g", p), ("dx", p), ("dw", p), ("db", p), ("ws", p), ("wsb", 1 << 24), ("stream", None))])
    BADARG, TOOLARGE, WORKSPACE = -1, -3, -4
    for call in (fwd, bwd):
        assert call(n=0) == BADARG and call(cin=0) == BADARG and call(c=0) == BADARG and call(n=-5) == BADARG
        for name in ("x", "w", "b", "labels", "lse", "meta"):
            assert call(**{name: None}) == BADARG, name
        assert call(wsb=16) == WORKSPACE and call(ws=None) == WORKSPACE
        assert call(n=65535 * 64 + 1) == TOOLARGE and call(cin=1 << 16, c=1 << 15) == TOOLARGE
    assert fwd(loss=None) == BADARG
    assert bwd(g=None) == BADARG and bwd(dw=None) == BADARG and bwd(db=None) == BADARG
    # the workspace: one query for both directions. The backward needs all of it, the forward the front (its slab
    # partials), and nothing up to 256 rows
    need = lib.mccnn_linear_xent_workspace_bytes(300, 6, 8)
    assert need >= 300 * 8 * 4
    assert bwd(wsb=need - 1) == WORKSPACE
    assert bwd(n=200, ws=None) == WORKSPACE and bwd(n=200, wsb=200 * 8 * 4 - 1) == WORKSPACE
    assert lib.mccnn_debug_launch_count() == before


def test_workspace_query():
    """Monotone in each size, 0 for sizes the op refuses, modest for a wide head (the dW planes stay below 16 MiB + one)."""
    from mccnn_amd import _lib
    lib = _lib.load()
    q = lib.mccnn_linear_xent_workspace_bytes
    assert q(0, 6, 8) == 0 and q(6, 0, 8) == 0 and q(6, 8, 0) == 0 and q(-1, 6, 8) == 0
    assert q(65535 * 64 + 1, 6, 8) == 0 and q(300, 1 << 16, 1 << 15) == 0
    assert q(1, 1, 1) >= 4
    ns = [1, 63, 64, 65, 256, 257, 512, 513, 1000, 4099, 20000, 131072, 65535 * 64]
    for cin, c in ((1, 1), (16, 21), (64, 40), (128, 50), (33, 257)):
        sizes = [q(n, cin, c) for n in ns]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (cin, c, sizes)
        assert all(s >= n * c * 4 for s, n in zip(sizes, ns))
    for n in (300, 20000):
        assert q(n, 16, 50) <= q(n, 17, 50) <= q(n, 64, 50) and q(n, 16, 50) <= q(n, 16, 51) <= q(n, 16, 130)
    big = q(131072, 1536, 1024)
    assert big - 131072 * 1024 * 4 <= (16 << 20) + 1536 * 1024 * 4 + 8192


def test_header_binding_and_library_agree():
    import re
    import subprocess
    from mccnn_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_linear_xent_workspace_bytes", "mccnn_linear_xent_fwd", "mccnn_linear_xent_bwd"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    assert "linear_xent.hip" in build.SOURCES and "lin_tile.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "lin_tile.h"))


# ------------------------------------------------------------------------------------------------- the Python op
def test_op_argument_errors_launch_nothing():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, dense_glue, native
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    assert M.linear_softmax_xent is dense_glue.linear_softmax_xent and M._linear_xent_args is dense_glue._linear_xent_args
    x, w, b = torch.zeros(6, 4), torch.zeros(4, 8), torch.zeros(8)
    y, rw = torch.zeros(6, dtype=torch.int32), torch.ones(6)
    bad = [(dict(x=x.double()), "x must be a float32 tensor"), (dict(w=w.double()), "w must be a float32 tensor"),
           (dict(x=torch.zeros(4, 6).t()), "x and w must be contiguous"), (dict(w=torch.zeros(5, 8)), r"expects x \(n, cin\) and w \(cin, c\)"),
           (dict(x=torch.zeros(6)), r"expects x \(n, cin\)"), (dict(b=torch.zeros(4)), r"b must be a float32 \(c,\) tensor"),
           (dict(b=b.double()), "b must be a float32"), (dict(labels=y.float()), "labels must be an int32"),
           (dict(labels=[0] * 6), "labels must be an int32"), (dict(labels=torch.zeros(5, dtype=torch.int32)), r"labels must have shape \(n,\) or \(n, 1\)"),
           (dict(labels=torch.zeros(1, 6, dtype=torch.int64)), "labels must have shape"),
           (dict(labels=torch.zeros(12, dtype=torch.int32)[::2]), "labels must be contiguous"),
           (dict(weights=rw.double()), "weights must be a float32 tensor"), (dict(weights=torch.ones(7)), "weights must have shape"),
           (dict(weights=torch.ones(12)[::2]), "weights must be contiguous"),
           (dict(weights=torch.ones(6, requires_grad=True)), "no gradient with respect to weights"),
           (dict(), "x must be a CUDA tensor"), (dict(labels=torch.zeros(6, 1, dtype=torch.int64), weights=rw), "x must be a CUDA tensor")]
    for op in (M.linear_softmax_xent, native.linear_softmax_xent):
        for kw, text in bad:   # (the last two: everything in order but on the CPU)
            args = dict(x=x, w=w, b=b, labels=y)
            args.update(kw)
            with pytest.raises(M.InvalidArgumentError, match="linear_softmax_xent.*" + text):
                op(**args)
    assert lib.mccnn_debug_launch_count() == before
    doc = M.linear_softmax_xent.__doc__
    assert "NOT" in doc and "differentiable" in doc and "int64" in doc and "one torch" in doc


# ------------------------------------------------------------------------------------------------- the helpers on the CPU
def _head_case(n=40, cin=12, C=5, seed=21):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32) * 2)
    labels = rng.integers(0, C, n)
    labels[3], labels[5] = -1, C
    rw = rng.uniform(0.25, 4, n).astype(np.float32)
    rw[::7] = 0
    return x, labels, rw


def _check_head(head, hidden, w, b, labels, rw, wantLogits):
    """A LossHead against the float64 reference on the float64 logits of the helper's own hidden rows."""
    import mccnn_amd.MCNetworkUtils as U
    assert isinstance(head, U.LossHead) and head._fields == ("loss", "pred", "correct", "denom", "logits")
    z = ref.linear(hidden.detach().numpy(), w.detach().numpy(), b.detach().numpy())
    want = ref.forward(z, labels, rw)
    assert head.loss.dim() == 0 and head.loss.dtype == torch.float32 and head.loss.requires_grad
    assert abs(float(head.loss.detach()) - want["loss"]) <= 1e-5 * max(1.0, abs(want["loss"]))
    assert head.pred.dtype == torch.int32 and np.array_equal(head.pred.numpy(), want["pred"])
    assert int(head.correct) == want["correct"] and int(head.denom) == want["D"]
    if wantLogits:
        assert not head.logits.requires_grad and np.abs(head.logits.numpy() - z).max() <= 1e-5 * np.abs(z).max()
    else:
        assert head.logits is None


@pytest.mark.parametrize("fusedLoss", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("wts", [False, True], ids=["plain", "weights"])
def test_helpers_with_labels_on_cpu_tensors(fusedLoss, wts):
    """MLP_2_hidden(labels=...), MLP_1_hidden and conv_1x1_softmax_cross_entropy on CPU tensors: the reference's loss, pred,
    correct and denom with the switch off AND on (on the CPU, on falls back to the torch code); the variables have the names,
    shapes, values and creation order of the labels=None calls; labels=None returns hidden @ w + b bit for bit; the gradients
    of the last linear are the reference's."""
    import mccnn_amd.MCNetworkUtils as U
    x, labels, rw = _head_case()
    weights = torch.from_numpy(rw) if wts else None
    rwn = rw if wts else None
    stores, outs = [], []
    for with_labels in (False, True):
        torch.manual_seed(11)
        st = U.VariableStore(fused=True, fusedLinear=True, fusedLoss=fusedLoss)
        assert st.fusedLoss_ is fusedLoss
        kw = dict(labels=torch.from_numpy(labels).reshape(-1, 1), labelWeights=weights, wantLogits=wts) if with_labels else {}
        kw1 = dict(labels=torch.from_numpy(labels.astype(np.int32)), labelWeights=weights) if with_labels else {}
        o = [U.MLP_2_hidden(x, 12, 10, 8, 5, "M2", 0.5, False, store=st, **kw),
             U.MLP_1_hidden(x, 12, 9, 5, "M1", 0.5, False, store=st, **kw1)]
        if with_labels:
            o.append(U.conv_1x1_softmax_cross_entropy("R", x, 12, 5, torch.from_numpy(labels), weights, True, st))
        else:
            o.append(U.conv_1x1("R", x, 12, 5, st))
        stores.append(st)
        outs.append(o)
    sd0, sd1 = stores[0].state_dict(), stores[1].state_dict()
    assert list(sd0.keys()) == list(sd1.keys()) and "M2_weights3" in sd0 and "M1_biases2" in sd0 and "R_weights" in sd0
    for k in sd0:
        assert sd0[k].shape == sd1[k].shape and torch.equal(sd0[k], sd1[k]), k
    for st in stores:
        assert [id(p) for p in st.get_collection('weight_decay_loss')] == [id(st.variables_[k]) for k in (
            "M2_weights1", "M2_weights2", "M2_weights3", "M1_weights1", "M1_weights2", "R_weights")]
    # labels=None: the logits as before, bit for bit -- and from them the hidden rows the heads were computed on
    st = stores[1]
    v = st.variables_
    with torch.no_grad():
        f = U.batch_normalization(x, False, "M2_BN_Init", st)
        h1 = torch.relu(U.batch_normalization(f @ v["M2_weights1"] + v["M2_biases1"], False, "M2_BN_h1", st))
        h2 = torch.relu(U.batch_normalization(h1 @ v["M2_weights2"] + v["M2_biases2"], False, "M2_BN_h2", st))
        g1 = torch.relu(U.batch_normalization(x @ v["M1_weights1"] + v["M1_biases1"], False, "M1_BN_h", st))
        assert torch.equal(outs[0][0], h2 @ v["M2_weights3"] + v["M2_biases3"])
        assert torch.equal(outs[0][1], g1 @ v["M1_weights2"] + v["M1_biases2"])
        assert torch.equal(outs[0][2], x @ v["R_weights"] + v["R_biases"])
    _check_head(outs[1][0], h2, v["M2_weights3"], v["M2_biases3"], labels, rwn, wts)
    _check_head(outs[1][1], g1, v["M1_weights2"], v["M1_biases2"], labels, rwn, False)
    _check_head(outs[1][2], x, v["R_weights"], v["R_biases"], labels, rwn, True)
    # the gradients of the helper's own linear
    (2.0 * outs[1][2].loss).backward()
    z = ref.linear(x.numpy(), v["R_weights"].detach().numpy(), v["R_biases"].detach().numpy())
    want = ref.backward(x.numpy(), v["R_weights"].detach().numpy(), z, labels, rwn, g=2.0)
    assert np.abs(v["R_weights"].grad.numpy() - want["dw"]).max() <= 1e-5 * np.abs(want["dw"]).max()
    assert np.abs(v["R_biases"].grad.numpy() - want["db"]).max() <= 1e-5 * np.abs(want["dz"]).sum(0).max()


def test_no_live_row_through_the_helper_on_cpu():
    import mccnn_amd.MCNetworkUtils as U
    x, labels, _ = _head_case()
    st = U.VariableStore(fusedLoss=True)
    head = U.conv_1x1_softmax_cross_entropy("R", x, 12, 5, torch.full((40,), 7, dtype=torch.int64), store=st)
    head.loss.backward()
    assert float(head.loss.detach()) == 0.0 and int(head.denom) == 1 and int(head.correct) == 0
    assert not st.variables_["R_weights"].grad.any() and not st.variables_["R_biases"].grad.any()
    assert not torch.isnan(st.variables_["R_weights"].grad).any()


def test_the_switch_is_off_by_default_and_reassignable():
    import mccnn_amd.MCNetworkUtils as U
    assert U.VariableStore().fusedLoss_ is False and U.get_default_store().fusedLoss_ is False
    st = U.VariableStore("cpu", True, True, False, True)
    assert st.fused_ is True and st.fusedLinear_ is True and st.fusedSync_ is False and st.fusedLoss_ is True
    y = torch.zeros(4, dtype=torch.int64)
    assert U._fused_loss(st, torch.zeros(4, 3), torch.zeros(3, 2), torch.zeros(2), y, None, False) is None   # (CPU tensors)
    st.fusedLoss_ = False
    assert U._fused_loss(st, torch.zeros(4, 3), torch.zeros(3, 2), torch.zeros(2), y, None, False) is None


def test_mcclass_s_takes_the_switch_and_labels():
    """The example network: the constructor argument reaches the store, forward() has the labels argument, the script the flag."""
    import inspect
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import mcclass_s
    net = mcclass_s.MCClassS(1, 2, 16, 4, torch.device("cpu"), fusedLoss=True)
    assert net.store.fusedLoss_ is True and mcclass_s.MCClassS(1, 2, 16, 4, torch.device("cpu")).store.fusedLoss_ is False
    assert inspect.signature(net.forward).parameters["labels"].default is None
    assert "--fused-loss" in inspect.getsource(mcclass_s.main)
