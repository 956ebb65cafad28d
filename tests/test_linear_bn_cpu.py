"""The linear layer + dense glue as one op (linear_bn_relu_dropout) without a GPU: the float64 reference pinned against
torch's autograd, the band cap and the conditioning of the shared cases, the ABI and the argument errors of the three
C entries, and the CPU route of VariableStore(fusedLinear=True)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_act_ref as bn  # noqa: E402
import linear_bn_ref as ref  # noqa: E402


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_reference_equals_torch_autograd(shape):
    """Forward and the five gradients, with a given mask, against float64 autograd of mask * relu(batch_norm(x @ W + b))."""
    n, cin, cout = shape
    d = ref.case(*shape)
    mask = bn.keep_mask(5, n, cout, bn.threshold(0.7))
    scale = 1.0 / 0.7
    out = ref.forward(d, True, True, mask, scale)
    grads = ref.backward(d, out["z"], out["mean"], out["rstd"], True, mask, scale)
    t = {k: torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("x", "w", "b", "gamma", "beta")}
    z = t["x"] @ t["w"] + t["b"]
    y = (z - z.mean(0)) * torch.rsqrt(z.var(0, unbiased=False) + 1e-3) * t["gamma"] + t["beta"]
    y = torch.relu(y) * torch.tensor(mask.astype(np.float64) * scale)
    y.backward(torch.tensor(d["dy"], dtype=torch.float64))

    def close(a, b, what, scale=None):
        b = b.detach().numpy()
        assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max() if scale is None else scale), what

    close(out["y"], y, "y")
    close(grads["dx"], t["x"].grad, "dx")
    close(grads["dw"], t["w"].grad, "dW")
    # db is a cancelling sum whose true value is 0 (batch norm removes the bias): float64 itself leaves rounding noise of the
    # size of the summed magnitudes in it, so that is its scale, as in the GPU test
    close(grads["db"], t["b"].grad, "db", scale=np.abs(grads["dz"]).sum(0).max())
    close(grads["dgamma"], t["gamma"].grad, "dgamma")
    close(grads["dbeta"], t["beta"].grad, "dbeta")


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_gate_band_share_is_small(shape):
    """|pre| <= 1e-5 max|pre| holds for at most 1e-3 of the elements: the cap the GPU gate and backward tests rely on."""
    out = ref.forward(ref.case(*shape), True, True)
    assert bn.band_share(out["pre"]) <= 1e-3


def test_naive_statistics_miss_the_bar_in_both_regimes():
    """sum z^2 / n - mean^2 in f32 misses the saved rstd by more than 1e-4 on a case of either launch regime (n <= 256 and
    above): an epilogue of that form fails the GPU test."""
    missed = {True: 0, False: 0}
    for shape in ref.SHAPES:
        if shape[0] < 2:
            continue
        out = ref.forward(ref.case(*shape), True, True)
        naive = bn.naive_f32_rstd(out["z"].astype(np.float32))
        if (np.abs(naive - out["rstd"]) / out["rstd"]).max() > 1e-4:
            missed[shape[0] <= 256] += 1
    assert missed[True] >= 1 and missed[False] >= 1, missed


# ------------------------------------------------------------------------------------------------- ABI, argument errors
def test_abi_version():
    from mccnn_amd import _lib
    assert _lib.load().mccnn_abi_version() >= 21


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 0x7f0000000000   # a made-up, 16-byte aligned address: never dereferenced, every call below returns before a launch
    T = 1 << 32
    fwd = lambda **k: lib.mccnn_linear_bn_act_fwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("w", p), ("b", p), ("n", 300), ("cin", 6), ("cout", 8), ("gamma", p), ("beta", p), ("mm", p), ("mv", p),
        ("mom", 0.99), ("eps", 1e-3), ("training", 1), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("z", p), ("y", p),
        ("bf16", 0), ("saved", p), ("ws", p), ("wsb", 1 << 24), ("stream", None))])
    bwd = lambda **k: lib.mccnn_linear_bn_act_bwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("w", p), ("z", p), ("y", p), ("bf16", 0), ("n", 300), ("cin", 6), ("cout", 8), ("gamma", p), ("beta", p),
        ("saved", p), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("dx", p), ("dw", p), ("db", p), ("dgamma", p),
        ("dbeta", p), ("ws", p), ("wsb", 1 << 24), ("stream", None))])
    BADARG, TOOLARGE, WORKSPACE, SHAPE = -1, -3, -4, -5
    for call in (fwd, bwd):
        assert call(n=0) == BADARG and call(cin=0) == BADARG and call(cout=0) == BADARG
        assert call(T=0) == BADARG and call(T=T + 1) == BADARG
        assert call(x=None) == BADARG and call(w=None) == BADARG and call(gamma=None) == BADARG and call(saved=None) == BADARG
        assert call(z=None) == BADARG and call(y=None) == BADARG
        assert call(bf16=2) == BADARG and call(bf16=-1) == BADARG
        assert call(bf16=1, cout=7) == SHAPE and call(bf16=1, y=p + 2) == SHAPE
        assert call(wsb=16) == WORKSPACE and call(ws=None) == WORKSPACE and call(bf16=1, wsb=16) == WORKSPACE
        assert call(n=65535 * 64 + 1) == TOOLARGE and call(cin=1 << 16, cout=1 << 15) == TOOLARGE
    assert fwd(b=None) == BADARG and fwd(mm=None) == BADARG and fwd(mv=None) == BADARG
    assert bwd(dw=None) == BADARG and bwd(db=None) == BADARG and bwd(dgamma=None) == BADARG and bwd(dbeta=None) == BADARG
    # the workspace: one query for both directions; the training forward needs the glue's share of it, eval none
    need = lib.mccnn_linear_bn_act_workspace_bytes(300, 6, 8)
    assert need >= 300 * 8 * 4 + lib.mccnn_bn_act_workspace_bytes(300, 8)
    assert bwd(wsb=need - 1) == WORKSPACE and fwd(wsb=lib.mccnn_bn_act_workspace_bytes(300, 8) - 1) == WORKSPACE
    assert lib.mccnn_linear_bn_act_workspace_bytes(0, 6, 8) == 0
    # modest for the widest layers: the dW planes stay below 16 MiB + one plane
    big = lib.mccnn_linear_bn_act_workspace_bytes(131072, 1536, 1024)
    assert big - 131072 * 1024 * 4 - lib.mccnn_bn_act_workspace_bytes(131072, 1024) <= (16 << 20) + 1536 * 1024 * 4 + 8192
    assert lib.mccnn_debug_launch_count() == before


def test_op_argument_errors_launch_nothing():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    x, w, b = torch.zeros(6, 4), torch.zeros(4, 8), torch.zeros(8)
    g, be, mm, mv = torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8)
    bad = [dict(x=x.double()), dict(x=torch.zeros(4, 6).t()), dict(w=torch.zeros(5, 8)), dict(w=w.double()), dict(b=torch.zeros(4)),
           dict(gamma=g.double()), dict(movingVar=torch.ones(16)[::2]), dict(keepProb=0.0), dict(keepProb=1.5),
           dict(seed=-1), dict(seed=1 << 32), dict(outDtype=torch.float16), dict(x=x.bfloat16()), dict()]
    for kw in bad:   # (the last one: everything in order but on the CPU)
        args = dict(x=x, w=w, b=b, gamma=g, beta=be, movingMean=mm, movingVar=mv, training=True, keepProb=0.5, seed=1)
        args.update(kw)
        with pytest.raises(M.InvalidArgumentError):
            M.linear_bn_relu_dropout(**args)
    with pytest.raises(M.InvalidArgumentError):
        M.linear_bn_relu_dropout(x, torch.zeros(4, 7), torch.zeros(7), torch.ones(7), torch.zeros(7), torch.zeros(7), torch.ones(7),
                                 True, outDtype=torch.bfloat16)
    assert lib.mccnn_debug_launch_count() == before


def test_header_binding_and_library_agree():
    import re
    import subprocess
    from mccnn_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_linear_bn_act_workspace_bytes", "mccnn_linear_bn_act_fwd", "mccnn_linear_bn_act_bwd"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    assert "linear_bn.hip" in build.SOURCES


# ------------------------------------------------------------------------------------------------- VariableStore(fusedLinear=True) on the CPU
def _outputs(fusedLinear, new_helper):
    import mccnn_amd.MCNetworkUtils as U
    torch.manual_seed(11)
    st = U.VariableStore(fused=True, fusedLinear=fusedLinear)
    x = torch.randn(40, 12)
    torch.manual_seed(12)
    if new_helper:
        r = U.conv_1x1_batch_norm_RELU_drop_out("R", "R_Out", x, 12, 6, True, True, 0.6, st)
    else:
        r = U.batch_norm_RELU_drop_out("R_Out", U.conv_1x1("R", x, 12, 6, st), True, True, 0.6, st)
    outs = [r,
            U.MLP_2_hidden(x, 12, 10, 8, 5, "M2", 0.5, True, useDropOut=True, store=st),
            U.MLP_1_hidden(x, 12, 9, 4, "M1", 0.5, True, useDropOut=True, store=st)]
    with torch.no_grad():
        if new_helper:
            outs.append(U.conv_1x1_batch_norm_RELU_drop_out("R", "R_Out", x, 12, 6, False, True, 0.6, st, outDtype=torch.bfloat16))
        else:
            outs.append(U.batch_norm_RELU_drop_out("R_Out", U.conv_1x1("R", x, 12, 6, st), False, True, 0.6, st,
                                                   outDtype=torch.bfloat16))
    return st, outs


def test_fused_linear_store_on_cpu_tensors_is_the_existing_path():
    """The new helper and both MLP helpers on CPU tensors: the bytes of the existing helpers, the same state_dict keys (in
    creation order) and initial values under one seed, dropCalls_ advancing equally."""
    st0, o0 = _outputs(False, False)
    for fusedLinear, new_helper in ((False, True), (True, True), (True, False)):
        st1, o1 = _outputs(fusedLinear, new_helper)
        assert st1.fusedLinear_ is fusedLinear
        for a, b in zip(o0, o1):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert st1.dropCalls_ == st0.dropCalls_
        sd0, sd1 = st0.state_dict(), st1.state_dict()
        assert list(sd0.keys()) == list(sd1.keys())
        for k in sd0:
            assert sd0[k].shape == sd1[k].shape and torch.equal(sd0[k], sd1[k]), k
        assert [id(p) for p in st1.get_collection('weight_decay_loss')] == [id(st1.variables_[k]) for k in (
            "R_weights", "M2_weights1", "M2_weights2", "M2_weights3", "M1_weights1", "M1_weights2")]
    assert "R_weights" in st0.state_dict() and "R_Out_BN/moving_variance" in st0.state_dict()


def test_the_switch_is_off_by_default_and_reassignable():
    import mccnn_amd.MCNetworkUtils as U
    assert U.VariableStore().fusedLinear_ is False and U.get_default_store().fusedLinear_ is False
    st = U.VariableStore("cpu", True, True)
    assert st.fused_ is True and st.fusedLinear_ is True
    st.fusedLinear_ = False
    assert U._fused_linear(st, torch.zeros(4, 3), torch.zeros(3, 2), torch.zeros(2), True, "L") is None
