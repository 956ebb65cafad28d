"""The fused dense glue on bf16 rows without a GPU: the helper's NumPy bfloat16 against torch's, the share of elements in
the gate band of every case, the argument checks of the op and of the C ABI (nothing is launched), header / binding /
library agreement, and the helpers' torch path with an output type."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bn_act_ref as ref  # noqa: E402
import bn_act_rows_ref as rows  # noqa: E402


def test_numpy_bf16_is_torch_bf16():
    rng = np.random.default_rng(11)
    a = (rng.standard_normal(20000) * 10.0 ** rng.uniform(-20, 20, 20000)).astype(np.float32)
    # exact ties: a bf16 value plus half a unit in its last place, for even and odd last bits, both signs
    base = (rng.integers(0x0080, 0x7F00, 4000).astype(np.uint32) << np.uint32(16)) | np.uint32(0x8000)
    ties = np.concatenate([base, base | np.uint32(0x80000000)]).view(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 3.25, 1.00390625, 1.01171875, 3.3895314e38, 1e-40], np.float32)
    for v in (a, ties, special):
        want = torch.from_numpy(v).to(torch.bfloat16)
        assert np.array_equal(rows.to_bf16_bits(v), want.view(torch.int16).numpy().view(np.uint16))
        assert np.array_equal(rows.round_bf16(v), want.float().numpy())
    assert np.array_equal(rows.from_bf16_bits(rows.to_bf16_bits(ties)), rows.round_bf16(ties))


@pytest.mark.parametrize("x_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", rows.SHAPES, ids=lambda s: "%dx%d" % s)
def test_few_elements_in_the_gate_band(shape, x_bf16):
    """The GPU gate test allows 1e-3 of the elements to differ, and gates can only differ inside the band."""
    out, _, _ = rows.reference(shape, x_bf16, True, None, 0)
    assert ref.band_share(out["pre"]) <= 1e-3


def test_case_rounds_the_bf16_operands_only():
    n, c = 63, 6
    base = ref.case(n, c)
    for xb, yb in rows.COMBOS:
        d = rows.case(n, c, xb, yb)
        assert np.array_equal(d["x"], rows.round_bf16(base["x"]) if xb else base["x"])
        assert np.array_equal(d["dy"], rows.round_bf16(base["dy"]) if yb else base["dy"])
        assert np.array_equal(d["gamma"], base["gamma"]) and d["x"].dtype == np.float32


def test_argument_errors_launch_nothing():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    g = lambda c: (torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c))   # noqa: E731
    bf = torch.bfloat16
    bad = [
        (torch.zeros(6, 5, dtype=bf), g(5), {}),                                 # odd c, bf16 x
        (torch.zeros(6, 5), g(5), dict(outDtype=bf)),                            # odd c, bf16 y
        (torch.zeros(6, 4), g(4), dict(outDtype=torch.float16)),
        (torch.zeros(6, 4), g(4), dict(outDtype=torch.float64)),
        (torch.zeros(6, 4, dtype=bf), g(4), dict(outDtype=torch.float16)),
        (torch.zeros(6, 4, dtype=torch.float16), g(4), {}),
        (torch.zeros(6, 4, dtype=bf), (torch.ones(4, dtype=bf),) + g(4)[1:], {}),    # bf16 gamma
        (torch.zeros(6, 4, dtype=bf), g(4)[:1] + (torch.zeros(4, dtype=bf),) + g(4)[2:], {}),   # bf16 beta
    ]
    for x, (gm, bt, mm, mv), kw in bad:
        with pytest.raises(M.InvalidArgumentError):
            M.bn_relu_dropout(x, gm, bt, mm, mv, True, True, 0.5, 1, **kw)
    # a host tensor of a valid type still gets as far as the device check, and no further
    with pytest.raises(M.InvalidArgumentError):
        M.bn_relu_dropout(torch.zeros(6, 4, dtype=bf), *g(4), True, True, 0.5, 1, outDtype=torch.float32)
    assert M._bn_act_args.__defaults__ == (None,)                               # outDtype is optional: old callers stand
    assert lib.mccnn_debug_launch_count() == before


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 4096   # never dereferenced on the host: every call below returns before a launch
    T = 1 << 32
    fwd = lambda **k: lib.mccnn_bn_act_fwd_rows(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("xb", 1), ("n", 300), ("c", 8), ("gamma", p), ("beta", p), ("mm", p), ("mv", p), ("mom", 0.99), ("eps", 1e-3),
        ("training", 1), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("y", p), ("yb", 1), ("saved", p), ("ws", p),
        ("wsb", 1 << 20), ("stream", None))])
    bwd = lambda **k: lib.mccnn_bn_act_bwd_rows(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("xb", 1), ("dy", p), ("yb", 1), ("n", 300), ("c", 8), ("gamma", p), ("beta", p), ("saved", p), ("relu", 1),
        ("T", T), ("scale", 1.0), ("seed", 0), ("dx", p), ("dgamma", p), ("dbeta", p), ("ws", p), ("wsb", 1 << 20),
        ("stream", None))])
    BADARG, WORKSPACE, SHAPE = -1, -4, -5
    for call in (fwd, bwd):
        for types in (dict(xb=0, yb=0), dict(xb=0, yb=1), dict(xb=1, yb=0), dict(xb=1, yb=1)):
            # everything the float32 entries reject
            assert call(n=0, **types) == BADARG and call(c=0, **types) == BADARG
            assert call(T=0, **types) == BADARG and call(T=T + 1, **types) == BADARG
            assert call(x=None, **types) == BADARG and call(gamma=None, **types) == BADARG and call(saved=None, **types) == BADARG
            assert call(wsb=16, **types) == WORKSPACE and call(ws=None, **types) == WORKSPACE
        # a type flag outside {0, 1}
        for flag in (2, -1, 3, 256):
            assert call(xb=flag) == BADARG and call(yb=flag) == BADARG
        # odd c with a bf16 operand
        assert call(c=7, xb=1, yb=0) == SHAPE and call(c=7, xb=0, yb=1) == SHAPE and call(c=7, xb=1, yb=1) == SHAPE
        # a bf16 pointer with bit 1 set
        assert call(x=p + 2, xb=1, yb=0) == SHAPE
    assert fwd(y=p + 2, xb=0, yb=1) == SHAPE and fwd(y=p + 6) == SHAPE
    assert bwd(dy=p + 2, xb=0, yb=1) == SHAPE and bwd(dx=p + 2, xb=1, yb=0) == SHAPE
    assert fwd(y=None) == BADARG and fwd(mm=None) == BADARG
    assert bwd(dy=None) == BADARG and bwd(dgamma=None) == BADARG and bwd(dbeta=None) == BADARG
    # the workspace query covers every type combination: it does not know the types
    need = lib.mccnn_bn_act_workspace_bytes(300, 8)
    assert fwd(wsb=need - 1) == WORKSPACE and bwd(wsb=need - 1) == WORKSPACE
    assert lib.mccnn_debug_launch_count() == before


def test_header_binding_and_library_agree():
    from mccnn_amd import _lib, build
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 19
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_bn_act_fwd_rows", "mccnn_bn_act_bwd_rows", "mccnn_bn_act_fwd", "mccnn_bn_act_bwd"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    # the number of parameters of the declaration is the number the binding passes
    for name in ("mccnn_bn_act_fwd_rows", "mccnn_bn_act_bwd_rows"):
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_helper_on_host_tensors_is_the_torch_result_cast(training):
    import mccnn_amd.MCNetworkUtils as U
    torch.manual_seed(4)
    x = torch.randn(40, 6) * 2 + 1
    outs = {}
    for fused in (False, True):          # (host tensors: the fused op does not apply, the torch code runs)
        for dt in (None, torch.bfloat16, torch.float32):
            st = U.VariableStore("cpu", fused=fused)
            kw = {} if dt is None else {"outDtype": dt}
            with torch.no_grad():
                outs[fused, dt] = U.batch_norm_RELU_drop_out("L", x, training, False, None, st, **kw)
            assert st.dropCalls_ == 0
    plain = outs[False, None]
    assert plain.dtype == torch.float32
    for fused in (False, True):
        assert torch.equal(outs[fused, None], plain) and torch.equal(outs[fused, torch.float32], plain)
        assert outs[fused, torch.bfloat16].dtype == torch.bfloat16
        assert torch.equal(outs[fused, torch.bfloat16], plain.to(torch.bfloat16))


def test_fused_glue_declines_what_it_does_not_cover():
    import mccnn_amd.MCNetworkUtils as U
    st = U.VariableStore("cpu", fused=True)
    assert U._fused_glue(st, torch.zeros(4, 6, dtype=torch.bfloat16), True, "A", True) is None     # a host tensor
    assert U._fused_glue(st, torch.zeros(4, 5, dtype=torch.bfloat16), True, "B", True) is None     # odd c
    assert U._fused_glue(st, torch.zeros(4, 6), True, "C", True, outDtype=torch.float16) is None
    assert st.dropCalls_ == 0
