"""The dense glue over a concatenation without a GPU (mccnn_bn_act_cat_fwd / _bwd, dense_glue.bn_relu_dropout_cat,
VariableStore(fusedCat=True)): the ABI, every argument error of the two entries and of the Python rule before a launch, the
helper on host tensors against torch.cat bit for bit, the plan predicate of tests/bn_cat_ref.py, and the host check of the
segment lookup (tools/bn_cat_check.cpp) compiled with the plain host compiler."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bn_act_ref as ref  # noqa: E402
import bn_cat_ref as cat  # noqa: E402

BADARG, TOOLARGE, WORKSPACE, SHAPE = -1, -3, -4, -5
P = 4096    # never dereferenced on the host: every call below returns before a launch
T = 1 << 32


def _table(ptrs, widths=None):
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    return arr if widths is None else (arr, (C.c_int * len(widths))(*widths))


def _calls(lib):
    def fwd(**k):
        widths = k.get("cs", (8, 4, 4))
        xs, cs = _table(k.get("xs", (P,) * len(widths)), widths)
        return lib.mccnn_bn_act_cat_fwd(*[k.get(a, d) for a, d in (
            ("xs_arr", xs), ("cs_arr", cs), ("nseg", len(widths)), ("n", 300), ("gamma", P), ("beta", P), ("mm", P), ("mv", P),
            ("mom", 0.99), ("eps", 1e-3), ("training", 1), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("y", P), ("yb", 0),
            ("saved", P), ("ws", P), ("wsb", 1 << 20), ("stream", None))])

    def bwd(**k):
        widths = k.get("cs", (8, 4, 4))
        xs, cs = _table(k.get("xs", (P,) * len(widths)), widths)
        dxs = k["dxs"] if "dxs" in k else _table((P,) * len(widths))
        return lib.mccnn_bn_act_cat_bwd(*[k.get(a, d) for a, d in (
            ("xs_arr", xs), ("cs_arr", cs), ("nseg", len(widths)), ("y", P), ("yb", 0), ("n", 300), ("gamma", P), ("beta", P),
            ("saved", P), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("dxs_arr", dxs), ("dgamma", P), ("dbeta", P),
            ("ws", P), ("wsb", 1 << 20), ("stream", None))])
    return fwd, bwd


def test_abi_and_binding():
    from mccnn_amd import _lib, build
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 28
    assert lib.mccnn_bn_act_cat_max_segments() == cat.MAX_SEGMENTS == 8
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_bn_act_cat_fwd", "mccnn_bn_act_cat_bwd", "mccnn_bn_act_cat_max_segments"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    for name in ("mccnn_bn_act_cat_fwd", "mccnn_bn_act_cat_bwd"):
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    fwd, bwd = _calls(lib)
    for call in (fwd, bwd):
        # the segments
        assert call(nseg=0) == BADARG and call(nseg=9) == BADARG and call(nseg=-1) == BADARG
        assert call(cs=(4,) * 9) == BADARG
        assert call(n=0) == BADARG and call(n=-5) == BADARG
        assert call(cs=(8, 0, 4)) == BADARG and call(cs=(8, 4, -4)) == BADARG
        assert call(xs=(P, None, P)) == BADARG
        assert call(xs_arr=None) == BADARG and call(cs_arr=None) == BADARG
        # what the contiguous entries reject
        assert call(T=0) == BADARG and call(T=T + 1) == BADARG
        assert call(gamma=None) == BADARG and call(beta=None) == BADARG and call(saved=None) == BADARG and call(y=None) == BADARG
        for flag in (2, -1, 3, 256):
            assert call(yb=flag) == BADARG
        # C past 2^31 - 1, behind the other argument errors
        big = (1 << 30, 1 << 30)
        assert call(cs=big) == TOOLARGE and call(cs=big + (1,)) == TOOLARGE
        assert call(cs=big, T=0) == BADARG and call(cs=big, gamma=None) == BADARG
        assert call(cs=((1 << 31) - 2, 1)) != TOOLARGE      # 2^31 - 1 itself is allowed (and then lacks its workspace)
        # bf16 rows: an odd C, a pointer off a 4-byte boundary
        assert call(cs=(8, 4, 3), yb=1) == SHAPE and call(cs=(1,), yb=1) == SHAPE
        assert call(y=P + 2, yb=1) == SHAPE
        assert call(cs=(5, 3), yb=1, wsb=16) == WORKSPACE   # (an even C of odd widths passes the shape rule)
        # the workspace
        assert call(wsb=16) == WORKSPACE and call(ws=None) == WORKSPACE
        need = lib.mccnn_bn_act_workspace_bytes(300, 16)
        assert need > 0 and call(wsb=need - 1) == WORKSPACE
    assert fwd(mm=None) == BADARG and fwd(mv=None) == BADARG
    assert bwd(dgamma=None) == BADARG and bwd(dbeta=None) == BADARG
    assert bwd(dxs=None, wsb=16) == WORKSPACE and bwd(dxs=_table((None, P, None)), wsb=16) == WORKSPACE   # both are allowed
    assert lib.mccnn_debug_launch_count() == before


def test_python_rule_refuses_before_launching():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    assert M.bn_relu_dropout_cat is not None and M._bn_cat_args is not None          # re-exported
    g = lambda c: (torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c))   # noqa: E731
    z = torch.zeros
    bad = [
        ([], g(4), {}),                                                   # no segment
        ([z(6, 1)] * 9, g(9), {}),                                        # more than 8
        (z(6, 4), g(4), {}),                                              # not a list
        ([z(6, 4), z(6, 4, dtype=torch.bfloat16)], g(8), {}),             # a bf16 segment
        ([z(6, 4), z(6, 4, dtype=torch.float64)], g(8), {}),
        ([z(6, 4), z(5, 4)], g(8), {}),                                   # rows differ
        ([z(6, 4), z(6, 0)], g(4), {}),                                   # an empty segment
        ([z(6, 4), z(24)], g(8), {}),                                     # not 2-D
        ([z(6, 4), z(6, 8)[:, ::2]], g(8), {}),                           # not contiguous
        ([z(6, 4), z(6, 4)], g(7), {}),                                   # per-column tensors of another width
        ([z(6, 4), z(6, 1)], g(5), dict(outDtype=torch.bfloat16)),        # odd C, bf16 y
        ([z(6, 4), z(6, 4)], g(8), dict(outDtype=torch.float16)),
        ([z(6, 4), z(6, 4)], g(8), dict(keepProb=0.0)),
        ([z(6, 4), z(6, 4)], g(8), dict(keepProb=1.5)),
        ([z(6, 4), z(6, 4)], g(8), dict(seed=-1)),
    ]
    for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
        for xs, (gm, bt, mm, mv), kw in bad:
            with pytest.raises(M.InvalidArgumentError):
                op(xs, gm, bt, mm, mv, True, True, **kw)
        # host tensors of valid types get as far as the device check, and no further
        with pytest.raises(M.InvalidArgumentError):
            op([z(6, 4), z(6, 4)], *g(8), True)
    assert lib.mccnn_debug_launch_count() == before


@pytest.mark.parametrize("fusedCat", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_helper_on_host_tensors_is_the_call_on_the_concatenation(training, fusedCat):
    """A list on CPU tensors: torch.cat followed by today's path, whatever the switches say -- bit for bit, forward and
    gradients, the same state_dict and no dropCalls_."""
    import mccnn_amd.MCNetworkUtils as U
    torch.manual_seed(4)
    parts = [torch.randn(40, w) * 2 + 1 for w in (3, 4, 1)]
    res = []
    for as_list in (False, True):
        st = U.VariableStore("cpu", fused=fusedCat, fusedCat=fusedCat)
        assert st.fusedCat_ is fusedCat
        xs = [p.clone().requires_grad_(training) for p in parts]
        arg = (tuple(xs) if training else list(xs)) if as_list else torch.cat(xs, 1)
        y = U.batch_norm_RELU_drop_out("L", arg, training, False, None, st)
        if training:
            (y * torch.arange(1.0, 9.0)).sum().backward()
        res.append((y.detach(), [x.grad for x in xs], {k: v.clone() for k, v in st.state_dict().items()},
                    [p.grad for p in st.parameters()]))
        assert st.dropCalls_ == 0
    (ya, ga, sa, pa), (yb, gb, sb, pb) = res
    assert torch.equal(ya, yb) and list(sa) == list(sb) == ["L_BN/gamma", "L_BN/beta", "L_BN/moving_mean", "L_BN/moving_variance"]
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    if training:
        assert all(torch.equal(a, b) for a, b in zip(ga, gb)) and all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_fused_cat_declines_what_it_does_not_cover():
    import mccnn_amd.MCNetworkUtils as U
    st = U.VariableStore("cpu", fused=True, fusedCat=True)
    z = torch.zeros
    assert U._fused_cat(st, [z(4, 6), z(4, 2)], True, "A", True) is None                                   # host tensors
    assert U._fused_cat(st, [z(4, 6), z(4, 2, dtype=torch.bfloat16)], True, "B", True) is None             # a bf16 segment
    assert U._fused_cat(st, [z(4, 1)] * 9, True, "C", True) is None                                        # more than 8
    st.fusedCat_ = False
    assert U._fused_cat(st, [z(4, 6), z(4, 2)], True, "D", True) is None and "D_BN/gamma" not in st.variables_
    assert st.dropCalls_ == 0
    assert U.VariableStore("cpu").fusedCat_ is False                                                       # opt-in


def test_plan_predicate_agrees_with_the_contiguous_rule():
    for c in range(1, 200):
        assert cat.row_lanes(cat.plain_vec(c), c) == ref.row_lanes(c)
        assert cat.row_lanes(cat.cat_vec((c,)), c) == ref.row_lanes(c)            # S = 1: always the contiguous plan
    expect = {cat.case_id(c): True for c in cat.CASES}
    expect["257-6+10"] = expect["257-8+8-off"] = False
    assert {cat.case_id(c): cat.plans_coincide(c) for c in cat.CASES} == expect
    assert len(cat.CASES) == 11 and max(len(c.widths) for c in cat.CASES) == cat.MAX_SEGMENTS
    for c in cat.CASES:   # the split is a partition of the shared case's columns
        d = cat.data(c)
        assert d["x"].shape == (c.n, cat.width(c))
        assert [s.shape[1] for s in cat.split(d["x"], c.widths)] == list(c.widths)


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("c++") is None, reason="no host compiler")
def test_host_check_of_the_segment_lookup(tmp_path):
    exe = str(tmp_path / "bn_cat_check")
    subprocess.check_call([shutil.which("g++") or shutil.which("c++"), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "bn_cat_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 disagreements" in out.stdout, out.stdout + out.stderr
