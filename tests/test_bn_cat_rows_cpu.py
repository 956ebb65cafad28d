"""The dense glue over a concatenation of typed segments without a GPU (mccnn_bn_act_cat_fwd_rows / _bwd_rows,
dense_glue.bn_relu_dropout_cat on float32 and bfloat16 segments): the ABI, every argument error of the two entries before a
launch, the Python rule and the result type it resolves, the case table of tests/bn_cat_rows_ref.py, and the
columns-per-thread predicate of csrc/bn_cat.h -- compiled with the plain host compiler (tools/bn_cat_rows_check.cpp) --
against its restatement in tests/bn_cat_rows_ref.py."""
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
import bn_cat_ref as cat  # noqa: E402
import bn_cat_rows_ref as rc  # noqa: E402

BADARG, TOOLARGE, WORKSPACE, SHAPE = -1, -3, -4, -5
P = 4096    # never dereferenced on the host: every call below returns before a launch
T = 1 << 32


def _ptrs(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _ints(v):
    return (C.c_int * len(v))(*v)


def _calls(lib):
    """fwd(**k), bwd(**k): the two entries on valid defaults -- widths (8, 4, 4), types (bf16, f32, bf16) -- with any argument
    replaced by name. bf: the flags (None: xs_bf16 == NULL)."""
    def table(k):
        widths = k.get("cs", (8, 4, 4))
        xs = _ptrs(k.get("xs", (P,) * len(widths)))
        bf = k.get("bf", (1, 0, 1)[:len(widths)] + (0,) * max(0, len(widths) - 3))
        return widths, xs, None if bf is None else _ints(bf), _ints(widths)

    def fwd(**k):
        widths, xs, bf, cs = table(k)
        return lib.mccnn_bn_act_cat_fwd_rows(*[k.get(a, d) for a, d in (
            ("xs_arr", xs), ("bf_arr", bf), ("cs_arr", cs), ("nseg", len(widths)), ("n", 300), ("gamma", P), ("beta", P), ("mm", P),
            ("mv", P), ("mom", 0.99), ("eps", 1e-3), ("training", 1), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("y", P),
            ("yb", 0), ("saved", P), ("ws", P), ("wsb", 1 << 20), ("stream", None))])

    def bwd(**k):
        widths, xs, bf, cs = table(k)
        dxs = k["dxs"] if "dxs" in k else _ptrs((P,) * len(widths))
        return lib.mccnn_bn_act_cat_bwd_rows(*[k.get(a, d) for a, d in (
            ("xs_arr", xs), ("bf_arr", bf), ("cs_arr", cs), ("nseg", len(widths)), ("y", P), ("yb", 0), ("n", 300), ("gamma", P),
            ("beta", P), ("saved", P), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("dxs_arr", dxs), ("dgamma", P),
            ("dbeta", P), ("ws", P), ("wsb", 1 << 20), ("stream", None))])
    return fwd, bwd


def test_abi_and_binding():
    from mccnn_amd import _lib, build
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 30
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name, old in (("mccnn_bn_act_cat_fwd_rows", "mccnn_bn_act_cat_fwd"), ("mccnn_bn_act_cat_bwd_rows", "mccnn_bn_act_cat_bwd")):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[old][1]) + 1, name   # (xs_bf16)
    header = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    section = header[header.index("OVER A CONCATENATION"):header.index("WITH BATCH STATISTICS ACROSS RANKS")]
    assert "Not covered" in section and "bf16 segments" not in section.split("Not covered")[1].split("*/")[0]


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    fwd, bwd = _calls(lib)
    for call in (fwd, bwd):
        # the segments' flags: outside {0, 1}
        for flag in (2, -1, 3, 256):
            assert call(bf=(flag, 0, 0)) == BADARG and call(bf=(0, 0, flag)) == BADARG and call(cs=(4,), bf=(flag,)) == BADARG
        assert call(bf=(2, 0, 0), xs=(P + 1, P, P)) == BADARG          # ahead of the pointer's error
        # a bf16 pointer at an odd address (an f32 one there is the caller's business, as in the existing entries)
        assert call(xs=(P + 1, P, P)) == SHAPE and call(xs=(P, P, P + 3)) == SHAPE
        assert call(xs=(P + 2, P, P + 6), wsb=16) == WORKSPACE          # an even address is allowed
        assert call(xs=(P + 1, P, P), gamma=None) == BADARG and call(xs=(P + 1, P, P), T=0) == BADARG
        assert call(xs=(P + 1, P, P), cs=(1 << 30, 1 << 30, 4)) == TOOLARGE
        # NULL flags: all float32 -- accepted, and then an odd address is nobody's bf16 pointer
        assert call(bf=None, wsb=16) == WORKSPACE and call(bf=None, xs=(P + 1, P, P), wsb=16) == WORKSPACE
        assert call(bf=(0, 0, 0), wsb=16) == WORKSPACE and call(bf=(1, 1, 1), wsb=16) == WORKSPACE
        # everything the existing entries reject
        assert call(nseg=0) == BADARG and call(nseg=9) == BADARG and call(nseg=-1) == BADARG
        assert call(cs=(4,) * 9) == BADARG
        assert call(n=0) == BADARG and call(n=-5) == BADARG
        assert call(cs=(8, 0, 4)) == BADARG and call(cs=(8, 4, -4)) == BADARG
        assert call(xs=(P, None, P)) == BADARG
        assert call(xs_arr=None) == BADARG and call(cs_arr=None) == BADARG
        assert call(T=0) == BADARG and call(T=T + 1) == BADARG
        assert call(gamma=None) == BADARG and call(beta=None) == BADARG and call(saved=None) == BADARG and call(y=None) == BADARG
        for flag in (2, -1, 3, 256):
            assert call(yb=flag) == BADARG
        big = (1 << 30, 1 << 30)
        assert call(cs=big) == TOOLARGE and call(cs=big + (1,)) == TOOLARGE
        assert call(cs=big, T=0) == BADARG and call(cs=big, gamma=None) == BADARG
        assert call(cs=((1 << 31) - 2, 1)) != TOOLARGE
        assert call(cs=(8, 4, 3), yb=1) == SHAPE and call(cs=(1,), yb=1) == SHAPE
        assert call(y=P + 2, yb=1) == SHAPE
        assert call(cs=(5, 3), yb=1, wsb=16) == WORKSPACE
        assert call(wsb=16) == WORKSPACE and call(ws=None) == WORKSPACE
        need = lib.mccnn_bn_act_workspace_bytes(300, 16)
        assert need > 0 and call(wsb=need - 1) == WORKSPACE
    assert fwd(mm=None) == BADARG and fwd(mv=None) == BADARG
    assert bwd(dgamma=None) == BADARG and bwd(dbeta=None) == BADARG
    assert bwd(dxs=None, wsb=16) == WORKSPACE and bwd(dxs=_ptrs((None, P, None)), wsb=16) == WORKSPACE   # both are allowed
    # a wanted bf16 dx_s at an odd address; an f32 segment's, or one that is not wanted, is not looked at
    assert bwd(dxs=_ptrs((P + 1, P, P))) == SHAPE and bwd(dxs=_ptrs((P, P, P + 1))) == SHAPE
    assert bwd(dxs=_ptrs((P, P + 1, None)), wsb=16) == WORKSPACE
    assert lib.mccnn_debug_launch_count() == before


def test_python_rule_and_the_result_type():
    import mccnn_amd.MCConvModule as M
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib, dense_glue, native
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    g = lambda c: (torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c))   # noqa: E731
    z = torch.zeros
    bf, f32 = torch.bfloat16, torch.float32
    for op in (M.bn_relu_dropout_cat, native.bn_relu_drop_cat):
        for bad in (torch.float16, torch.float64, torch.int32):
            with pytest.raises(M.InvalidArgumentError, match="float32 \\(or bfloat16 storage\\)"):
                op([z(6, 4), z(6, 4, dtype=bad)], *g(8), True)
        # a bf16 segment on host tensors gets as far as the device check, and no further
        for xs in ([z(6, 4), z(6, 4, dtype=bf)], [z(6, 4, dtype=bf)], [z(6, 3, dtype=bf), z(6, 5, dtype=bf)]):
            with pytest.raises(M.InvalidArgumentError, match="must be CUDA tensors"):
                op(xs, *g(sum(x.shape[1] for x in xs)), True)
        # an odd C: refused where y is bf16 -- asked for, or (all segments bf16) by default
        with pytest.raises(M.InvalidArgumentError, match="even number of columns"):
            op([z(6, 4, dtype=bf), z(6, 1, dtype=bf)], *g(5), True)
        with pytest.raises(M.InvalidArgumentError, match="even number of columns"):
            op([z(6, 4, dtype=bf), z(6, 1)], *g(5), True, outDtype=bf)
        for kw in ({}, {"outDtype": f32}):      # a float32 y of an odd C passes that rule, whatever the segments are
            xs = [z(6, 4, dtype=bf), z(6, 1, dtype=bf if kw else f32)]
            with pytest.raises(M.InvalidArgumentError, match="must be CUDA tensors"):
                op(xs, *g(5), True, **kw)
    # the resolving function itself: torch.cat's result type where nothing is asked for
    res = dense_glue._bn_cat_out_dtype
    assert res([bf]) == bf and res([bf, bf, bf]) == bf
    assert res([f32]) == f32 and res([bf, f32]) == f32 and res([f32, bf, bf]) == f32
    for dts in ([bf], [f32], [bf, f32], [bf, bf]):
        assert res(dts, f32) == f32 and res(dts, bf) == bf
        assert res(dts) == torch.cat([z(2, 2, dtype=d) for d in dts], 1).dtype
        assert (res(dts) == bf) == rc.out_dtype_is_bf16([int(d == bf) for d in dts])
    # the helper's rule is that one: a host list of valid types is declined at the device check, call for call as before
    st = U.VariableStore("cpu", fused=True, fusedCat=True)
    assert U._fused_cat(st, [z(4, 6, dtype=bf), z(4, 2)], True, "A", True) is None
    assert st.dropCalls_ == 0
    assert lib.mccnn_debug_launch_count() == before


def test_case_table():
    ids = [rc.case_id(c) for c in rc.CASES]
    assert len(set(ids)) == len(rc.CASES) == 10
    assert max(len(c.widths) for c in rc.CASES) == cat.MAX_SEGMENTS
    expect = {i: True for i in ids}
    expect["257-8b+8b-off"] = False                     # 1 per thread by the 8-byte rule, 4 on the widened copies
    assert {rc.case_id(c): rc.same_plan(c) for c in rc.CASES} == expect
    assert [rc.rows_vec(c.widths, c.types, rc.byte_offsets(c)) for c in rc.CASES] == [1, 1, 4, 4, 4, 4, 1, 1, 4, 1]
    assert [rc.out_dtype_is_bf16(c.types) for c in rc.CASES] == [True, False, False, False, False, True, False, False, False, True]
    for c in rc.CASES:
        assert len(c.widths) == len(c.types) and set(c.types) <= {0, 1} and any(c.types)
        d = rc.data(c)
        at = 0
        for w, t in zip(c.widths, c.types):     # a bf16 segment's columns are bf16 values, the others the shared case's
            blk = d["x"][:, at:at + w]
            if t:
                assert (blk.view("uint32") & 0xffff == 0).all()
            else:
                assert blk.tobytes() == cat.ref.case(c.n, rc.width(c))["x"][:, at:at + w].tobytes()
            at += w


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("c++") is None, reason="no host compiler")
def test_host_check_of_the_columns_per_thread_predicate(tmp_path):
    exe = str(tmp_path / "bn_cat_rows_check")
    subprocess.check_call([shutil.which("g++") or shutil.which("c++"), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "bn_cat_rows_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 disagreements" in out.stdout, out.stdout[-2000:] + out.stderr
    lines = out.stdout.strip().split("\n")[:-1]
    assert len(lines) > 40000
    seen = set()
    for line in lines:
        widths, types, xo, dxo, vec = [f.strip() for f in line.split("|")]
        widths, types, xo = [[int(v) for v in f.split(",")] for f in (widths, types, xo)]
        dxo = None if dxo == "none" else [None if int(v) < 0 else int(v) for v in dxo.split(",")]
        assert rc.rows_vec(widths, types, xo, dxo) == int(vec), line
        seen.add((len(widths), int(vec), dxo is None, any(types), all(types)))
    # the tuples reach both answers for every number of segments, with and without gradients, and every mix of types
    for nseg in (1, 2, 3, 8):
        assert {(nseg, 1, False, True, False), (nseg, 4, False, True, False)} <= seen or nseg == 1
    assert {(1, 4, False, True, True), (1, 1, False, True, True), (2, 4, True, True, False), (2, 4, False, False, False)} <= seen
