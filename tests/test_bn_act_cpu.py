"""The fused dense glue (bn_relu_dropout) without a GPU: the float64 reference pinned against torch's autograd, the mask
header compiled for the host, the kernels' f32 arithmetic restated in NumPy against the GPU test's bar, the band cap the
GPU backward test relies on, the CPU fallback of VariableStore(fused=True) and the argument errors."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_act_ref as ref  # noqa: E402
import helpers  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["%dx%d" % s for s in ref.SHAPES]


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
@pytest.mark.parametrize("relu", [True, False])
def test_reference_equals_torch_autograd(shape, relu):
    """Forward and the three gradients, with a given mask, against float64 autograd of mask * relu(batch_norm(x))."""
    n, c = shape
    d = ref.case(n, c)
    mask = ref.keep_mask(5, n, c, ref.threshold(0.7))
    scale = 1.0 / 0.7
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, relu, mask, scale)
    dx, dg, db = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale)
    x = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
    g = torch.tensor(d["gamma"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(d["beta"], dtype=torch.float64, requires_grad=True)
    if n > 1:
        y = torch.nn.functional.batch_norm(x, None, None, g, b, True, 0.0, 1e-3)
    else:   # (F.batch_norm refuses one value per channel: the same normalisation spelled out)
        y = (x - x.mean(0)) * torch.rsqrt(x.var(0, unbiased=False) + 1e-3) * g + b
    if relu:
        y = torch.relu(y)
    y = y * torch.tensor(mask.astype(np.float64) * scale)
    y.backward(torch.tensor(d["dy"], dtype=torch.float64))

    def close(a, t, what):
        t = t.detach().numpy()
        assert np.abs(a - t).max() <= 1e-10 * max(1.0, np.abs(t).max()), what

    close(out["y"], y, "y")
    close(dx, x.grad, "dx")
    close(dg, g.grad, "dgamma")
    close(db, b.grad, "dbeta")
    # the moving statistics: biased variance, momentum 0.99
    xd = d["x"].astype(np.float64)
    mv0, mm0 = d["mov_var"].astype(np.float64), d["mov_mean"].astype(np.float64)
    assert np.allclose(out["mov_var"], mv0 * 0.99 + xd.var(0) * 0.01, rtol=1e-12, atol=0)
    assert np.allclose(out["mov_mean"], mm0 * 0.99 + xd.mean(0) * 0.01, rtol=1e-12, atol=1e-15)


def test_host_build_of_the_mask_predicate(tmp_path):
    """csrc/bn_drop.h compiled for the host (tools/bn_drop_check.cpp): its own check passes and every dumped tuple has the
    NumPy mask's bit, T = 2^32 (all kept) and T = 1 included."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "bn_drop_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "bn_drop_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 disagreements" in out.stdout, out.stdout + out.stderr
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe, "--dump"], text=True).splitlines()]
    assert len(rows) == 4 * 5 * 5 * 5
    thresholds = {r[3] for r in rows}
    assert {1, ref.DROP_ALL, ref.threshold(0.7)} <= thresholds
    for seed, i, j, T, keep in rows:
        assert bool(ref.keep_bits(seed, i, j, T)) == bool(keep), (seed, i, j, T)
    assert all(r[4] == 1 for r in rows if r[3] == ref.DROP_ALL)
    assert sum(r[4] for r in rows if r[3] == 1) == 0   # (none of the 100 hashes is 0)


def test_mask_is_a_function_of_seed_row_and_column():
    a = ref.keep_mask(3, 50, 40, ref.threshold(0.7))
    assert np.array_equal(a, ref.keep_mask(3, 50, 40, ref.threshold(0.7)))
    assert not np.array_equal(a, ref.keep_mask(4, 50, 40, ref.threshold(0.7)))
    assert np.array_equal(a[:20, :10], ref.keep_mask(3, 20, 10, ref.threshold(0.7)))   # independent of the shape
    assert abs(a.mean() - 0.7) < 0.06
    assert ref.keep_mask(3, 5, 5, ref.DROP_ALL).all()
    assert int(ref.mix(0)) == 0 and int(ref.mix(1)) == 0x514E28B7


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernel_arithmetic_in_f32_meets_the_gpu_bar(shape):
    """Slab partials + Chan's merge restated in f32 NumPy stay within the GPU test's bar (assert_float_close, 1e-4) of the
    float64 reference; the plain f32 sum x^2 / n - mean^2 does not (so a kernel of that form fails the GPU test)."""
    n, c = shape
    d = ref.case(n, c)
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, False)
    y, mean, rstd = ref.kernel_forward_f32(d["x"], d["gamma"], d["beta"], relu=False)
    helpers.assert_float_close(mean, out["mean"], what="mean")
    helpers.assert_float_close(rstd, out["rstd"], what="rstd")
    helpers.assert_float_close(y, out["y"], what="y")
    if n >= 2:
        naive = ref.naive_f32_rstd(d["x"])
        assert (np.abs(naive - out["rstd"]) / out["rstd"]).max() > 1e-4   # (element-wise: assert_float_close's second half)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_gate_band_share_is_small(shape):
    """|pre| <= 1e-5 max|pre| holds for at most 1e-3 of the elements: the cap the GPU backward test relies on."""
    n, c = shape
    d = ref.case(n, c)
    out = ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, True)
    assert ref.band_share(out["pre"]) <= 1e-3


def test_slab_plan_of_the_restatement():
    assert ref.slab_rows(256) == 256 and ref.slab_rows(257) == 128 and ref.slab_rows(128 * 64) == 128
    assert ref.slab_rows(128 * 64 + 1) == 160 and ref.slab_rows(20000) == 320
    for n in (257, 1000, 4099, 8193, 20000, 100000, 131072):
        assert -(-n // ref.slab_rows(n)) <= ref.MAX_SLABS
    assert ref.row_lanes(1) == 256 and ref.row_lanes(3) == 64 and ref.row_lanes(16) == 64 and ref.row_lanes(64) == 32
    assert ref.row_lanes(33) == 8 and ref.row_lanes(130) == 8


# ------------------------------------------------------------------------------------------------- VariableStore(fused=True) on the CPU
def _glue_outputs(fused):
    import mccnn_amd.MCNetworkUtils as U
    st = U.VariableStore(fused=fused)
    torch.manual_seed(11)
    x = torch.randn(40, 12)
    outs = [U.batch_norm_RELU_drop_out("A", x, True, True, 0.6, st),
            U.MLP_2_hidden(x, 12, 10, 8, 5, "M2", 0.5, True, useDropOut=True, store=st),
            U.MLP_1_hidden(x, 12, 9, 4, "M1", 0.5, True, useDropOut=True, store=st),
            U.batch_norm_RELU_drop_out("A", x, False, True, 0.6, st)]
    return st, outs


def test_fused_store_on_cpu_tensors_is_the_torch_path():
    st0, o0 = _glue_outputs(False)
    st1, o1 = _glue_outputs(True)
    assert st1.fused_ is True and st0.fused_ is False and st1.dropSeed_ == 0
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    assert st1.dropCalls_ == 0
    sd0, sd1 = st0.state_dict(), st1.state_dict()
    assert list(sd0.keys()) == list(sd1.keys())
    for k in sd0:
        assert sd0[k].shape == sd1[k].shape and torch.equal(sd0[k], sd1[k]), k
    st1.fused_ = False   # may be reassigned at any time
    assert "A_BN/gamma" in sd1 and "M2_BN_Init/moving_variance" in sd1 and "M1_BN_h/beta" in sd1


def test_default_store_has_the_switch_off():
    import mccnn_amd.MCNetworkUtils as U
    assert U.VariableStore().fused_ is False and U.get_default_store().fused_ is False
    assert U.VariableStore("cpu", True).fused_ is True


# ------------------------------------------------------------------------------------------------- argument errors, ABI
def test_argument_errors_launch_nothing():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 18
    before = lib.mccnn_debug_launch_count()
    x, g, b, mm, mv = torch.zeros(6, 4), torch.ones(4), torch.zeros(4), torch.zeros(4), torch.ones(4)
    bad = [dict(x=x.double()), dict(x=torch.zeros(4, 6).t()), dict(gamma=g.double()), dict(movingVar=torch.ones(8)[::2]),
           dict(keepProb=0.0), dict(keepProb=1.5), dict(keepProb=-0.1), dict(keepProb=float("nan")),
           dict(seed=-1), dict(seed=1 << 32), dict(seed=0.5)]
    for kw in bad:
        args = dict(x=x, gamma=g, beta=b, movingMean=mm, movingVar=mv, training=True, keepProb=0.5, seed=1)
        args.update(kw)
        with pytest.raises(M.InvalidArgumentError):
            M.bn_relu_dropout(**args)
    assert lib.mccnn_debug_launch_count() == before


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 4096   # never dereferenced on the host: every call below returns before a launch
    T = 1 << 32
    fwd = lambda **k: lib.mccnn_bn_act_fwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("n", 300), ("c", 8), ("gamma", p), ("beta", p), ("mm", p), ("mv", p), ("mom", 0.99), ("eps", 1e-3),
        ("training", 1), ("relu", 1), ("T", T), ("scale", 1.0), ("seed", 0), ("y", p), ("saved", p), ("ws", p),
        ("wsb", 1 << 20), ("stream", None))])
    bwd = lambda **k: lib.mccnn_bn_act_bwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", p), ("dy", p), ("n", 300), ("c", 8), ("gamma", p), ("beta", p), ("saved", p), ("relu", 1), ("T", T),
        ("scale", 1.0), ("seed", 0), ("dx", p), ("dgamma", p), ("dbeta", p), ("ws", p), ("wsb", 1 << 20), ("stream", None))])
    BADARG, WORKSPACE = -1, -4
    for call in (fwd, bwd):
        assert call(n=0) == BADARG and call(c=0) == BADARG and call(T=0) == BADARG and call(T=T + 1) == BADARG
        assert call(x=None) == BADARG and call(gamma=None) == BADARG and call(saved=None) == BADARG
        assert call(wsb=16) == WORKSPACE and call(ws=None) == WORKSPACE
    assert fwd(y=None) == BADARG and fwd(mm=None) == BADARG
    assert bwd(dy=None) == BADARG and bwd(dgamma=None) == BADARG and bwd(dbeta=None) == BADARG
    assert lib.mccnn_bn_act_workspace_bytes(256, 8) == 0
    need = lib.mccnn_bn_act_workspace_bytes(300, 8)
    assert need >= 3 * 3 * 8 * 4 and fwd(wsb=need - 1) == WORKSPACE
    assert lib.mccnn_debug_launch_count() == before


def test_header_binding_and_library_agree():
    import re
    from mccnn_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_bn_act_workspace_bytes", "mccnn_bn_act_fwd", "mccnn_bn_act_bwd"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    assert "bn_act.hip" in build.SOURCES
