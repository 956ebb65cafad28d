"""The cosine-distance loss of normal estimation as one op (cosine_distance_loss) without a GPU: the float64 reference pinned
against torch's autograd, the ABI and the argument errors of the three C entries, the checks of the Python op, and the CPU
route of VariableStore(fusedLoss=True), MCNetworkUtils.cosine_distance_loss and MCNormS(normals=...)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosine_ref as ref  # noqa: E402

CASES = [(s, wts) for s in ref.SHAPES for wts in (False, True)]
CASE_IDS = ["%dx%d%s" % (s + ("-weights" if wts else "",)) for s, wts in CASES]


def _torch_f64(pred, target, rw):
    """The definition in float64 torch -> (loss, per-row cos): clamp_min has gradient 0 below the clamp, which is what makes the
    unit row linear in pred there."""
    t = torch.tensor(target, dtype=torch.float64)
    u = pred / torch.sqrt((pred * pred).sum(1, keepdim=True).clamp_min(float(ref.EPS)))
    v = t / torch.sqrt((t * t).sum(1, keepdim=True).clamp_min(float(ref.EPS)))
    cos = (u * v).sum(1)
    rows = 1.0 - cos
    live = torch.ones(len(cos), dtype=torch.bool)
    if rw is not None:
        w = torch.tensor(rw, dtype=torch.float64)
        live = w != 0
        rows = rows * w
    return torch.where(live, rows, torch.zeros_like(rows)).sum() / max(int(live.sum()), 1), cos, u, v, live


@pytest.mark.parametrize("shape,wts", CASES, ids=CASE_IDS)
def test_reference_equals_torch_autograd(shape, wts):
    """Forward and dpred against float64 torch: tf.losses.cosine_distance over two l2_normalize'd tensors, spelled out. The
    angle is checked against acos(cos) where that is well conditioned (|cos| <= 0.9, no clamped row) and at the exact rows."""
    n, c = shape
    d = ref.case(n, c)
    rw = d["rw"] if wts else None
    out = ref.forward(d["pred"], d["target"], rw)
    got = ref.backward(d["pred"], d["target"], rw, g=0.75)
    p = torch.tensor(d["pred"], dtype=torch.float64, requires_grad=True)
    loss, cos, u, v, live = _torch_f64(p, d["target"], rw)
    (0.75 * loss).backward()
    live = live.numpy()
    assert out["D"] == max(int(live.sum()), 1) and np.array_equal(out["live"], live)
    assert abs(out["loss"] - float(loss.detach())) <= 1e-10 * max(1.0, abs(float(loss.detach())))
    cosn = cos.detach().numpy()
    assert np.abs(out["cos"] - cosn).max() <= 1e-12
    assert abs(out["cosSum"] - cosn[live].sum()) <= 1e-10 * max(1.0, np.abs(cosn[live]).sum())
    mid = (np.abs(cosn) <= 0.9) & ~d["clamped"] & d["target"].any(1)   # (both rows of unit length: only there is it acos)
    assert np.abs(out["angle"][mid] - np.arccos(cosn[mid])).max(initial=0.0) <= 1e-10
    assert abs(out["angleSum"] - out["angle"][live].sum()) <= 1e-10 * max(1.0, out["angleAbs"])
    k = np.arange(n)
    assert not out["angle"][k % 8 == 1].any()                                        # exactly parallel: exactly 0
    assert np.all(out["angle"][k % 8 == 2] == np.pi)                                 # exactly opposite
    zero_t = ~d["target"].any(1)
    assert np.all(out["cos"][zero_t] == 0) and np.all(out["angle"][zero_t] == np.pi / 2)   # a zero target: cos = 0
    # the clamped rows' slope is 1 / sqrt(eps) for autograd and the op's constant 1e6f in the reference: they differ by 2e-9
    want = p.grad.numpy()
    cl = d["clamped"]
    terms = ref.backward_terms(d["pred"], d["target"], rw, g=0.75)
    for rows, tol in ((~cl, 1e-10), (cl, 1e-8)):
        if rows.any():
            assert np.abs(got[rows] - want[rows]).max() <= tol * ref.grad_scale(want, terms, rows, c), (rows.sum(), tol)
    if wts and n >= 8:
        assert not live[7] and not got[7].any() and not want[7].any()
    if n >= 64:
        # (why the two sets are held to their own scales: 1e6 against 1 / |pred| <= 1e3)
        assert cl.any() and (~cl).any() and np.abs(terms[cl]).max() > 100 * np.abs(terms[~cl]).max()


def test_no_live_row_gives_zero_not_nan():
    d = ref.case(64, 3)
    rw = np.zeros(64, np.float32)
    out = ref.forward(d["pred"], d["target"], rw)
    g = ref.backward(d["pred"], d["target"], rw, g=2.0)
    assert out["loss"] == 0.0 and not np.signbit(out["loss"]) and out["D"] == 1 and out["cosSum"] == 0.0 and out["angleSum"] == 0.0
    assert not g.any() and not np.isnan(g).any()


# ------------------------------------------------------------------------------------------------- ABI, argument errors
def test_abi_version():
    from mccnn_amd import _lib
    assert _lib.load().mccnn_abi_version() >= 24


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 0x7f0000000000   # a made-up address: never dereferenced, every call below returns before a launch
    fwd = lambda **k: lib.mccnn_cosine_loss_fwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("pred", p), ("target", p), ("n", 300), ("c", 3), ("rw", p), ("loss", p), ("sums", p), ("meta", p), ("ws", p),
        ("wsb", 1 << 20), ("stream", None))])
    bwd = lambda **k: lib.mccnn_cosine_loss_bwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("pred", p), ("target", p), ("n", 300), ("c", 3), ("rw", p), ("meta", p), ("g", p), ("dpred", p), ("stream", None))])
    BADARG, TOOLARGE, WORKSPACE = -1, -3, -4
    for call in (fwd, bwd):
        assert call(n=0) == BADARG and call(c=0) == BADARG and call(n=-5) == BADARG and call(c=-1) == BADARG
        for name in ("pred", "target", "meta"):
            assert call(**{name: None}) == BADARG, name
        assert call(n=1 << 30, c=2) == TOOLARGE and call(n=(1 << 31) - 1, c=3) == TOOLARGE and call(n=65536, c=32768) == TOOLARGE
    for name in ("loss", "sums"):
        assert fwd(**{name: None}) == BADARG, name
    assert bwd(g=None) == BADARG and bwd(dpred=None) == BADARG
    need = lib.mccnn_cosine_loss_workspace_bytes(300, 3)
    assert need > 0 and fwd(wsb=need - 1) == WORKSPACE and fwd(ws=None) == WORKSPACE and fwd(wsb=0) == WORKSPACE
    assert lib.mccnn_debug_launch_count() == before


def test_workspace_query():
    """0 up to 256 rows (one launch: no partials), positive above, 0 for sizes the op refuses; modest whatever n is."""
    from mccnn_amd import _lib
    q = _lib.load().mccnn_cosine_loss_workspace_bytes
    for c in (1, 3, 17):
        assert q(1, c) == 0 and q(255, c) == 0 and q(256, c) == 0
        assert q(257, c) > 0 and q(4099, c) > 0 and q(131072, c) >= q(4099, c)
        assert q(131072, c) <= 4 * 1024 * 4 + 256
    assert q(0, 3) == 0 and q(3, 0) == 0 and q(-1, 3) == 0 and q(300, -2) == 0
    assert q(1 << 30, 2) == 0 and q((1 << 31) - 1, 3) == 0 and q(65536, 32768) == 0
    assert 0 < q((1 << 31) - 1, 1) <= 4 * 1024 * 4 + 256


def test_header_binding_and_library_agree():
    import re
    import subprocess
    from mccnn_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_cosine_loss_workspace_bytes", "mccnn_cosine_loss_fwd", "mccnn_cosine_loss_bwd"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    assert len(_lib.SIGNATURES["mccnn_cosine_loss_fwd"][1]) == 11 and len(_lib.SIGNATURES["mccnn_cosine_loss_bwd"][1]) == 9
    assert "cosine_loss.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "cosine_loss.hip"))


# ------------------------------------------------------------------------------------------------- the Python op
def test_op_argument_errors_launch_nothing():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, dense_glue, native
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    assert M.cosine_distance_loss is dense_glue.cosine_distance_loss and M._cosine_loss_args is dense_glue._cosine_loss_args
    p, t, rw = torch.zeros(6, 3), torch.zeros(6, 3), torch.ones(6)
    bad = [(dict(pred=p.double()), "pred must be a float32 tensor"), (dict(target=t.double()), "target must be a float32 tensor"),
           (dict(pred=[0.0] * 6), "pred must be a float32 tensor"),
           (dict(pred=torch.zeros(6)), r"expects pred \(n, c\) and target \(n, c\)"),
           (dict(target=torch.zeros(5, 3)), r"expects pred \(n, c\) and target \(n, c\)"),
           (dict(pred=torch.zeros(0, 3), target=torch.zeros(0, 3)), r"expects pred \(n, c\)"),
           (dict(pred=torch.zeros(3, 6).t()), "pred and target must be contiguous"),
           (dict(target=torch.zeros(6, 6)[:, :3]), "pred and target must be contiguous"),
           (dict(target=torch.zeros(6, 3, requires_grad=True)), "no gradient with respect to target"),
           (dict(weights=rw.double()), "weights must be a float32 tensor"), (dict(weights=torch.ones(7)), "weights must have shape"),
           (dict(weights=torch.ones(1, 6)), "weights must have shape"), (dict(weights=torch.ones(12)[::2]), "weights must be contiguous"),
           (dict(weights=torch.ones(6, requires_grad=True)), "no gradient with respect to weights"),
           (dict(), "pred must be a CUDA tensor"), (dict(weights=torch.ones(6, 1)), "pred must be a CUDA tensor")]
    for op in (M.cosine_distance_loss, native.cosine_distance_loss):
        for kw, text in bad:   # (the last two: everything in order but on the CPU)
            args = dict(pred=p, target=t)
            args.update(kw)
            with pytest.raises(M.InvalidArgumentError, match="cosine_distance_loss.*" + text):
                op(**args)
    assert lib.mccnn_debug_launch_count() == before
    doc = M.cosine_distance_loss.__doc__
    assert "NOT" in doc and "differentiable" in doc and "atan2" in doc


# ------------------------------------------------------------------------------------------------- the helper on the CPU
def _check_head(head, d, rw, grad=None, g=1.0):
    import mccnn_amd.MCNetworkUtils as U
    want = ref.forward(d["pred"], d["target"], rw)
    assert isinstance(head, U.NormalHead) and head._fields == ("loss", "cosSum", "angleSum", "denom")
    assert head.loss.dim() == 0 and head.loss.dtype == torch.float32 and head.loss.requires_grad
    for t in (head.cosSum, head.angleSum, head.denom):
        assert t.dim() == 0 and not t.requires_grad
    assert head.denom.dtype == torch.int32 and int(head.denom) == want["D"]
    assert abs(float(head.loss.detach()) - want["loss"]) <= 1e-4 * max(want["lossAbs"], 1.0)
    assert abs(float(head.cosSum) - want["cosSum"]) <= 1e-4 * max(want["cosAbs"], 1.0)
    assert abs(float(head.angleSum) - want["angleSum"]) <= 1e-4 * max(want["angleAbs"], 1.0)
    if grad is not None:
        wg = ref.backward(d["pred"], d["target"], rw, g=g)
        terms = ref.backward_terms(d["pred"], d["target"], rw, g=g)
        for rows in (d["clamped"], ~d["clamped"]):   # each against its own scale: a clamped row's gradient is 1e6 times larger
            if rows.any():
                assert np.abs(grad[rows] - wg[rows]).max() <= 1e-4 * ref.grad_scale(wg, terms, rows, d["pred"].shape[1])
        assert not grad[~want["live"]].any()


@pytest.mark.parametrize("fusedLoss", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("shape,wts", CASES, ids=CASE_IDS)
def test_helper_on_cpu_tensors(shape, wts, fusedLoss):
    """MCNetworkUtils.cosine_distance_loss on CPU tensors: the reference's loss, sums, D and gradient with the switch off AND on
    (on the CPU, on falls back to the torch code)."""
    import mccnn_amd.MCNetworkUtils as U
    d = ref.case(*shape)
    st = U.VariableStore(fusedLoss=fusedLoss)
    p = torch.from_numpy(d["pred"]).requires_grad_(True)
    weights = torch.from_numpy(d["rw"]).reshape(-1, 1) if wts else None
    assert U._fused_cosine(st, p, torch.from_numpy(d["target"]), weights) is None
    head = U.cosine_distance_loss(p, torch.from_numpy(d["target"]), weights, store=st)
    (0.37 * head.loss).backward()
    _check_head(head, d, d["rw"] if wts else None, p.grad.numpy(), g=0.37)


def test_no_live_row_through_the_helper_on_cpu():
    import mccnn_amd.MCNetworkUtils as U
    d = ref.case(63, 3)
    p = torch.from_numpy(d["pred"]).requires_grad_(True)
    head = U.cosine_distance_loss(p, torch.from_numpy(d["target"]), torch.zeros(63), store=U.VariableStore(fusedLoss=True))
    head.loss.backward()
    assert float(head.loss.detach()) == 0.0 and not math.copysign(1.0, float(head.loss.detach())) < 0
    assert int(head.denom) == 1 and float(head.cosSum) == 0.0 and float(head.angleSum) == 0.0
    assert not p.grad.any() and not torch.isnan(p.grad).any()


def test_angles_of_a_hand_computed_case():
    """Three rows: parallel, orthogonal, opposite -- cos 1, 0, -1 and angles 0, pi / 2, pi. mean_angle = pi / 2; the
    reference's figure is acos of the mean over all nine ELEMENTS of u * v, acos(0 / 9) = pi / 2 here, and acos(1 / 3) for the
    first row alone (its own angle is 0)."""
    import mccnn_amd.MCNetworkUtils as U
    p = torch.tensor([[2.0, 0, 0], [0, 3.0, 0], [0, 0, -0.5]])
    t = torch.tensor([[1.0, 0, 0], [1.0, 0, 0], [0, 0, 4.0]])
    head = U.cosine_distance_loss(p, t)
    assert float(head.loss) == 1.0 and float(head.cosSum) == 0.0 and int(head.denom) == 3
    assert abs(float(head.angleSum) - 1.5 * math.pi) <= 1e-6
    assert abs(float(U.mean_angle(head)) - math.pi / 2) <= 1e-6
    assert abs(float(U.reference_angle(head, 3)) - math.pi / 2) <= 1e-6
    one = U.cosine_distance_loss(p[:1], t[:1])
    assert float(U.mean_angle(one)) == 0.0 and abs(float(U.reference_angle(one, 3)) - math.acos(1.0 / 3.0)) <= 1e-6
    two = U.cosine_distance_loss(p, t, torch.tensor([1.0, 0.0, 2.0]))   # rows 0 and 2: loss (0 + 2 * 2) / 2
    assert int(two.denom) == 2 and float(two.loss) == 2.0 and abs(float(U.mean_angle(two)) - math.pi / 2) <= 1e-6


def test_mcnorm_s_takes_the_switch_and_normals(oracle):
    """The example network on the CPU path (oracle ops): the constructor argument reaches the store, forward() with normals
    returns the NormalHead over the prediction that forward() without them returns, unchanged."""
    import inspect
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import mcclass_s
    import mccnn_amd.MCNetworkUtils as U
    from tests.oracle_ops import OracleOps
    rng = np.random.default_rng(4)
    B, n = 2, 48
    P = torch.from_numpy(rng.random((B * n, 3), dtype=np.float32))
    Bi = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), n).reshape(-1, 1))
    F = torch.ones((B * n, 1))
    N = torch.from_numpy(rng.standard_normal((B * n, 3)).astype(np.float32))
    W = torch.from_numpy((rng.random(B * n) > 0.3).astype(np.float32))
    assert mcclass_s.MCNormS(1, B, 8, torch.device("cpu")).store.fusedLoss_ is False
    heads = []
    for fusedLoss in (False, True):
        torch.manual_seed(5)
        net = mcclass_s.MCNormS(1, B, 8, torch.device("cpu"), ops=OracleOps(oracle), fusedLoss=fusedLoss)
        assert net.store.fusedLoss_ is fusedLoss
        pred = net(P, Bi, F, True)
        assert torch.is_tensor(pred) and pred.shape == (B * n, 3) and pred.requires_grad
        head = net(P, Bi, F, True, normals=N, normalWeights=W)
        assert isinstance(head, U.NormalHead)
        want = U._normal_head(net(P, Bi, F, True), N, W)
        assert torch.equal(head.loss.detach(), want.loss.detach()) and torch.equal(head.angleSum, want.angleSum)
        assert int(head.denom) == int((W != 0).sum())
        head.loss.backward()
        assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in net.convBuilder.parameters())
        heads.append(head)
    assert torch.equal(heads[0].loss.detach(), heads[1].loss.detach())
    sig = inspect.signature(mcclass_s.MCNormS.forward).parameters
    assert sig["normals"].default is None and sig["normalWeights"].default is None
    src = inspect.getsource(mcclass_s.main)
    assert "--normals" in src and "mean_angle" in inspect.getsource(mcclass_s.train_normals)
