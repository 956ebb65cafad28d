"""The optimiser step as one op (mccnn_adam_step, mccnn_amd.optim.FusedAdam) without a GPU: the float64 reference pinned
against float64 torch.optim.Adam, the 'tf' form by hand, the ABI and the argument errors of the C entry, and FusedAdam on CPU
parameters (the same definition in torch) against torch.optim.Adam."""
import argparse
import copy
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
LR = 1e-3


class Rec(C.Structure):   # mccnn_adam_tensor (include/mccnn.h)
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int), ("step_size", C.c_float),
                ("bc2_sqrt", C.c_float), ("weight_decay", C.c_float)]


# ------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["plain", "decay"])
def test_reference_equals_float64_torch_adam(wd):
    """Form 'torch' over 5 steps against torch.optim.Adam on float64 tensors, everything (betas, scalars) in double: 1e-12
    relative to |p| + lr."""
    n = 1000
    p0, _ = ref.inputs(n, 1, wd != 0)
    q = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([q], lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        _, g = ref.inputs(n, 10 + t, wd != 0)
        q.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        ss, bs = ref.scalars("torch", LR, 0.9, 0.999, t, round32=False)
        out = ref.step(p, g, m, v, ss, bs, wd, 0.9, 0.999, 1e-8, 1.0)
        p, m, v = out["p"], out["m"], out["v"]
        assert np.abs(p - q.detach().numpy()).max() <= 1e-12 * (np.abs(p).max() + LR)
        assert np.all(np.abs(p - q.detach().numpy()) <= 1e-12 * (np.abs(p) + LR))
    st = opt.state[q]
    assert np.all(np.abs(m - st["exp_avg"].numpy()) <= 1e-12 * (np.abs(m) + 1e-30))
    assert np.all(np.abs(v - st["exp_avg_sq"].numpy()) <= 1e-12 * (np.abs(v) + 1e-30))


def test_tf_form_on_a_hand_computed_case():
    """t = 1 from zero moments with lr 0.1, beta1 0.5, beta2 0.75, eps 0.5, g = (2, -4, 0): m' = g / 2 = (1, -2, 0),
    v' = g^2 / 4 = (1, 4, 0). 'tf': step_size = 0.1 sqrt(0.25) / 0.5 = 0.1, den = sqrt(v') + 0.5 = (1.5, 2.5, 0.5),
    p' = p - 0.1 (1 / 1.5, -2 / 2.5, 0). 'torch' differs: step_size 0.2, den = sqrt(v') / 0.5 + 0.5 = (2.5, 4.5, 0.5)."""
    from mccnn_amd.optim import FusedAdam
    p0, g = np.array([1.0, 2.0, 3.0]), np.array([2.0, -4.0, 0.0])
    hand = {"tf": p0 - 0.1 * np.array([1 / 1.5, -2 / 2.5, 0.0]), "torch": p0 - 0.2 * np.array([1 / 2.5, -2 / 4.5, 0.0])}
    assert ref.scalars("tf", 0.1, 0.5, 0.75, 1, round32=False) == (0.1 * 0.5 / 0.5, 1.0)
    assert ref.scalars("torch", 0.1, 0.5, 0.75, 1, round32=False) == (0.2, 0.5)
    for form in ref.FORMS:
        ss, bs = ref.scalars(form, 0.1, 0.5, 0.75, 1, round32=False)
        out = ref.step(p0, g, np.zeros(3), np.zeros(3), ss, bs, 0.0, 0.5, 0.75, 0.5, 1.0)
        assert np.array_equal(out["m"], [1.0, -2.0, 0.0]) and np.array_equal(out["v"], [1.0, 4.0, 0.0])
        assert np.abs(out["p"] - hand[form]).max() <= 1e-15
        q = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float32))
        opt = FusedAdam([q], lr=0.1, betas=(0.5, 0.75), eps=0.5, form=form)
        q.grad = torch.tensor(g, dtype=torch.float32)
        opt.step()
        assert np.abs(q.detach().numpy() - hand[form]).max() <= 4 * ref.E * 3.0
        assert torch.equal(opt.state[q]["exp_avg"], torch.tensor([1.0, -2.0, 0.0]))
        assert torch.equal(opt.state[q]["exp_avg_sq"], torch.tensor([1.0, 4.0, 0.0]))
    assert np.abs(hand["tf"] - hand["torch"]).max() > 1e-2


@pytest.mark.parametrize("form", ref.FORMS)
def test_the_float32_definition_stays_inside_the_bars(form):
    """The CPU route (_adam_torch: the definition in float32 torch, separate multiply and add) against the reference's bars, so
    the bars of the GPU tests are known to be reachable: one step at t = 2 from the reference's previous step, with decay and
    a gradient scale."""
    from mccnn_amd.optim import _adam_torch
    for wd, gs in ((0.0, 1.0), (1e-2, 0.25)):
        d = ref.case(30000, 5, form, wd, gs, 2)
        p, g, m, v = (torch.from_numpy(d[k].copy()) for k in ("p", "g", "m", "v"))
        _adam_torch(p, g, m, v, d["step_size"], d["bc2_sqrt"], d["weight_decay"], d["beta1"], d["beta2"], d["eps"], d["grad_scale"])
        shares = ref.worst(p.numpy(), m.numpy(), v.numpy(), d["want"])
        print("float32 torch uses %.2f of tol_p, %.2f of tol_m, %.2f of tol_v (%s, wd %g, scale %g)" % (shares + (form, wd, gs)))
        assert max(shares) <= 1.0 / 3.0   # (a third: the reference alone leaves a factor of three)


# ------------------------------------------------------------------------------------------------- ABI, argument errors
def test_abi_version():
    from mccnn_amd import _lib
    assert _lib.load().mccnn_abi_version() >= 27


def test_capacity_and_record_layout():
    from mccnn_amd import _lib, optim
    cap = _lib.load().mccnn_adam_max_tensors()
    assert C.sizeof(Rec) == 48 == optim.RECORD.itemsize
    for name, _ in Rec._fields_:
        assert getattr(Rec, name).offset == optim.RECORD.fields[name][1], name
    assert 16 <= cap and cap * C.sizeof(Rec) + (cap + 1) * 4 < 4096   # records and the workgroup prefix: under 4 KB of arguments
    src = open(os.path.join(ROOT, "mccnn_amd", "csrc", "adam.hip")).read()
    assert int(re.search(r"kAdamChunk = (\d+);", src).group(1)) == optim.CHUNK
    assert int(re.search(r"kAdamMax = (\d+);", src).group(1)) == cap
    assert "static_assert(sizeof(AdamArgs) < 4096" in src


def _records(specs):
    arr = (Rec * len(specs))()
    for r, s in zip(arr, specs):
        d = dict(p=0x7f0000000000, g=0x7f0000100000, m=0x7f0000200000, v=0x7f0000300000, n=100, step_size=1e-3, bc2_sqrt=0.5,
                 weight_decay=0.0)   # made-up addresses: never dereferenced, every call below returns before a launch
        d.update(s)
        for k, val in d.items():
            setattr(r, k, val)
    return arr


def test_c_abi_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()

    def call(specs, count=None, **k):
        arr = _records(specs)
        a = dict(beta1=0.9, beta2=0.999, eps=1e-8, gs=1.0)
        a.update(k)
        return lib.mccnn_adam_step(C.addressof(arr) if "arr" not in k else k["arr"], len(specs) if count is None else count,
                                   a["beta1"], a["beta2"], a["eps"], a["gs"], None)
    inf, nan = float("inf"), float("nan")
    assert call([{}], count=-1) == BADARG
    assert call([{}], arr=None) == BADARG
    assert call([{}, {"n": -1}]) == BADARG
    for name in ("p", "g", "m", "v"):
        assert call([{}, {name: None}]) == BADARG, name
        for low in (1, 2, 3):
            assert call([{name: 0x7f0000000000 + low}]) == BADARG, (name, low)
    for b in (-0.1, 1.0, 1.5, inf, nan):
        assert call([{}], beta1=b) == BADARG and call([{}], beta2=b) == BADARG, b
    for e in (-1e-8, inf, nan):
        assert call([{}], eps=e) == BADARG, e
    for s in (inf, -inf, nan):
        assert call([{}], gs=s) == BADARG
        assert call([{"step_size": s}]) == BADARG and call([{"weight_decay": s}]) == BADARG and call([{"bc2_sqrt": s}]) == BADARG
    assert call([{"bc2_sqrt": 0.0}]) == BADARG and call([{"bc2_sqrt": -0.5}]) == BADARG
    # a bad record behind good ones, and behind more than one launch's worth of them, still stops the whole call
    cap = lib.mccnn_adam_max_tensors()
    assert call([{}] * (cap + 2) + [{"n": -3}]) == BADARG
    assert lib.mccnn_debug_launch_count() == before


def test_nothing_to_do_is_ok_and_launches_nothing():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    assert lib.mccnn_adam_step(None, 0, 0.9, 0.999, 1e-8, 1.0, None) == 0
    arr = _records([{"n": 0, "p": None, "g": 0x3, "m": 0x5, "v": None, "bc2_sqrt": 0.0, "step_size": float("nan")}] * 5)
    assert lib.mccnn_adam_step(C.addressof(arr), 5, 0.9, 0.999, 1e-8, 1.0, None) == 0   # (n == 0: nothing of it is looked at)
    assert lib.mccnn_debug_launch_count() == before


def test_header_binding_and_library_agree():
    from mccnn_amd import _lib, build
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ("mccnn_adam_max_tensors", "mccnn_adam_step"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES and name in exported
    assert len(_lib.SIGNATURES["mccnn_adam_step"][1]) == 7 and _lib.SIGNATURES["mccnn_adam_max_tensors"][1] == []
    rec = re.search(r"typedef struct \{([^}]*)\} mccnn_adam_tensor;", code).group(1)
    assert re.findall(r"(\w+);", rec) == [n for n, _ in Rec._fields_]
    assert "adam.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "adam.hip"))
    text = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    assert "cannot check that the arrays of a call do not overlap" in text


# ------------------------------------------------------------------------------------------------- FusedAdam on the CPU
SHAPES = [(3,), (8, 16), (5, 7), (1,), (33, 4), (129,)]


def _twins(seed=0, shapes=SHAPES):
    torch.manual_seed(seed)
    ps = [torch.randn(s) for s in shapes]
    return [torch.nn.Parameter(p.clone()) for p in ps], [torch.nn.Parameter(p.clone()) for p in ps]


def _feed(a, b, seed, skip=()):
    gen = torch.Generator().manual_seed(seed)
    for i, (x, y) in enumerate(zip(a, b)):
        g = torch.randn(x.shape, generator=gen)
        x.grad, y.grad = (None, None) if i in skip else (g.clone(), g.clone())


def _share(a, b, lr=LR):
    """The largest share of 64 e (|p| + lr) between two parameter lists."""
    return max(float(((x.detach() - y.detach()).abs() / (64 * ref.E * (y.detach().abs() + lr))).max()) for x, y in zip(a, b))


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["plain", "decay"])
def test_fused_adam_on_cpu_against_torch_adam(wd):
    from mccnn_amd.optim import FusedAdam
    a, b = _twins()
    oa, ob = FusedAdam(a, lr=LR, weightDecay=wd), torch.optim.Adam(b, lr=LR, weight_decay=wd)
    for s in range(5):
        _feed(a, b, 100 + s)
        assert oa.step() is None
        ob.step()
        assert _share(a, b) <= 1.0, s
    for x, y in zip(a, b):
        sa, sb = oa.state[x], ob.state[y]
        assert set(sa) == {"step", "exp_avg", "exp_avg_sq"} == set(sb)
        assert sa["step"].dtype == torch.float32 and sa["step"].dim() == 0 and sa["step"].device.type == "cpu" and float(sa["step"]) == 5
        assert sa["exp_avg"].shape == x.shape and sa["exp_avg_sq"].shape == x.shape
        assert sa["exp_avg"].data_ptr() % 16 == 0 and sa["exp_avg_sq"].data_ptr() % 16 == 0
    # the moments of one first step are views of ONE buffer each
    assert len({oa.state[x]["exp_avg"].untyped_storage().data_ptr() for x in a}) == 1
    assert oa.step(lambda: torch.tensor(2.5)) == torch.tensor(2.5)


def test_grad_scale_equals_prescaled_gradients():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(1)
    oa, ob = FusedAdam(a, lr=LR, gradScale=0.25), torch.optim.Adam(b, lr=LR)
    for s in range(5):
        _feed(a, b, 200 + s)
        for y in b:
            y.grad.mul_(0.25)
        oa.step()
        ob.step()
    assert _share(a, b) <= 1.0


def test_decay_params_decays_exactly_the_named_tensors():
    """decayParams against a two-group torch Adam; and against decay on everything, which must differ on the others."""
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(2)
    named = [0, 2, 5]
    oa = FusedAdam(a, lr=LR, weightDecay=0.1, decayParams=[a[i] for i in named])
    ob = torch.optim.Adam([{"params": [b[i] for i in named], "weight_decay": 0.1},
                           {"params": [y for i, y in enumerate(b) if i not in named], "weight_decay": 0.0}], lr=LR)
    c, _ = _twins(2)
    oc = FusedAdam(c, lr=LR, weightDecay=0.1)
    for s in range(5):
        _feed(a, b, 300 + s)
        for x, z in zip(a, c):
            z.grad = x.grad.clone()
        oa.step()
        ob.step()
        oc.step()
    assert _share(a, b) <= 1.0
    for i, (x, z) in enumerate(zip(a, c)):
        assert torch.equal(x, z) == (i in named), i


def test_a_parameter_without_a_gradient_is_left_alone():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(3)
    oa, ob = FusedAdam(a, lr=LR), torch.optim.Adam(b, lr=LR)
    keep = a[2].detach().clone()
    for s in range(3):
        _feed(a, b, 400 + s, skip=(2,))
        oa.step()
        ob.step()
    assert torch.equal(a[2], keep) and a[2] not in oa.state and len(oa.state) == len(a) - 1
    assert _share(a, b) <= 1.0
    # ... and joins later with a step count of its own, as in torch
    for s in range(2):
        _feed(a, b, 410 + s)
        oa.step()
        ob.step()
    assert float(oa.state[a[2]]["step"]) == 2 and float(oa.state[a[0]]["step"]) == 5
    assert _share(a, b) <= 1.0
    _feed(a, b, 420, skip=range(len(a)))
    oa.step()                                  # no gradient anywhere: nothing happens
    assert float(oa.state[a[0]]["step"]) == 5


def test_lr_assigned_between_steps_and_a_scheduler():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(4)
    oa, ob = FusedAdam(a, lr=1e-2), torch.optim.Adam(b, lr=1e-2)
    for s in range(4):
        for o in (oa, ob):
            o.param_groups[0]["lr"] = max(1e-2 * 0.5 ** s, 2e-3)   # (the reference's staircase decay with a floor)
        _feed(a, b, 500 + s)
        oa.step()
        ob.step()
    assert _share(a, b, 2e-3) <= 1.0
    sa, sb = torch.optim.lr_scheduler.StepLR(oa, 2, 0.1), torch.optim.lr_scheduler.StepLR(ob, 2, 0.1)
    before = [x.detach().clone() for x in a]
    for s in range(4):
        _feed(a, b, 510 + s)
        oa.step()
        ob.step()
        sa.step()
        sb.step()
    assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"] == pytest.approx(2e-5)
    assert _share(a, b, 2e-5) <= 1.0 and not any(torch.equal(x, y) for x, y in zip(a, before))


def test_state_dict_round_trips_with_torch_adam():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(5)
    oa, ob = FusedAdam(a, lr=LR, weightDecay=1e-2), torch.optim.Adam(b, lr=LR, weight_decay=1e-2)
    for s in range(3):
        _feed(a, b, 600 + s)
        oa.step()
        ob.step()
    sda, sdb = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())
    # each optimiser continues from the OTHER one's checkpoint (fresh instances, as after a restart)
    a2, b2 = [torch.nn.Parameter(x.detach().clone()) for x in a], [torch.nn.Parameter(y.detach().clone()) for y in b]
    oa2, ob2 = FusedAdam(a2, lr=5.0), torch.optim.Adam(b2, lr=5.0)
    oa2.load_state_dict(sdb)
    ob2.load_state_dict(sda)
    # (torch's checkpoint has no 'form': the key keeps this instance's default)
    assert oa2.param_groups[0]["lr"] == LR and oa2.param_groups[0]["weight_decay"] == 1e-2 and oa2.param_groups[0]["form"] == "torch"
    assert ob2.param_groups[0]["lr"] == LR and ob2.param_groups[0]["weight_decay"] == 1e-2
    for s in range(2):
        _feed(a2, b2, 610 + s)
        _feed(a, b, 610 + s)
        for o in (oa, ob, oa2, ob2):
            o.step()
    assert float(oa2.state[a2[0]]["step"]) == 5 and float(ob2.state[b2[0]]["step"]) == 5
    assert _share(a2, b) <= 1.0 and _share(b2, b) <= 1.0 and _share(a, b) <= 1.0
    # its own checkpoint, through torch.save's pickling
    import io
    buf = io.BytesIO()
    torch.save(oa.state_dict(), buf)
    buf.seek(0)
    a3 = [torch.nn.Parameter(x.detach().clone()) for x in a]
    oa3 = FusedAdam(a3, lr=LR, weightDecay=1e-2)
    oa3.load_state_dict(torch.load(buf))
    _feed(a3, a, 620)
    oa3.step()
    oa.step()
    assert all(torch.equal(x, y) for x, y in zip(a3, a))


def test_a_deep_copy_and_a_pickle_step_like_the_original():
    import pickle
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(8)
    oa = FusedAdam(a, lr=LR, weightDecay=0.1, decayParams=a[:2], gradScale=0.5)
    _feed(a, b, 800)
    oa.step()
    ob, oc = copy.deepcopy(oa), pickle.loads(pickle.dumps(oa))
    for o in (ob, oc):
        assert o.gradScale == 0.5 and o._decay_ids == {id(p) for p in o.param_groups[0]["params"][:2]}
    gen = torch.Generator().manual_seed(801)
    for i in range(len(a)):
        g = torch.randn(a[i].shape, generator=gen)
        for o in (oa, ob, oc):
            o.param_groups[0]["params"][i].grad = g.clone()
    for o in (oa, ob, oc):
        o.step()
    for x, y, z in zip(a, ob.param_groups[0]["params"], oc.param_groups[0]["params"]):
        assert torch.equal(x, y) and torch.equal(x, z) and x is not y and x is not z
    assert float(ob.state[ob.param_groups[0]["params"][0]]["step"]) == 2 == float(oa.state[a[0]]["step"])


def test_groups_with_their_own_hyper_parameters():
    """Two groups with different betas (separate calls), a third that shares the first one's but does not stand next to it."""
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(6)
    groups = lambda q: [{"params": q[:2]}, {"params": q[2:4], "betas": (0.8, 0.99), "lr": 3e-3}, {"params": q[4:], "weight_decay": 0.05}]  # noqa: E731
    oa, ob = FusedAdam(groups(a), lr=LR), torch.optim.Adam(groups(b), lr=LR)
    for s in range(5):
        _feed(a, b, 700 + s)
        oa.step()
        ob.step()
    assert _share(a, b) <= 1.0


def test_argument_errors_raise_and_launch_nothing():
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import InvalidArgumentError
    from mccnn_amd.optim import FusedAdam
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    q = lambda *s, **k: torch.nn.Parameter(torch.zeros(*(s or (4,)), **k))  # noqa: E731
    for kw, text in [(dict(lr=torch.tensor(1e-3)), "lr must be a Python float, not a tensor"), (dict(lr=-1.0), "invalid lr"),
                     (dict(betas=(0.9, 1.0)), r"betas must be two numbers in \[0, 1\)"), (dict(betas=(-0.1, 0.9)), "betas must be"),
                     (dict(eps=-1e-8), "invalid eps"), (dict(weightDecay=-0.1), "invalid weight_decay"),
                     (dict(form="adamw"), "form must be 'torch' or 'tf'"), (dict(gradScale=float("nan")), "gradScale must be a finite"),
                     (dict(decayParams=[q()]), "decayParams holds something that is not among params")]:
        with pytest.raises(InvalidArgumentError, match="FusedAdam: " + text):
            FusedAdam([q()], **kw)

    def stepped(params, grads, **kw):
        opt = FusedAdam(params, **kw)
        for p, g in zip(params, grads):
            p.grad = g
        return opt

    p = q(4, 3)
    opt = stepped([p], [torch.zeros(4, 3).to_sparse()])
    with pytest.raises(InvalidArgumentError, match="FusedAdam: sparse gradients are not supported"):
        opt.step()
    p = q(dtype=torch.float64)
    with pytest.raises(InvalidArgumentError, match="FusedAdam: parameters must be dense float32 tensors"):
        stepped([p], [torch.zeros(4, dtype=torch.float64)]).step()
    with pytest.raises(InvalidArgumentError, match="FusedAdam: parameters on more than one device"):
        stepped([q(), q(device="meta")], [torch.zeros(4), torch.zeros(4, device="meta")]).step()
    opt = stepped([q()], [torch.ones(4)])
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(InvalidArgumentError, match="FusedAdam: lr must be a Python float, not a tensor"):
        opt.step()
    assert not opt.state and not opt.param_groups[0]["params"][0].any()
    opt = stepped([q()], [torch.ones(4)])
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(InvalidArgumentError, match="FusedAdam: amsgrad, maximize and decoupled weight decay are not covered"):
        opt.step()
    assert lib.mccnn_debug_launch_count() == before


def test_a_non_contiguous_gradient_is_taken_by_value():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(7, [(6, 5)])
    oa, ob = FusedAdam(a, lr=LR), torch.optim.Adam(b, lr=LR)
    g = torch.randn(5, 6).t()
    assert not g.is_contiguous()
    a[0].grad, b[0].grad = g, g.clone()
    oa.step()
    ob.step()
    assert _share(a, b) <= 1.0 and "contiguous" in FusedAdam.__doc__


# ------------------------------------------------------------------------------------------------- the example
def test_example_takes_the_flags_and_moves_every_parameter(oracle):
    """examples/mcclass_s.py: --fused-adam and --weight-decay exist, all three loops make their optimiser through
    make_optimizer, and on the CPU path (oracle ops) one FusedAdam step moves every parameter that has a gradient."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import mcclass_s
    from mccnn_amd.optim import FusedAdam
    from tests.oracle_ops import OracleOps
    src = inspect.getsource(mcclass_s.main)
    assert "--fused-adam" in src and "--weight-decay" in src
    for fn in (mcclass_s.main, mcclass_s.train_normals, mcclass_s.train_parts):
        assert "make_optimizer(net, args)" in inspect.getsource(fn) and "torch.optim.Adam(" not in inspect.getsource(fn)
    rng = np.random.default_rng(4)
    B, n = 2, 48
    P = torch.from_numpy(rng.random((B * n, 3), dtype=np.float32))
    Bi = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), n).reshape(-1, 1))
    F = torch.ones((B * n, 1))
    N = torch.from_numpy(rng.standard_normal((B * n, 3)).astype(np.float32))
    torch.manual_seed(5)
    net = mcclass_s.MCNormS(1, B, 8, torch.device("cpu"), ops=OracleOps(oracle))
    net(P, Bi, F, True)   # creates the variables
    off = mcclass_s.make_optimizer(net, argparse.Namespace(fused_adam=False, weight_decay=0.0))
    assert type(off) is torch.optim.Adam and off.param_groups[0]["lr"] == 5e-3 and off.param_groups[0]["weight_decay"] == 0
    opt = mcclass_s.make_optimizer(net, argparse.Namespace(fused_adam=True, weight_decay=1e-4))
    assert isinstance(opt, FusedAdam) and opt.param_groups[0]["weight_decay"] == 1e-4 and opt.param_groups[0]["lr"] == 5e-3
    decay = net.store.get_collection("weight_decay_loss") + net.convBuilder.get_collection("weight_decay_loss")
    assert len(decay) > 0 and opt._decay_ids == {id(p) for p in decay}
    head = net(P, Bi, F, True, normals=N)
    opt.zero_grad(set_to_none=True)
    head.loss.backward()
    params = list(net.parameters())
    before = [p.detach().clone() for p in params]
    with_grad = [p.grad is not None and bool(p.grad.any()) for p in params]
    assert sum(with_grad) >= 12
    opt.step()
    for p, p0, moved in zip(params, before, with_grad):
        assert bool(torch.isfinite(p).all()) and (not torch.equal(p, p0)) == moved
