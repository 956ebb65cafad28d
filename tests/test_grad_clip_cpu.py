"""Clipping by the global gradient norm and the non-finite skip inside the optimiser op (mccnn_grad_norm,
mccnn_adam_step_clipped, FusedAdam(maxGradNorm, skipNonFinite)) without a GPU: the ABI and the argument errors of the C
entries, the scalar rule compiled for the host, and FusedAdam on CPU parameters (the same definition in torch and NumPy)
against the unclipped class, the float64 norm and clip_grad_norm_ + torch.optim.Adam."""
import argparse
import copy
import ctypes as C
import inspect
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref  # noqa: E402
import grad_clip_ref as ref  # noqa: E402
from test_adam_cpu import LR, SHAPES, Rec, _feed, _records, _share, _twins  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BADARG, TOOLARGE, WORKSPACE = 0, -1, -3, -4
ENTRIES = ("mccnn_grad_norm_ws", "mccnn_grad_norm", "mccnn_adam_step_clipped")


class GradRec(C.Structure):   # mccnn_grad_record (include/mccnn.h)
    _fields_ = [("norm", C.c_float), ("coef", C.c_float), ("skipped", C.c_int), ("skips", C.c_int)]


# ------------------------------------------------------------------------------------------------- 1. ABI and bindings
def test_abi_version_and_error_codes():
    from mccnn_amd import _lib
    assert _lib.load().mccnn_abi_version() >= 29
    text = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    for name, code in (("MCCNN_E_BADARG", BADARG), ("MCCNN_E_TOOLARGE", TOOLARGE), ("MCCNN_E_WORKSPACE", WORKSPACE)):
        assert re.search(r"#define %s \(%d\)" % (name, code), text), name


def test_header_binding_and_library_agree():
    from mccnn_amd import _lib, build, optim
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mccnn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl and name in _lib.SIGNATURES and name in exported, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["mccnn_grad_norm_ws"][0] is C.c_size_t
    rec = re.search(r"typedef struct \{([^}]*)\} mccnn_grad_record;", code).group(1)
    assert re.findall(r"(\w+);", rec) == [n for n, _ in GradRec._fields_] == list(ref.RECORD.names) == list(optim.GradRecord._fields)
    assert C.sizeof(GradRec) == 16 == ref.RECORD.itemsize
    for name, _ in GradRec._fields_:
        assert getattr(GradRec, name).offset == ref.RECORD.fields[name][1], name
    assert "grad_clip.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "grad_clip.h"))
    src = open(os.path.join(build.CSRC, "adam.hip")).read()
    assert "kAdamMax = 76;" in src and "static_assert(sizeof(AdamArgs) < 4096" in src


# ------------------------------------------------------------------------------------------------- 2. bad arguments
RECORD_AT, WS_AT = 0x7f0000400000, 0x7f0000500000   # made-up addresses: never dereferenced, every call returns before a launch


def test_grad_norm_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()

    def call(specs, count=None, arr=False, gs=1.0, max_norm=1.0, skip=1, record=RECORD_AT, ws=WS_AT, ws_bytes=1 << 20):
        a = _records(specs)
        return lib.mccnn_grad_norm(None if arr is None else C.addressof(a), len(specs) if count is None else count, gs, max_norm, skip,
                                   record, ws, ws_bytes, None)
    inf, nan = float("inf"), float("nan")
    assert call([{}], count=-1) == BADARG
    assert call([{}], arr=None) == BADARG
    assert call([{}, {"n": -1}]) == BADARG
    assert call([{}, {"g": None}]) == BADARG
    for low in (1, 2, 3):
        assert call([{"g": 0x7f0000100000 + low}]) == BADARG, low
    for s in (inf, -inf, nan):
        assert call([{}], gs=s) == BADARG, s
    for m in (-1.0, -1e-30, inf, -inf, nan):
        assert call([{}], max_norm=m) == BADARG, m
    assert call([{}], record=None) == BADARG
    for low in (4, 8, 12):
        assert call([{}], record=RECORD_AT + low) == BADARG, low
    # p, m, v and the scalars are not looked at: a table that mccnn_adam_step refuses passes every check up to the workspace
    odd = {"p": None, "m": 0x3, "v": None, "step_size": nan, "bc2_sqrt": 0.0, "weight_decay": -inf}
    assert call([odd], ws_bytes=0) == WORKSPACE
    # the workspace: 8 bytes per chunk of 4096 elements of every live tensor
    three = [{"n": 4096}, {"n": 0, "g": None}, {"n": 4097}]
    a = _records(three)
    assert lib.mccnn_grad_norm_ws(C.addressof(a), 3) == 8 * 3
    assert call(three, ws_bytes=8 * 3 - 1) == WORKSPACE and call(three, ws=None) == WORKSPACE and call(three, ws_bytes=0) == WORKSPACE
    assert lib.mccnn_grad_norm_ws(None, 0) == 0
    # 2^31 chunks: a tensor of 2^31 - 1 elements is 2^19 chunks, so it takes 4096 of them
    cap = 4096
    assert call([{"n": (1 << 31) - 1}] * cap, ws_bytes=1 << 40) == TOOLARGE
    assert call([{"n": (1 << 31) - 1}] * (cap - 1), ws_bytes=0) == WORKSPACE
    # a bad record behind more than one launch's worth of good ones still stops the whole call
    assert call([{}] * (lib.mccnn_adam_max_tensors() + 2) + [{"n": -3}]) == BADARG
    assert lib.mccnn_debug_launch_count() == before


def test_adam_step_clipped_rejects_bad_arguments_before_launching():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()

    def call(specs, count=None, record=RECORD_AT, **k):
        a = _records(specs)
        s = dict(beta1=0.9, beta2=0.999, eps=1e-8, gs=1.0)
        s.update(k)
        return lib.mccnn_adam_step_clipped(C.addressof(a), len(specs) if count is None else count, s["beta1"], s["beta2"], s["eps"],
                                           s["gs"], record, None)
    inf, nan = float("inf"), float("nan")
    assert call([{}], record=None) == BADARG
    for low in (4, 8, 12):
        assert call([{}], record=RECORD_AT + low) == BADARG, low
    # mccnn_adam_step's own checks
    assert call([{}], count=-1) == BADARG and call([{}, {"n": -1}]) == BADARG
    for name in ("p", "g", "m", "v"):
        assert call([{}, {name: None}]) == BADARG and call([{name: 0x7f0000000000 + 2}]) == BADARG, name
    for b in (-0.1, 1.0, inf, nan):
        assert call([{}], beta1=b) == BADARG and call([{}], beta2=b) == BADARG, b
    assert call([{}], eps=-1e-8) == BADARG and call([{}], gs=nan) == BADARG
    assert call([{"step_size": inf}]) == BADARG and call([{"bc2_sqrt": 0.0}]) == BADARG and call([{"weight_decay": nan}]) == BADARG
    assert lib.mccnn_debug_launch_count() == before


def test_nothing_to_do_is_ok_and_launches_nothing():
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    assert lib.mccnn_grad_norm(None, 0, 1.0, 1.0, 1, RECORD_AT, None, 0, None) == OK
    assert lib.mccnn_adam_step_clipped(None, 0, 0.9, 0.999, 1e-8, 1.0, RECORD_AT, None) == OK
    arr = _records([{"n": 0, "p": None, "g": 0x3, "m": 0x5, "v": None, "bc2_sqrt": 0.0, "step_size": float("nan")}] * 5)
    assert lib.mccnn_grad_norm_ws(C.addressof(arr), 5) == 0
    assert lib.mccnn_grad_norm(C.addressof(arr), 5, 1.0, 0.0, 0, RECORD_AT, None, 0, None) == OK   # (n == 0: nothing of it is looked at)
    assert lib.mccnn_adam_step_clipped(C.addressof(arr), 5, 0.9, 0.999, 1e-8, 1.0, RECORD_AT, None) == OK
    assert lib.mccnn_debug_launch_count() == before


# ------------------------------------------------------------------------------------------------- 3. the rule on the host
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_coefficient_header_on_the_host(tmp_path, flags):
    """mccnn_amd/csrc/grad_clip.h compiled for the host as a stand-alone program (tools/grad_clip_check.cpp): max_norm = 0,
    norm = 0, norm < max_norm (exactly 1), norm > max_norm, norm inf and NaN."""
    exe = str(tmp_path / "grad_clip_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1"] + flags + ["-I", os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "grad_clip_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    m = re.match(r"ok (\d+)\n", out.stdout)
    assert out.returncode == 0 and m and int(m.group(1)) >= 30
    text = open(os.path.join(ROOT, "tools", "grad_clip_check.cpp")).read()
    for case in ("max_norm 0", "norm 0", "norm < max_norm", "norm > max_norm", "norm inf", "norm NaN"):
        assert '"%s"' % case in text, case


def test_the_python_rule_is_the_header_rule():
    """optim.clip_coef (the CPU route) against the reference's float32 formula, bit for bit, on the program's cases."""
    from mccnn_amd.optim import clip_coef
    big = np.finfo(np.float32).max
    for norm in (0.0, 1e-30, 0.999, 1.0, 3.0, 4.0, 123.456, 1e30, big, np.inf, np.nan):
        for max_norm in (0.0, 1e-7, 1e-3, 0.25, 1.0, 4.0, 1e30, big):
            a, b = np.float32(clip_coef(norm, max_norm)), ref.coef32(norm, max_norm)
            assert a.tobytes() == b.tobytes(), (norm, max_norm, a, b)
    assert ref.coef32(4.0, 1.0) < 0.25 and ref.coef32(1.0, 2.0) == 1 and ref.coef32(np.inf, 1.0) == 1 and ref.coef32(9.0, 0.0) == 1


# ------------------------------------------------------------------------------------------------- 4. FusedAdam on the CPU
def _grads(params):
    return [p.grad.detach().numpy() for p in params]


def _state_bytes(opt, params):
    return [(p.detach().numpy().tobytes(), opt.state[p]["exp_avg"].numpy().tobytes(), opt.state[p]["exp_avg_sq"].numpy().tobytes())
            for p in params]


@pytest.mark.parametrize("gs", [1.0, 0.25])
def test_a_clipped_step_equals_the_step_with_the_scaled_grad_scale(gs):
    from mccnn_amd.optim import FusedAdam, GradRecord
    a, b = _twins(11)
    _feed(a, b, 1100)
    want = ref.norm64(_grads(a), gs)
    oa = FusedAdam(a, lr=LR, weightDecay=1e-2, gradScale=gs, maxGradNorm=want / 4)
    assert oa.grad_record is None
    oa.step()
    r = oa.grad_record
    assert isinstance(r, GradRecord) and all(x.dim() == 0 and x.device.type == "cpu" for x in r)
    assert r.norm.dtype == r.coef.dtype == torch.float32 and r.skipped.dtype == r.skips.dtype == torch.int32
    print("norm uses %.3f of 16 e" % ref.share(float(r.norm), want))
    assert ref.share(float(r.norm), want) <= 1.0
    coef = np.float32(float(r.coef))
    assert coef.tobytes() == ref.coef32(float(r.norm), want / 4).tobytes() and abs(float(coef) - 0.25) < 1e-5
    assert int(r.skipped) == 0 and int(r.skips) == 0
    ob = FusedAdam(b, lr=LR, weightDecay=1e-2, gradScale=float(np.float32(np.float32(gs) * coef)))
    ob.step()
    assert _state_bytes(oa, a) == _state_bytes(ob, b) and ob.grad_record is None
    # the views follow the next step
    _feed(a, b, 1101)
    oa.maxGradNorm = 1e30
    oa.step()
    assert oa.grad_record is r and float(r.coef) == 1.0 and ref.share(float(r.norm), ref.norm64(_grads(a), gs)) <= 1.0


def test_an_inactive_clip_changes_no_bit():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(12)
    oa, ob = FusedAdam(a, lr=LR, gradScale=0.25, maxGradNorm=1e30), FusedAdam(b, lr=LR, gradScale=0.25)
    for s in range(3):
        _feed(a, b, 1200 + s)
        oa.step()
        ob.step()
        assert float(oa.grad_record.coef) == 1.0 and oa.grad_record.coef.numpy().tobytes() == np.float32(1.0).tobytes()
        assert _state_bytes(oa, a) == _state_bytes(ob, b)


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["plain", "decay"])
def test_five_clipped_steps_against_clip_grad_norm_and_torch_adam(wd):
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(13)
    clip = 3.0   # (the norm of these gradients is about sqrt(347): every step clips)
    oa, ob = FusedAdam(a, lr=LR, weightDecay=wd, maxGradNorm=clip), torch.optim.Adam(b, lr=LR, weight_decay=wd)
    for s in range(5):
        _feed(a, b, 1300 + s)
        oa.step()
        total = torch.nn.utils.clip_grad_norm_(b, clip)
        ob.step()
        assert float(total) > clip and float(oa.grad_record.coef) < 1.0
        assert ref.share(float(oa.grad_record.norm), float(total.double())) <= 2.0   # (torch's own float32 norm: twice the bar)
        worst = _share(a, b)
        assert worst <= 1.0, (s, worst)
    print("against clip_grad_norm_ + torch.optim.Adam after 5 steps: at most %.3f of 64 e (|p| + lr)" % worst)


def test_one_norm_over_all_groups_and_a_missing_gradient():
    """Two groups with different betas and a parameter without a gradient: one norm over the live tensors of both groups."""
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(14)
    groups = lambda q: [{"params": q[:3]}, {"params": q[3:], "betas": (0.8, 0.99)}]  # noqa: E731
    _feed(a, b, 1400, skip=(1,))
    want = ref.norm64([p.grad.numpy() for p in a if p.grad is not None])
    oa = FusedAdam(groups(a), lr=LR, maxGradNorm=want / 4)
    oa.step()
    assert ref.share(float(oa.grad_record.norm), want) <= 1.0
    ob = FusedAdam(groups(b), lr=LR, gradScale=float(oa.grad_record.coef))
    ob.step()
    live = [i for i in range(len(a)) if i != 1]
    assert _state_bytes(oa, [a[i] for i in live]) == _state_bytes(ob, [b[i] for i in live]) and a[1] not in oa.state


# ------------------------------------------------------------------------------------------------- 5. a NaN gradient
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e20], ids=["nan", "inf", "-inf", "1e20"])
def test_a_non_finite_step_is_skipped_and_counted(bad):
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(15)
    oa, ob = FusedAdam(a, lr=LR, weightDecay=1e-2, maxGradNorm=1.0, skipNonFinite=True), FusedAdam(b, lr=LR, weightDecay=1e-2, maxGradNorm=1.0)
    _feed(a, b, 1500)
    oa.step()
    ob.step()
    keep = _state_bytes(oa, a)
    assert keep == _state_bytes(ob, b) and int(oa.grad_record.skipped) == 0
    for k in (1, 2):
        _feed(a, b, 1500 + k)
        a[2].grad.view(-1)[-1] = bad
        oa.step()
        r = oa.grad_record
        assert _state_bytes(oa, a) == keep
        assert int(r.skipped) == 1 and int(r.skips) == k and float(r.coef) == 1.0 and not np.isfinite(float(r.norm))
        assert float(oa.state[a[0]]["step"]) == 1 + k   # (the host counts a skipped step: nothing is read back)
    # a finite step afterwards applies, at the step count the host has reached, and leaves skips alone
    _feed(a, b, 1510)
    oa.step()
    assert int(oa.grad_record.skipped) == 0 and int(oa.grad_record.skips) == 2 and np.isfinite(float(oa.grad_record.norm))
    for st in ob.state.values():
        st["step"] += 2.0
    ob._plan = None   # (the plan caches the counts it aliases)
    ob.step()
    assert _state_bytes(oa, a) == _state_bytes(ob, b) and _state_bytes(oa, a) != keep


def test_a_nan_with_the_switch_off_goes_through_like_the_unclipped_step():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(16)
    oa, ob = FusedAdam(a, lr=LR, maxGradNorm=1.0), FusedAdam(b, lr=LR)
    _feed(a, b, 1600)
    a[0].grad[1] = b[0].grad[1] = float("nan")
    oa.step()
    ob.step()
    r = oa.grad_record
    assert float(r.coef) == 1.0 and int(r.skipped) == 0 and int(r.skips) == 0 and np.isnan(float(r.norm))
    assert _state_bytes(oa, a) == _state_bytes(ob, b) and bool(torch.isnan(a[0]).any())


# ------------------------------------------------------------------------------------------------- 6. state and flags
def test_constructor_and_attribute_errors():
    from mccnn_amd.MCConvModule import InvalidArgumentError
    from mccnn_amd.optim import FusedAdam
    q = lambda: torch.nn.Parameter(torch.zeros(4))  # noqa: E731
    for v in (0, 0.0, -1.0, float("inf"), float("nan"), "1", torch.tensor(1.0), True, 1e39, 1e-50):
        with pytest.raises(InvalidArgumentError, match="FusedAdam: maxGradNorm must be None or a finite Python number > 0"):
            FusedAdam([q()], maxGradNorm=v)
    for v in (None, 1, 0, "yes", torch.tensor(True)):
        with pytest.raises(InvalidArgumentError, match="FusedAdam: skipNonFinite must be a bool"):
            FusedAdam([q()], skipNonFinite=v)
    opt = FusedAdam([q()], maxGradNorm=2, skipNonFinite=True)
    assert opt.maxGradNorm == 2 and opt.skipNonFinite is True
    # plain attributes: a bad value assigned later raises at the step, before anything is counted
    p = q()
    p.grad = torch.ones(4)
    opt = FusedAdam([p])
    opt.maxGradNorm = -3.0
    with pytest.raises(InvalidArgumentError, match="maxGradNorm"):
        opt.step()
    assert not opt.state and not p.any()
    opt.maxGradNorm = None
    opt.step()
    assert opt.grad_record is None and float(opt.state[p]["step"]) == 1
    opt.skipNonFinite = True
    opt.step()
    assert float(opt.grad_record.norm) == 2.0 and int(opt.grad_record.skips) == 0


def test_pickle_and_deepcopy_keep_both_and_state_dict_carries_neither():
    from mccnn_amd.optim import FusedAdam
    a, b = _twins(17)
    oa = FusedAdam(a, lr=LR, gradScale=0.5, maxGradNorm=2.5, skipNonFinite=True)
    keys = set(FusedAdam(b, lr=LR).state_dict()["param_groups"][0])
    _feed(a, b, 1700)
    oa.step()
    sd = oa.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["param_groups"][0]) == keys
    assert not any("Norm" in k or "NonFinite" in k or "clip" in k for g in sd["param_groups"] for k in g)
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    ot = torch.optim.Adam(b, lr=5.0)
    ot.load_state_dict(copy.deepcopy(sd))
    assert ot.param_groups[0]["lr"] == LR and float(ot.state[b[0]]["step"]) == 1
    for o in (copy.deepcopy(oa), pickle.loads(pickle.dumps(oa))):
        assert o.maxGradNorm == 2.5 and o.skipNonFinite is True and o.gradScale == 0.5 and o.grad_record is None
        ps = o.param_groups[0]["params"]
        for x, y in zip(a, ps):
            y.grad = x.grad.clone()
        o.step()
        assert float(o.grad_record.norm) == float(oa.grad_record.norm) and float(o.state[ps[0]]["step"]) == 2
    # load_state_dict keeps the attributes and the record
    oa.load_state_dict(sd)
    assert oa.maxGradNorm == 2.5 and oa.skipNonFinite is True and oa.grad_record is not None


def test_the_example_flags_reach_the_optimiser():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import mcclass_s
    import mcseg
    from mccnn_amd.optim import FusedAdam
    for mod in (mcclass_s, mcseg):
        src = inspect.getsource(mod.main)
        assert "--clip-norm" in src and "--skip-nonfinite" in src and "need --fused-adam" in src, mod.__name__

    class Collection:
        def __init__(self, items):
            self.items = items

        def get_collection(self, name):
            return list(self.items) if name == "weight_decay_loss" else []

    class Net:
        def __init__(self):
            self.ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
            self.store, self.convBuilder = Collection(self.ps[:1]), Collection([])

        def parameters(self):
            return iter(self.ps)

    opt = mcclass_s.make_optimizer(Net(), argparse.Namespace(fused_adam=True, weight_decay=1e-4, clip_norm=0.5, skip_nonfinite=True))
    assert isinstance(opt, FusedAdam) and opt.maxGradNorm == 0.5 and opt.skipNonFinite is True
    opt = mcclass_s.make_optimizer(Net(), argparse.Namespace(fused_adam=True, weight_decay=0.0))   # (the namespace of the older test)
    assert isinstance(opt, FusedAdam) and opt.maxGradNorm is None and opt.skipNonFinite is False
    assert type(mcclass_s.make_optimizer(Net(), argparse.Namespace(fused_adam=False, weight_decay=0.0))) is torch.optim.Adam
    with pytest.raises(ValueError, match="need --fused-adam"):
        mcclass_s.make_optimizer(Net(), argparse.Namespace(fused_adam=False, weight_decay=0.0, clip_norm=1.0))
    assert "maxGradNorm" in FusedAdam.__doc__ and "SKIPPED STEP IS STILL COUNTED" in FusedAdam.__doc__
    assert adam_ref.E == ref.E and SHAPES and Rec
