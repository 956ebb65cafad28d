"""The optimiser step as one op on the GPU (mccnn_adam_step, csrc/adam.hip; mccnn_amd.optim.FusedAdam): every element of p', m',
v' against the float64 reference of tests/adam_ref.py at its own bars, across chunk and tail boundaries, pointers off the
16-byte grid with guard words, more tensors than one launch takes, torch.optim.Adam on the GPU, and the gradients as autograd
leaves them after a backward pass of MCClassS."""
import functools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import adam_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LR = 1e-3
NPARAMS = 44   # the parameter tensors of MCClassS: 18 of three convolutions, 16 of eight batch-norm blocks, 10 of five linear layers
GUARD = 0x7FC0BEEF   # a NaN with a payload: any arithmetic on it, or any store over it, changes the bits


def _lib():
    from mccnn_amd import _lib as L
    return L


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _records(tensors):
    """tensors: dicts with the device addresses p, g, m, v and n, step_size, bc2_sqrt, weight_decay -> the HOST record array."""
    from mccnn_amd.optim import RECORD
    rec = np.zeros(len(tensors), dtype=RECORD)
    for r, t in zip(rec, tensors):
        for k in RECORD.names:
            r[k] = t[k]
    return rec


def _step(rec, d):
    """One mccnn_adam_step over the records with the call scalars of case d -> the number of launches it issued."""
    L = _lib()
    lib = L.load()
    before = lib.mccnn_debug_launch_count()
    L.check(lib.mccnn_adam_step(rec.ctypes.data, len(rec), d["beta1"], d["beta2"], d["eps"], d["grad_scale"], L.stream_handle()),
            "mccnn_adam_step")
    return lib.mccnn_debug_launch_count() - before


@functools.lru_cache(maxsize=None)
def _cases(sizes, form, grad_scale, t, seed=0):
    """One reference case per size, weight decay 1e-2 on every second tensor (computed once per parameter set, never written)."""
    return tuple(ref.case(n, seed + 31 * i, form, 1e-2 if i % 2 else 0.0, grad_scale, t, lr=LR) for i, n in enumerate(sizes))


def _check(got, cases, what):
    """got: per tensor (p', m', v') as float32 arrays."""
    worst = (0.0, 0.0, 0.0)
    for i, ((p, m, v), d) in enumerate(zip(got, cases)):
        assert p.dtype == m.dtype == v.dtype == np.float32 and len(p) == len(d["p"])
        s = ref.worst(p, m, v, d["want"])
        worst = tuple(max(a, b) for a, b in zip(worst, s))
        assert max(s) <= 1.0, "%s: tensor %d of %d elements uses %.3g of tol_p, %.3g of tol_m, %.3g of tol_v" % ((what, i, len(p)) + s)
    print("%s: at most %.2f of tol_p, %.2f of tol_m, %.2f of tol_v" % ((what,) + worst))


def _boundary_sizes():
    from mccnn_amd.optim import CHUNK as c
    return (1, 2, 3, 4, 5, 63, 64, 65, 255, 257, c - 1, c, c + 1, 2 * c + 7)


def _run_separate(cases):
    """Every array of every tensor in an allocation of its own (all 16-byte aligned), one call -> (results, launches)."""
    import torch
    bufs = [{k: _dev(d[k]) for k in ("p", "g", "m", "v")} for d in cases]
    rec = _records([dict({k: b[k].data_ptr() for k in b}, n=len(d["p"]), step_size=d["step_size"], bc2_sqrt=d["bc2_sqrt"],
                         weight_decay=d["weight_decay"]) for b, d in zip(bufs, cases)])
    launches = _step(rec, cases[0])
    torch.cuda.synchronize()
    for b, d in zip(bufs, cases):
        assert np.array_equal(b["g"].cpu().numpy().view(np.int32), d["g"].view(np.int32))   # the gradient is only read
    return [tuple(b[k].cpu().numpy() for k in ("p", "m", "v")) for b in bufs], launches


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("form", ref.FORMS)
def test_chunk_and_tail_boundaries_in_one_call(mc, form, grad_scale, t):
    cases = _cases(_boundary_sizes(), form, grad_scale, t)
    got, launches = _run_separate(cases)
    assert launches == 1
    _check(got, cases, "boundaries %s scale %g t %d" % (form, grad_scale, t))


# 2 ------------------------------------------------------------------------------------------------------------------------
WIDTHS = (3, 8, 17, 64, 5, 1)


@pytest.mark.parametrize("offsets", [(0, 1, 2, 3), (3, 3, 3, 3), (1, 1, 1, 1)], ids=["0123", "3333", "1111"])
def test_pointers_off_the_16_byte_grid_with_guard_words(mc, offsets):
    """The four arrays of six tensors side by side in one buffer each, as spatial_conv's backward hands out a layer's gradients,
    with one guard word in front of, between and behind the tensors; the buffers start `offsets` floats behind a 256-byte
    boundary. (3, 3, 3, 3): the guard of every buffer sits on word 3, so tensors 0 and 1 start on a 16-byte boundary in all
    four arrays and take the wide path with a neighbour right behind their last element."""
    import torch
    cases = _cases(WIDTHS, "torch", 0.25, 2, seed=500)
    total = 1 + sum(w + 1 for w in WIDTHS)
    host, starts = {}, []
    pos = 1
    for w in WIDTHS:
        starts.append(pos)
        pos += w + 1
    for k in ("p", "g", "m", "v"):
        a = np.full(total, GUARD, dtype=np.int32)
        for s, d in zip(starts, cases):
            a[s:s + len(d[k])] = d[k].view(np.int32)
        host[k] = a
    whole = {k: torch.full((total + 8,), 0x55555555, dtype=torch.int32, device="cuda") for k in host}
    view = {}
    for k, off in zip(("p", "g", "m", "v"), offsets):
        assert whole[k].data_ptr() % 256 == 0
        view[k] = whole[k][off:off + total]
        view[k].copy_(torch.from_numpy(host[k]))
    rec = _records([dict({k: view[k].data_ptr() + 4 * s for k in view}, n=len(d["p"]), step_size=d["step_size"],
                         bc2_sqrt=d["bc2_sqrt"], weight_decay=d["weight_decay"]) for s, d in zip(starts, cases)])
    if offsets == (3, 3, 3, 3):
        assert all(int(rec[k][i]) % 16 == 0 for k in ("p", "g", "m", "v") for i in (0, 1))
    assert _step(rec, cases[0]) == 1
    torch.cuda.synchronize()
    out = {k: view[k].cpu().numpy() for k in view}
    assert np.array_equal(out["g"], host["g"])                         # the gradient buffer as a whole
    guards = np.ones(total, dtype=bool)
    for s, w in zip(starts, WIDTHS):
        guards[s:s + w] = False
    for k in ("p", "m", "v"):
        assert np.all(out[k][guards] == GUARD), k
        rest = whole[k].cpu().numpy()
        off = offsets["pgmv".index(k)]
        assert np.all(rest[:off] == 0x55555555) and np.all(rest[off + total:] == 0x55555555), k
    got = [tuple(out[k][s:s + w].view(np.float32) for k in ("p", "m", "v")) for s, w in zip(starts, WIDTHS)]
    _check(got, cases, "offsets %s" % (offsets,))


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["max+1", "2max+3"])
def test_more_tensors_than_one_launch_takes(mc, which):
    import torch
    cap = _lib().load().mccnn_adam_max_tensors()
    live = cap + 1 if which == "max+1" else 2 * cap + 3
    sizes = tuple(1 + (7 * i) % 9 for i in range(live))
    cases = _cases(sizes, "tf", 1.0, 2, seed=900)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    bufs = {k: _dev(np.concatenate([d[k] for d in cases])) for k in ("p", "g", "m", "v")}   # side by side: mostly off the grid
    specs = []
    for i, d in enumerate(cases):
        if i % 11 == 5 or i == live - 1:   # n == 0 records in between, and one right before the last: never dereferenced
            specs.append(dict(p=0x1, g=0, m=0xDEAD0003, v=0x7, n=0, step_size=float("nan"), bc2_sqrt=0.0, weight_decay=0.0))
        specs.append(dict({k: bufs[k].data_ptr() + 4 * int(starts[i]) for k in bufs}, n=sizes[i], step_size=d["step_size"],
                          bc2_sqrt=d["bc2_sqrt"], weight_decay=d["weight_decay"]))
    specs.append(dict(p=0, g=0, m=0, v=0, n=0, step_size=0.0, bc2_sqrt=0.0, weight_decay=0.0))
    rec = _records(specs)
    keep = rec.copy()
    assert int((rec["n"] > 0).sum()) == live and len(rec) > live + 2
    assert _step(rec, cases[0]) == math.ceil(live / cap)
    torch.cuda.synchronize()
    assert rec.tobytes() == keep.tobytes()   # the host array is read, not written
    out = {k: bufs[k].cpu().numpy() for k in bufs}
    assert np.array_equal(out["g"].view(np.int32), np.concatenate([d["g"] for d in cases]).view(np.int32))
    got = [tuple(out[k][starts[i]:starts[i + 1]] for k in ("p", "m", "v")) for i in range(live)]
    _check(got, cases, "%d live tensors, capacity %d" % (live, cap))


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mcclass_s_shapes(mc):
    """The parameter shapes of MCClassS (k = 16, 40 classes) in parameters() order, and which of them the reference decays."""
    import torch
    from mcclass_s import MCClassS
    from mccnn_amd.workloads import modelnet_like
    dev = torch.device("cuda", 0)
    pts, bids = modelnet_like(64, 2, 11)
    net = MCClassS(1, 2, 16, 40, dev)
    with torch.no_grad():
        net(torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev), torch.ones((len(pts), 1), device=dev), True)
    params = list(net.parameters())
    decay = {id(p) for p in net.store.get_collection("weight_decay_loss") + net.convBuilder.get_collection("weight_decay_loss")}
    assert len(params) == NPARAMS and 0 < len(decay) < NPARAMS
    return [tuple(p.shape) for p in params], [id(p) in decay for p in params]


@pytest.mark.parametrize("mode", ["decayParams", "gradScale"])
def test_against_torch_adam_on_the_gpu(mc, mcclass_s_shapes, mode):
    """The same seeded values and gradients to FusedAdam and torch.optim.Adam, 5 steps, every parameter within
    64 e (|p| + lr): with decayParams against a two-group torch Adam, with gradScale against gradients scaled by torch."""
    import torch
    from mccnn_amd.optim import FusedAdam
    shapes, decayed = mcclass_s_shapes
    gen = torch.Generator(device="cuda").manual_seed(17)
    init = [torch.randn(s, device="cuda", generator=gen) for s in shapes]
    a = [torch.nn.Parameter(x.clone()) for x in init]
    b = [torch.nn.Parameter(x.clone()) for x in init]
    if mode == "decayParams":
        oa = FusedAdam(a, lr=LR, weightDecay=1e-2, decayParams=[x for x, d in zip(a, decayed) if d])
        ob = torch.optim.Adam([{"params": [y for y, d in zip(b, decayed) if d], "weight_decay": 1e-2},
                               {"params": [y for y, d in zip(b, decayed) if not d], "weight_decay": 0.0}], lr=LR)
        scale = 1.0
    else:
        oa, ob, scale = FusedAdam(a, lr=LR, gradScale=0.25), torch.optim.Adam(b, lr=LR), 0.25
    lib = _lib().load()
    for step in range(5):
        for x, y in zip(a, b):
            g = torch.randn(x.shape, device="cuda", generator=gen)
            x.grad, y.grad = g.clone(), g * scale
        before = lib.mccnn_debug_launch_count()
        oa.step()
        assert lib.mccnn_debug_launch_count() - before == math.ceil(NPARAMS / lib.mccnn_adam_max_tensors())
        ob.step()
    torch.cuda.synchronize()
    worst = 0.0
    for i, (x, y) in enumerate(zip(a, b)):
        share = float(((x.detach() - y.detach()).abs() / (64 * ref.E * (y.detach().abs() + LR))).max())
        worst = max(worst, share)
        assert share <= 1.0, (i, shapes[i], share)
        assert float(oa.state[x]["step"]) == 5 and not torch.equal(x.detach(), init[i])
    print("%s against torch.optim.Adam on the GPU after 5 steps: at most %.3f of 64 e (|p| + lr)" % (mode, worst))


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_the_gradients_as_autograd_leaves_them(mc):
    """One forward and backward of MCClassS on the HIP ops (2 clouds x 64 points, k = 8), the gradients taken as they are: views
    of a layer's gradient buffer, offsets and all. One FusedAdam.step() against the reference over clones, in one launch; then
    zero_grad(set_to_none=True), fresh gradients in new memory (the old ones are kept alive) and a second step: the
    persistent record array follows the new pointers."""
    import torch
    from mcclass_s import MCClassS
    from mccnn_amd.optim import FusedAdam
    from mccnn_amd.workloads import modelnet_like
    dev = torch.device("cuda", 0)
    B, n, k, ncat = 2, 64, 8, 40
    torch.manual_seed(23)
    net = MCClassS(1, B, k, ncat, dev)
    lib = _lib().load()

    def backward(seed):
        pts, bids = modelnet_like(n, B, seed)
        P, Bi = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev)
        y = torch.from_numpy(np.random.default_rng(seed).integers(0, ncat, B)).to(dev)
        loss = torch.nn.functional.cross_entropy(net(P, Bi, torch.ones((len(pts), 1), device=dev), True), y)
        loss.backward()

    with torch.no_grad():
        pts, bids = modelnet_like(n, B, 1)
        net(torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev), torch.ones((len(pts), 1), device=dev), True)
    params = list(net.parameters())
    assert len(params) == NPARAMS
    opt = FusedAdam(params, lr=LR)
    b1, b2, eps = ref.f32(0.9), ref.f32(0.999), ref.f32(1e-8)
    m = [np.zeros(p.numel(), np.float32) for p in params]
    v = [np.zeros(p.numel(), np.float32) for p in params]
    old, off_grid = [], 0
    for t in (1, 2):
        opt.zero_grad(set_to_none=True)
        backward(40 + t)
        grads = [p.grad for p in params]
        assert all(g is not None for g in grads)
        if old:
            assert not {g.data_ptr() for g in grads} & {g.data_ptr() for g in old}
        off_grid += sum(g.data_ptr() % 16 != 0 for g in grads)
        p0 = [p.detach().cpu().numpy().reshape(-1).copy() for p in params]
        g0 = [g.detach().contiguous().cpu().numpy().reshape(-1).copy() for g in grads]
        before = lib.mccnn_debug_launch_count()
        opt.step()
        assert lib.mccnn_debug_launch_count() - before == math.ceil(NPARAMS / lib.mccnn_adam_max_tensors())
        torch.cuda.synchronize()
        ss, bs = ref.scalars("torch", LR, b1, b2, t)
        cases = [dict(p=p0[i], want=ref.step(p0[i], g0[i], m[i], v[i], ss, bs, 0.0, b1, b2, eps, 1.0)) for i in range(NPARAMS)]
        got = [(p.detach().cpu().numpy().reshape(-1), opt.state[p]["exp_avg"].cpu().numpy().reshape(-1),
                opt.state[p]["exp_avg_sq"].cpu().numpy().reshape(-1)) for p in params]
        _check(got, cases, "MCClassS step %d" % t)
        for g, g_before in zip(grads, g0):
            assert np.array_equal(g.detach().contiguous().cpu().numpy().reshape(-1).view(np.int32), g_before.view(np.int32))
        assert any(not np.array_equal(a[0], c["p"]) for a, c in zip(got, cases))
        m, v = [a[1].copy() for a in got], [a[2].copy() for a in got]
        old = old + grads
    print("gradients off the 16-byte grid over both steps: %d of %d" % (off_grid, 2 * NPARAMS))
    # (at k = 8 every slice of a convolution's gradient buffer is a multiple of four floats long, so all of them can lie on the
    # grid; the pointers off it are test 2's)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_the_same_inputs_give_the_same_bytes(mc):
    cases = _cases(_boundary_sizes(), "torch", 0.25, 2)
    first, _ = _run_separate(cases)
    second, _ = _run_separate(cases)
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
