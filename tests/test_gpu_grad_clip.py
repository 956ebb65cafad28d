"""Clipping by the global gradient norm and the non-finite skip on the GPU (mccnn_grad_norm, mccnn_adam_step_clipped,
csrc/adam.hip; FusedAdam(maxGradNorm, skipNonFinite)): the norm against float64 NumPy at 16 e across chunk and tail
boundaries, gradients off the 16-byte grid, more tensors than one launch takes; the clipped step byte for byte against
mccnn_adam_step with the scaled grad_scale; non-finite values as data; FusedAdam against clip_grad_norm_ + torch.optim.Adam."""
import functools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import adam_ref  # noqa: E402
import grad_clip_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LR = 1e-3
NPARAMS = 44   # the parameter tensors of MCClassS
GUARD = 0x7FC0BEEF   # a NaN with a payload: any arithmetic on it, or any store over it, changes the bits
CAP = 76       # mccnn_adam_max_tensors()
KEYS = ("p", "g", "m", "v")


def _lib():
    from mccnn_amd import _lib as L
    return L


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f32mul(a, b):
    return float(np.float32(np.float32(a) * np.float32(b)))


class Norm:
    """A record between guard words, and one mccnn_grad_norm over a record array with exactly the bytes of partials the library
    asks for, between guard words too."""

    def __init__(self):
        import torch
        self.buf = torch.full((12,), GUARD, dtype=torch.int32, device="cuda")
        self.buf[4:8] = 0            # the owner zeroes the record once
        self.rec = self.buf[4:8]
        assert self.rec.data_ptr() % 16 == 0

    def __call__(self, rec, grad_scale, max_norm, skip):
        """-> the launches of the call."""
        import torch
        L = _lib()
        lib = L.load()
        need = lib.mccnn_grad_norm_ws(rec.ctypes.data, len(rec))
        assert need % 8 == 0
        ws = torch.full((need // 4 + 4,), GUARD, dtype=torch.int32, device="cuda")
        before = lib.mccnn_debug_launch_count()
        L.check(lib.mccnn_grad_norm(rec.ctypes.data, len(rec), grad_scale, max_norm, int(skip), self.rec.data_ptr(), ws.data_ptr() + 8,
                                    need, L.stream_handle()), "mccnn_grad_norm")
        launches = lib.mccnn_debug_launch_count() - before
        torch.cuda.synchronize()
        w = ws.cpu().numpy()
        assert np.all(w[:2] == GUARD) and np.all(w[-2:] == GUARD), "guard words around the partials"
        assert not np.any(np.all(w[2:-2].reshape(-1, 2) == GUARD, axis=1)), "every partial is written"
        b = self.buf.cpu().numpy()
        assert np.all(b[:4] == GUARD) and np.all(b[8:] == GUARD), "guard words around the record"
        return launches

    def read(self):
        return self.rec.cpu().numpy().view(ref.RECORD)[0]

    def ptr(self):
        return self.rec.data_ptr()


def _grad_records(ptrs, sizes):
    """Records that carry g and n only; p, m, v and the scalars hold what mccnn_adam_step would refuse."""
    from mccnn_amd.optim import RECORD
    rec = np.zeros(len(sizes), dtype=RECORD)
    rec["g"], rec["n"] = ptrs, sizes
    rec["p"], rec["m"], rec["v"] = 0, 0x3, 0x7
    rec["step_size"], rec["bc2_sqrt"], rec["weight_decay"] = np.nan, 0.0, -np.inf
    return rec


@functools.lru_cache(maxsize=None)
def _grad(n, seed):
    return adam_ref.inputs(n, seed, False)[1]


def _check_norm(r, grads, gs, what, max_norm=0.0):
    want = ref.norm64(grads, gs)
    used = ref.share(r["norm"], want)
    print("%s: norm %.9g, float64 %.17g, %.3f of 16 e" % (what, r["norm"], want, used))
    assert used <= 1.0, what
    assert np.float32(r["coef"]).tobytes() == ref.coef32(r["norm"], max_norm).tobytes(), what
    return want


# 1 ------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193)


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_chunk_and_tail_boundaries(mc, grad_scale):
    """Every size in a call of its own and all in one call, every gradient in an allocation of its own (16-byte loads)."""
    grads = [_grad(n, 40 + i) for i, n in enumerate(SIZES)]
    bufs = [_dev(g) for g in grads]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    for n, g, b in zip(SIZES, grads, bufs):
        nr = Norm()
        assert nr(_grad_records([b.data_ptr()], [n]), grad_scale, 0.0, False) == 2
        r = nr.read()
        _check_norm(r, [g], grad_scale, "n = %d" % n)
        assert r["skipped"] == 0 and r["skips"] == 0
    nr = Norm()
    want = ref.norm64(grads, grad_scale)
    assert nr(_grad_records([b.data_ptr() for b in bufs], SIZES), grad_scale, want / 4, True) == 2
    r = nr.read()
    _check_norm(r, grads, grad_scale, "all sizes in one call", want / 4)
    assert abs(float(r["coef"]) - 0.25) < 1e-5 and r["skipped"] == 0 and r["skips"] == 0
    for g, b in zip(grads, bufs):
        assert np.array_equal(b.cpu().numpy().view(np.int32), g.view(np.int32))   # the gradient is only read


def test_a_zero_gradient(mc):
    bufs = [_dev(np.zeros(n, np.float32)) for n in (5, 4097)]
    nr = Norm()
    assert nr(_grad_records([b.data_ptr() for b in bufs], [5, 4097]), 0.25, 1.0, True) == 2
    r = nr.read()
    assert r["norm"] == 0.0 and r["coef"] == 1.0 and r["skipped"] == 0 and r["skips"] == 0


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 2, 3], ids=["4 bytes", "8 bytes", "12 bytes"])
def test_gradients_off_the_16_byte_grid(mc, off):
    """Gradient pointers 4, 8 and 12 bytes behind a 16-byte boundary (one float per lane), side by side with guard words
    between them, over tails and more than one chunk."""
    import torch
    sizes = (17, 4096, 4099, 8193, 1, 255)
    grads = [_grad(n, 70 + i) for i, n in enumerate(sizes)]
    starts, pos = [], off
    for n in sizes:
        starts.append(pos)
        pos += (n + 1 + 3) // 4 * 4   # (the next tensor starts `off` words behind a boundary too, at least one guard word on)
    host = np.full(pos + 4, GUARD, dtype=np.int32)
    for s, g in zip(starts, grads):
        host[s:s + len(g)] = g.view(np.int32)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0
    ptrs = [buf.data_ptr() + 4 * s for s in starts]
    assert all(p % 16 == 4 * off for p in ptrs)
    nr = Norm()
    assert nr(_grad_records(ptrs, sizes), 0.25, 0.0, False) == 2
    _check_norm(nr.read(), grads, 0.25, "gradients %d bytes off the grid" % (4 * off))
    assert np.array_equal(buf.cpu().numpy(), host)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["2max+3", "300 of one element"])
def test_more_tensors_than_one_launch_takes(mc, which):
    assert _lib().load().mccnn_adam_max_tensors() == CAP
    if which == "2max+3":
        live = 2 * CAP + 3
        sizes = tuple(1 + (7 * i) % 9 if i % 50 else 4097 + i for i in range(live))
    else:
        live, sizes = 300, (1,) * 300   # more partials than the finish workgroup has lanes
    grads = [_grad(n, 900 + i) for i, n in enumerate(sizes)]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    buf = _dev(np.concatenate(grads))   # side by side: mostly off the grid
    ptrs, ns = [], []
    for i in range(live):
        if i % 11 == 5 or i == live - 1:   # n == 0 records in between, and one right before the last: never dereferenced
            ptrs.append(0x1)
            ns.append(0)
        ptrs.append(buf.data_ptr() + 4 * int(starts[i]))
        ns.append(sizes[i])
    ptrs.append(0)
    ns.append(0)
    rec = _grad_records(ptrs, ns)
    keep = rec.copy()
    assert int((rec["n"] > 0).sum()) == live and len(rec) > live + 2
    nr = Norm()
    assert nr(rec, 1.0, 0.0, False) == math.ceil(live / CAP) + 1
    assert rec.tobytes() == keep.tobytes()   # the host array is read, not written
    _check_norm(nr.read(), grads, 1.0, "%d live tensors" % live)


# 4 ------------------------------------------------------------------------------------------------------------------------
class Flat:
    """p, g, m, v of several tensors side by side in one buffer each, guard words in front of, between and behind them: one
    word each (most tensors then start off the 16-byte grid), or with on_grid as many as put every tensor on the grid (16-byte
    accesses, and a guard word right behind the last n % 4 elements)."""

    def __init__(self, tensors, on_grid=False):
        import torch
        self.sizes = [len(t["p"]) for t in tensors]
        self.starts, pos = [], 4 if on_grid else 1
        for n in self.sizes:
            self.starts.append(pos)
            pos += n + 1
            if on_grid:
                pos = (pos + 3) // 4 * 4
        self.host = {}
        for k in KEYS:
            a = np.full(pos, GUARD, dtype=np.int32)
            for s, t in zip(self.starts, tensors):
                a[s:s + len(t[k])] = t[k].view(np.int32)
            self.host[k] = a
        self.dev = {k: torch.from_numpy(self.host[k]).cuda() for k in KEYS}
        assert all(self.dev[k].data_ptr() % 256 == 0 for k in KEYS)
        self.guards = np.ones(pos, dtype=bool)
        for s, n in zip(self.starts, self.sizes):
            self.guards[s:s + n] = False

    def records(self, scalars):
        from mccnn_amd.optim import RECORD
        rec = np.zeros(len(self.sizes), dtype=RECORD)
        for k in KEYS:
            rec[k] = [self.dev[k].data_ptr() + 4 * s for s in self.starts]
        rec["n"] = self.sizes
        for k in ("step_size", "bc2_sqrt", "weight_decay"):
            rec[k] = [s[k] for s in scalars]
        return rec

    def reset(self, grads=None):
        import torch
        for k in KEYS:
            self.dev[k].copy_(torch.from_numpy(self.host[k] if k != "g" or grads is None else grads))

    def out(self):
        """-> the bytes of p, m, v (guard words included), after checking those guard words and the gradient buffer."""
        import torch
        torch.cuda.synchronize()
        got = {k: self.dev[k].cpu().numpy() for k in KEYS}
        for k in ("p", "m", "v"):
            assert np.all(got[k][self.guards] == GUARD), k
        return tuple(got[k].tobytes() for k in ("p", "m", "v")), got["g"]


def _plain(rec, d, gs):
    L = _lib()
    L.check(L.load().mccnn_adam_step(rec.ctypes.data, len(rec), d["beta1"], d["beta2"], d["eps"], gs, L.stream_handle()), "mccnn_adam_step")


def _clipped(rec, d, gs, record_ptr):
    L = _lib()
    lib = L.load()
    before = lib.mccnn_debug_launch_count()
    L.check(lib.mccnn_adam_step_clipped(rec.ctypes.data, len(rec), d["beta1"], d["beta2"], d["eps"], gs, record_ptr, L.stream_handle()),
            "mccnn_adam_step_clipped")
    return lib.mccnn_debug_launch_count() - before


@pytest.mark.parametrize("t", [1, 5])
@pytest.mark.parametrize("form", adam_ref.FORMS)
def test_a_clipped_step_equals_the_step_with_the_scaled_grad_scale(mc, form, t):
    """mccnn_grad_norm + mccnn_adam_step_clipped at max_norm = norm / 4 against mccnn_adam_step with float32(gs * coef), coef
    read from the record; at max_norm = 0 and 4 * norm, coef == 1.0 and the bytes are mccnn_adam_step's with gs."""
    sizes = (3, 4097, 300, 8)
    for wd in (0.0, 1e-2):
        for gs in (1.0, 0.25):
            cases = [adam_ref.case(n, 31 * i, form, wd, gs, t, lr=LR) for i, n in enumerate(sizes)]
            d = cases[0]
            fl = Flat(cases, on_grid=wd != 0)
            rec = fl.records(cases)
            want = ref.norm64([c["g"] for c in cases], gs)
            _plain(rec, d, d["grad_scale"])
            unclipped, _ = fl.out()
            assert unclipped[0] != fl.host["p"].tobytes()
            for max_norm, active in ((want / 4, True), (0.0, False), (4 * want, False)):
                fl.reset()
                nr = Norm()
                assert nr(rec, d["grad_scale"], max_norm, True) == 2
                assert _clipped(rec, d, d["grad_scale"], nr.ptr()) == 1
                got, g_after = fl.out()
                assert np.array_equal(g_after, fl.host["g"])
                r = nr.read()
                what = "%s t %d wd %g scale %g max_norm %g" % (form, t, wd, gs, max_norm)
                _check_norm(r, [c["g"] for c in cases], gs, what, max_norm)
                assert r["skipped"] == 0 and r["skips"] == 0
                if not active:
                    assert r["coef"] == 1.0 and got == unclipped, what
                    continue
                assert abs(float(r["coef"]) - 0.25) < 1e-5 and got != unclipped, what
                fl.reset()
                _plain(rec, d, _f32mul(d["grad_scale"], r["coef"]))
                assert got == fl.out()[0], what


# 5 ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _many():
    """80 tensors: a tail, two and three chunks, and a second launch's worth of small ones; moments of an earlier step."""
    sizes = (5, 4099, 9000, 7) + (3,) * (CAP - 4) + (6, 2, 9, 1)
    rng = np.random.default_rng(5)
    tensors, scalars = [], []
    for i, n in enumerate(sizes):
        p, g = adam_ref.inputs(n, 300 + i, False)
        tensors.append(dict(p=p, g=g, m=(0.1 * rng.standard_normal(n)).astype(np.float32), v=(rng.random(n) * 1e-2).astype(np.float32)))
        scalars.append(dict(step_size=1e-3, bc2_sqrt=0.5, weight_decay=1e-2 if i % 2 else 0.0))
    return sizes, tensors, scalars


PLACES = {"the first element": (0, 0), "the last tail element": (1, 4098), "the second chunk of the third tensor": (2, 4096 + 100),
          "a tensor of the second launch": (CAP + 2, 8)}
SCALARS = dict(beta1=adam_ref.f32(0.9), beta2=adam_ref.f32(0.999), eps=adam_ref.f32(1e-8))


@pytest.mark.parametrize("place", list(PLACES))
def test_non_finite_values_as_data(mc, place):
    sizes, tensors, scalars = _many()
    fl = Flat(tensors, on_grid=True)
    rec = fl.records(scalars)
    k, j = PLACES[place]
    assert sizes[k] > j and sum(1 for n in sizes[:k] if n > 0) == k
    gs = 0.25
    fl.reset()
    _plain(rec, SCALARS, gs)
    finite_step, _ = fl.out()
    before = tuple(fl.host[key].tobytes() for key in ("p", "m", "v"))
    for bad in (np.nan, np.inf, -np.inf, 1e20):
        what = "%s at %s" % (bad, place)
        g = fl.host["g"].copy()
        g.view(np.float32)[fl.starts[k] + j] = bad
        # the switch on: nothing of p, m, v changes, and the record counts
        fl.reset(g)
        nr = Norm()
        for n in (1, 2):
            assert nr(rec, gs, 1.0, True) == 3
            assert _clipped(rec, SCALARS, gs, nr.ptr()) == 2
            got, _ = fl.out()
            r = nr.read()
            assert got == before, what
            assert r["skipped"] == 1 and r["skips"] == n and r["coef"] == 1.0 and not np.isfinite(r["norm"]), what
        # a finite call afterwards applies, and leaves the count alone
        fl.reset()
        nr(rec, gs, 0.0, True)
        _clipped(rec, SCALARS, gs, nr.ptr())
        got, _ = fl.out()
        r = nr.read()
        assert r["skipped"] == 0 and r["skips"] == 2 and r["coef"] == 1.0 and np.isfinite(r["norm"]), what
        assert got == finite_step, what
        # the switch off: the non-finite value goes through as in mccnn_adam_step
        fl.reset(g)
        _plain(rec, SCALARS, gs)
        through, _ = fl.out()
        fl.reset(g)
        nr = Norm()
        nr(rec, gs, 1.0, False)
        _clipped(rec, SCALARS, gs, nr.ptr())
        got, _ = fl.out()
        r = nr.read()
        assert r["coef"] == 1.0 and r["skipped"] == 0 and r["skips"] == 0 and not np.isfinite(r["norm"]), what
        assert got == through and got != before, what


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mcclass_s_shapes(mc):
    """The parameter shapes of MCClassS (k = 16, 40 classes) in parameters() order."""
    import torch
    from mcclass_s import MCClassS
    from mccnn_amd.workloads import modelnet_like
    dev = torch.device("cuda", 0)
    pts, bids = modelnet_like(64, 2, 11)
    net = MCClassS(1, 2, 16, 40, dev)
    with torch.no_grad():
        net(torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev), torch.ones((len(pts), 1), device=dev), True)
    shapes = [tuple(p.shape) for p in net.parameters()]
    assert len(shapes) == NPARAMS
    return shapes


def test_fused_adam_against_clip_grad_norm_and_torch_adam_on_the_gpu(mc, mcclass_s_shapes):
    """The same seeded values and gradients to FusedAdam(maxGradNorm) and clip_grad_norm_ + torch.optim.Adam, 5 steps, every
    parameter within 64 e (|p| + lr); three launches per clipped step, one with both switches off."""
    import torch
    from mccnn_amd.optim import FusedAdam
    shapes = mcclass_s_shapes
    gen = torch.Generator(device="cuda").manual_seed(19)
    init = [torch.randn(s, device="cuda", generator=gen) for s in shapes]
    a = [torch.nn.Parameter(x.clone()) for x in init]
    b = [torch.nn.Parameter(x.clone()) for x in init]
    c = [torch.nn.Parameter(x.clone()) for x in init]
    clip = 10.0   # (standard normal gradients over some 1e5 elements: every step clips)
    oa, ob, oc = FusedAdam(a, lr=LR, maxGradNorm=clip, skipNonFinite=True), torch.optim.Adam(b, lr=LR), FusedAdam(c, lr=LR)
    lib = _lib().load()
    norms = []
    for step in range(5):
        for x, y, z in zip(a, b, c):
            g = torch.randn(x.shape, device="cuda", generator=gen)
            x.grad, y.grad, z.grad = g.clone(), g.clone(), g
        want = ref.norm64([x.grad.cpu().numpy() for x in a])
        before = lib.mccnn_debug_launch_count()
        oa.step()
        assert lib.mccnn_debug_launch_count() - before == 2 * math.ceil(NPARAMS / CAP) + 1 == 3
        before = lib.mccnn_debug_launch_count()
        oc.step()
        assert lib.mccnn_debug_launch_count() - before == 1
        torch.nn.utils.clip_grad_norm_(b, clip)
        ob.step()
        r = oa.grad_record
        assert all(v.device.type == "cuda" and v.dim() == 0 for v in r)
        norms.append(torch.stack([r.norm, r.coef]))   # (a loop's read-back of its own: the class reads nothing back)
        rec = norms[-1].cpu().numpy()
        assert ref.share(rec[0], want) <= 1.0 and rec[0] > clip and rec[1] < 1.0
    torch.cuda.synchronize()
    assert int(r.skipped) == 0 and int(r.skips) == 0 and oc.grad_record is None
    worst = 0.0
    for i, (x, y) in enumerate(zip(a, b)):
        share = float(((x.detach() - y.detach()).abs() / (64 * adam_ref.E * (y.detach().abs() + LR))).max())
        worst = max(worst, share)
        assert share <= 1.0, (i, shapes[i], share)
        assert float(oa.state[x]["step"]) == 5 and not torch.equal(x.detach(), init[i])
    print("maxGradNorm against clip_grad_norm_ + torch.optim.Adam on the GPU after 5 steps: at most %.3f of 64 e (|p| + lr)" % worst)


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_two_groups_with_different_betas_share_one_norm(mc):
    import torch
    from mccnn_amd.optim import FusedAdam
    shapes = [(3,), (70, 64), (5, 7), (4099,), (33, 4), (129,)]
    gen = torch.Generator(device="cuda").manual_seed(23)
    init = [torch.randn(s, device="cuda", generator=gen) for s in shapes]
    grads = [torch.randn(s, device="cuda", generator=gen) for s in shapes]
    a = [torch.nn.Parameter(x.clone()) for x in init]
    b = [torch.nn.Parameter(x.clone()) for x in init]
    groups = lambda q: [{"params": q[:3]}, {"params": q[3:], "betas": (0.8, 0.99), "weight_decay": 1e-2}]  # noqa: E731
    want = ref.norm64([g.cpu().numpy() for g in grads], 0.5)
    oa = FusedAdam(groups(a), lr=LR, gradScale=0.5, maxGradNorm=want / 4)
    lib = _lib().load()
    for x, y, g in zip(a, b, grads):
        x.grad, y.grad = g.clone(), g.clone()
    before = lib.mccnn_debug_launch_count()
    oa.step()
    assert lib.mccnn_debug_launch_count() - before == 1 + 1 + 2   # one sum pass and one finish for both groups, a step each
    r = oa.grad_record
    norm, coef = float(r.norm), float(r.coef)
    assert ref.share(norm, want) <= 1.0 and np.float32(coef).tobytes() == ref.coef32(norm, want / 4).tobytes()
    ob = FusedAdam(groups(b), lr=LR, gradScale=_f32mul(0.5, coef))   # mccnn_adam_step per group with the shared grad_scale'
    ob.step()
    torch.cuda.synchronize()
    for x, y, x0 in zip(a, b, init):
        assert torch.equal(x, y) and not torch.equal(x, x0)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[x][k], ob.state[y][k])


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_the_same_inputs_give_the_same_bytes(mc):
    sizes, tensors, scalars = _many()
    fl = Flat(tensors, on_grid=True)
    rec = fl.records(scalars)
    want = ref.norm64([t["g"] for t in tensors], 0.25)
    runs = []
    for _ in range(2):
        fl.reset()
        nr = Norm()
        nr(rec, 0.25, want / 4, True)
        _clipped(rec, SCALARS, 0.25, nr.ptr())
        got, _ = fl.out()
        runs.append((got, nr.read().tobytes()))
    assert runs[0] == runs[1] and runs[0][0][0] != fl.host["p"].tobytes()
