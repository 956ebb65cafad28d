"""The optimiser step as one op (mccnn_amd.optim.FusedAdam, mccnn_adam_step) against torch's two Adams, measured in ONE process
with the settings taken in turn block by block; torch.optim.Adam (default, foreach) and torch.optim.Adam(fused=True) are the
yardsticks: python tools/adam_time.py [--part a|b|c|all] (on the GPU box).

(a) The optimiser step alone, gradients resident, on two parameter sets: the 44 tensors of MCClassS (k = 16, 40 classes) and a
    200-tensor set with the shapes of the MCSegScanNet graph (workloads.mcseg_scannet(64): the six tensors of every
    convolution, a batch-norm pair and a 1x1 layer of every convolution's width, batch-norm pairs up to 200). Per optimiser:
    wall time per step over windows of 200 steps that end in a synchronise, HIP-event time over the same window, best of five
    blocks [worst], and the library's launches per step for FusedAdam.
(b) The MCClassS cfg1 training step of tools/e2e_time.py's deepest loop (hierarchy two batches ahead + prefetch_step) with
    fused, fusedLinear and fusedLoss on, the three optimisers alternating: five blocks of 200 steps each, best block and worst.

(c) The clipped step alone, on the parameter sets of (a): FusedAdam(maxGradNorm=C), the norm and the coefficient inside the op,
    against torch.nn.utils.clip_grad_norm_(params, C, foreach=True) in front of the unclipped FusedAdam.step() -- how clipping is
    done without it -- with the unclipped FusedAdam beside them. Same windows, blocks and columns as (a).

torch's launches per step come from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats ... -- python tools/adam_time.py --part trace --opt torch --set mcclass --steps S
runs S optimiser steps and nothing else; the dispatches per step are (calls at S = 60 - calls at S = 10) / 50.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mccnn_amd import _lib, workloads  # noqa: E402
from mccnn_amd.optim import FusedAdam  # noqa: E402
from mcclass_s import MCClassS, synthetic_batch  # noqa: E402

dev = torch.device("cuda", 0)
B, N, K = 32, 1024, 16
OPTIMISERS = [("torch.optim.Adam", lambda ps: torch.optim.Adam(ps, lr=1e-3)),
              ("torch.optim.Adam(fused=True)", lambda ps: torch.optim.Adam(ps, lr=1e-3, fused=True)),
              ("FusedAdam", lambda ps: FusedAdam(ps, lr=1e-3))]
SHORT = {"torch": 0, "torch-fused": 1, "ours": 2}


def mcclass_shapes():
    net = MCClassS(1, 2, K, 40, dev)
    pts, bids = workloads.modelnet_like(64, 2, 11)
    with torch.no_grad():
        net(torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev), torch.ones((len(pts), 1), device=dev), True)
    return [tuple(p.shape) for p in net.parameters()]


def seg_shapes(count=200):
    shapes = []
    convs = workloads.mcseg_scannet(64)
    for c in convs:
        nb = workloads.conv_nb(c.fin, c.fout, c.combin)
        shapes += [(3, 8 * nb), (8 * nb,), (nb, 8, 8), (nb, 8), (nb, 8, 8), (nb, 8)]
        shapes += [(c.fout,), (c.fout,), (c.fout, c.fout), (c.fout,)]
    k = 0
    while len(shapes) < count:
        shapes += [(convs[k % len(convs)].fout,)] * 2
        k += 1
    return shapes[:count]


def make_params(shapes, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen)) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen)
    return ps


def time_steps(steppers, blocks, steps):
    """steppers: callables that run one step each -> per stepper the wall and HIP-event us per step of every block, and the
    library's launches per step; the steppers take the blocks in turn."""
    lib = _lib.load()
    wall, ev, launches = [[] for _ in steppers], [[] for _ in steppers], [0.0] * len(steppers)
    for step in steppers:
        for _ in range(20):
            step()
    for _ in range(blocks):
        for i, step in enumerate(steppers):
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            before = lib.mccnn_debug_launch_count()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            wall[i].append((time.perf_counter() - t0) / steps * 1e6)
            ev[i].append(e0.elapsed_time(e1) * 1e3 / steps)
            launches[i] = (lib.mccnn_debug_launch_count() - before) / float(steps)
    return wall, ev, launches


def part_a(blocks=5, steps=200):
    print("(a) the optimiser step alone, us per step: best of %d blocks of %d steps [worst], the optimisers in turn block by block"
          % (blocks, steps))
    print("| parameter set | tensors | elements | optimiser | wall us | HIP-event us | library launches per step |")
    print("|---|---|---|---|---|---|---|")
    for name, shapes in (("MCClassS", mcclass_shapes()), ("MCSegScanNet-like", seg_shapes())):
        opts = [make(make_params(shapes, 3)) for _, make in OPTIMISERS]
        wall, ev, launches = time_steps([o.step for o in opts], blocks, steps)
        elements = sum(int(np.prod(s)) for s in shapes)
        for i, (oname, _) in enumerate(OPTIMISERS):
            print("| %s | %d | %d | %s | %.1f [%.1f] | %.1f [%.1f] | %s |" % (
                name, len(shapes), elements, oname, min(wall[i]), max(wall[i]), min(ev[i]), max(ev[i]),
                "%.1f" % launches[i] if oname == "FusedAdam" else "-"))


CLIP = 1.0   # (below the norm of the standard normal gradients of either set: the clip is active)


def part_c(blocks=5, steps=200):
    print("(c) the clipped optimiser step alone, us per step: best of %d blocks of %d steps [worst], the settings in turn block by block"
          % (blocks, steps))
    print("| parameter set | tensors | setting | wall us | HIP-event us | library launches per step |")
    print("|---|---|---|---|---|---|")
    for name, shapes in (("MCClassS", mcclass_shapes()), ("MCSegScanNet-like", seg_shapes())):
        ps = [make_params(shapes, 3) for _ in range(3)]
        plain, behind, inside = FusedAdam(ps[0], lr=1e-3), FusedAdam(ps[1], lr=1e-3), FusedAdam(ps[2], lr=1e-3, maxGradNorm=CLIP)

        def yardstick(params=ps[1], opt=behind):
            torch.nn.utils.clip_grad_norm_(params, CLIP, foreach=True)
            opt.step()

        names = ["FusedAdam (no clipping)", "clip_grad_norm_(foreach=True) + FusedAdam", "FusedAdam(maxGradNorm=%g)" % CLIP]
        wall, ev, launches = time_steps([plain.step, yardstick, inside.step], blocks, steps)
        for i, sname in enumerate(names):
            print("| %s | %d | %s | %.1f [%.1f] | %.1f [%.1f] | %.1f%s |" % (
                name, len(shapes), sname, min(wall[i]), max(wall[i]), min(ev[i]), max(ev[i]), launches[i],
                " + torch's" if i == 1 else ""))
        win = max(wall[2]) < min(wall[1])
        print("every block of FusedAdam(maxGradNorm) below every block of the yardstick (wall): %s" % ("yes" if win else "no"))


def part_b(blocks=5, steps=200):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    net = MCClassS(1, B, K, 40, dev, fused=True, fusedLinear=True, fusedLoss=True)
    P, Bi, F, y = synthetic_batch(B, N, 40, rng, dev)
    y = y.to(torch.int32)
    net(P, Bi, F, True)   # creates the variables
    opts = [make(list(net.parameters())) for _, make in OPTIMISERS]
    torch.autograd.set_multithreading_enabled(False)
    state = {"ph": net.hierarchy(P, Bi, F)}
    net.convBuilder.hostStepsAhead_ = 1
    state["fut"] = net.prefetch_hierarchy(P, Bi, after=True)

    def deep_step(opt):
        ph_nxt = net.hierarchy(P, Bi, F, prefetched=state["fut"])
        state["fut"] = net.prefetch_hierarchy(P, Bi, after=True)
        head = net(P, Bi, F, True, hierarchy=state["ph"], nextHierarchy=ph_nxt, labels=y)
        opt.zero_grad(set_to_none=True)
        head.loss.backward()
        opt.step()
        state["ph"] = ph_nxt

    ms = [[] for _ in opts]
    for o in opts:
        for _ in range(20):
            deep_step(o)
    for _ in range(blocks):
        for i, o in enumerate(opts):
            for _ in range(10):
                deep_step(o)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                deep_step(o)
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) / steps * 1e3)
    print("(b) MCClassS cfg1 training step, fused glue, fusedLinear and fusedLoss on (hierarchy two batches ahead + prefetch_step), "
          "ms per step over %d alternating blocks of %d steps" % (blocks, steps))
    print("| optimiser | best ms | worst ms |")
    print("|---|---|---|")
    for (oname, _), t in zip(OPTIMISERS, ms):
        print("| %s | %.3f | %.3f |" % (oname, min(t), max(t)))
    print("best torch.optim.Adam / best FusedAdam = %.3f, best fused=True / best FusedAdam = %.3f" % (
        min(ms[0]) / min(ms[2]), min(ms[1]) / min(ms[2])))


def part_trace(opt, which, steps):
    shapes = mcclass_shapes() if which == "mcclass" else seg_shapes()
    o = OPTIMISERS[SHORT[opt]][1](make_params(shapes, 3))
    for _ in range(steps):
        o.step()
    torch.cuda.synchronize()
    print("%d steps of %s over %d tensors" % (steps, OPTIMISERS[SHORT[opt]][0], len(shapes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["a", "b", "c", "all", "trace"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--opt", default="torch", choices=sorted(SHORT))
    ap.add_argument("--set", default="mcclass", choices=["mcclass", "seg"])
    args = ap.parse_args()
    if args.part == "trace":
        return part_trace(args.opt, args.set, args.steps)
    if args.part in ("a", "all"):
        part_a(steps=args.steps)
    if args.part in ("b", "all"):
        part_b(steps=args.steps)
    if args.part in ("c", "all"):
        part_c(steps=args.steps)


if __name__ == "__main__":
    main()
