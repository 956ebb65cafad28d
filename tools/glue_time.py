"""The dense glue as one op (VariableStore(fused=True), dense_glue.bn_relu_dropout) against the torch path it replaces,
measured in ONE process; the torch path is the yardstick: python tools/glue_time.py [--part a|b|both] (on the GPU box).

(a) The op, forward + backward, per shape: the glue shapes an MCClassS 32 x 1024 step sees (taken from a forward pass) plus
    (100000, 64) and (131072, 32). HIP events, best of five runs of 50 calls after a warm-up, worst in brackets; library
    launches per call (mccnn_debug_launch_count); GB/s of algorithmic bytes (forward 12 n c, backward 20 n c).
(b) The whole training step of tools/e2e_time.py's deepest loop (hierarchy two batches ahead + prefetch_step, Adam) with
    fused off and on, alternating blocks: five blocks of 200 steps each, best block and worst.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mccnn_amd.MCNetworkUtils as U  # noqa: E402
from mccnn_amd import _lib  # noqa: E402
from mcclass_s import MCClassS, synthetic_batch  # noqa: E402

dev = torch.device("cuda", 0)
B, N, K = 32, 1024, 16


def glue_shapes(net, P, Bi, F):
    """(n, c, relu, keepProb) of every fused glue call of one training forward pass."""
    seen = []
    assert U._fused_native() is not None, "the library does not load"
    gate = U._fused_glue

    def record(st, x, training, name, relu, keepProb=None, **rest):
        y = gate(st, x, training, name, relu, keepProb, **rest)
        if y is not None:
            seen.append((int(x.shape[0]), int(x.shape[1]), bool(relu), keepProb))
        return y

    was = net.store.fused_
    U._fused_glue, net.store.fused_ = record, True
    try:
        with torch.no_grad():
            net(P, Bi, F, True)
    finally:
        U._fused_glue, net.store.fused_ = gate, was
    return seen


def time_op(n, c, relu, keepProb, fused, calls=50, runs=5):
    """-> (best us, worst us, library launches per call) of forward + backward of one glue block."""
    lib = _lib.load()
    st = U.VariableStore(dev, fused=fused)
    x = (torch.randn(n, c, device=dev) * 2 + 3).requires_grad_(True)
    dy = torch.randn(n, c, device=dev)

    def call():
        y = (U._bn_relu_drop(st, x, True, "T", keepProb is not None, keepProb) if relu else
             (U._fused_glue(st, x, True, "T", False) if fused else U.batch_normalization(x, True, "T", st)))
        x.grad = None
        y.backward(dy)

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    before = lib.mccnn_debug_launch_count()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / calls)
    launches = (lib.mccnn_debug_launch_count() - before) / float(runs * calls)
    return min(times), max(times), launches


def part_a(net, P, Bi, F):
    shapes = glue_shapes(net, P, Bi, F) + [(100000, 64, True, None), (131072, 32, True, None)]
    print("(a) one glue block, forward + backward, us per call: best of 5 runs of 50 calls [worst]")
    print("| n | c | relu | keepProb | torch us | fused us | torch / fused | fused launches | fused GB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n, c, relu, kp in shapes:
        t = time_op(n, c, relu, kp, False)
        f = time_op(n, c, relu, kp, True)
        print("| %d | %d | %s | %s | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f | %.0f |" % (
            n, c, "yes" if relu else "no", "-" if kp is None else "%g" % kp, t[0], t[1], f[0], f[1], t[0] / f[0], f[2],
            32.0 * n * c / (f[0] * 1e-6) / 1e9))
        assert t[2] == 0.0, "the torch path launched library kernels"


def part_b(net, P, Bi, F, y, blocks=5, steps=200):
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    torch.autograd.set_multithreading_enabled(False)
    state = {"ph": net.hierarchy(P, Bi, F)}
    net.convBuilder.hostStepsAhead_ = 1
    state["fut"] = net.prefetch_hierarchy(P, Bi, after=True)

    def deep_step():
        ph_nxt = net.hierarchy(P, Bi, F, prefetched=state["fut"])
        state["fut"] = net.prefetch_hierarchy(P, Bi, after=True)
        logits = net(P, Bi, F, True, hierarchy=state["ph"], nextHierarchy=ph_nxt)
        loss = torch.nn.functional.cross_entropy(logits, y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        state["ph"] = ph_nxt

    ms = {False: [], True: []}
    for fused in (False, True):
        net.store.fused_ = fused
        for _ in range(20):
            deep_step()
    for _ in range(blocks):
        for fused in (False, True):
            net.store.fused_ = fused
            for _ in range(10):
                deep_step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                deep_step()
            torch.cuda.synchronize()
            ms[fused].append((time.perf_counter() - t0) / steps * 1e3)
    print("(b) MCClassS cfg1 training step (hierarchy two batches ahead + prefetch_step, Adam), ms per step over %d "
          "alternating blocks of %d steps" % (blocks, steps))
    print("| fused | best ms | worst ms |")
    print("|---|---|---|")
    for fused in (False, True):
        print("| %s | %.3f | %.3f |" % ("on" if fused else "off", min(ms[fused]), max(ms[fused])))
    print("best off / best on = %.3f" % (min(ms[False]) / min(ms[True])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["a", "b", "both"])
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    net = MCClassS(1, B, K, 40, dev)
    P, Bi, F, y = synthetic_batch(B, N, 40, rng, dev)
    net(P, Bi, F, True)   # creates the variables
    if args.part in ("a", "both"):
        part_a(net, P, Bi, F)
    if args.part in ("b", "both"):
        part_b(net, P, Bi, F, y, steps=args.steps)


if __name__ == "__main__":
    main()
