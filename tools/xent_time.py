"""The last linear layer + softmax cross-entropy as one op (VariableStore(fusedLoss=True), dense_glue.linear_softmax_xent)
against the path it replaces -- the matmul on rocBLAS, log_softmax, the weighted sum over the live rows, arg-max -- measured
in ONE process; the switch-off path is the yardstick: python tools/xent_time.py [--part a|b|c|all] (on the GPU box).

(a) One head forward + backward through the helpers (conv_1x1_softmax_cross_entropy), fusedLoss off against on, per shape:
    two classification heads, a ScanNet-like and a ShapeNet-like per-point head. HIP events, best of five runs of 50 calls
    after a warm-up, worst in brackets; library launches per call (mccnn_debug_launch_count).
(b) Kernel-only C-ABI calls back to back, forward and backward, against torch.addmm + torch.nn.functional.cross_entropy +
    argmax (forward) and their autograd backward on the same buffers.
(c) The whole training step of tools/e2e_time.py's deepest loop (hierarchy two batches ahead + prefetch_step, Adam) with
    fused and fusedLinear on, fusedLoss off and on alternating: five blocks of 200 steps each, best block and worst. Both
    ways the loop hands the labels to the network and takes the loss from its LossHead.
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
from mccnn_amd.MCConvModule import _ws  # noqa: E402
from mcclass_s import MCClassS, synthetic_batch  # noqa: E402

dev = torch.device("cuda", 0)
B, N, K = 32, 1024, 16
SHAPES = [(32, 16, 40), (32, 64, 40), (8192, 64, 21), (131072, 128, 50)]


def best_of(call, calls=50, runs=5, warm=10):
    """-> (best us, worst us, library launches per call)."""
    lib = _lib.load()
    for _ in range(warm):
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
    return min(times), max(times), (lib.mccnn_debug_launch_count() - before) / float(runs * calls)


def _labels(n, c, weighted):
    rng = np.random.default_rng(n + c)
    y = torch.from_numpy(rng.integers(0, c, n).astype(np.int32)).to(dev)
    rw = torch.from_numpy(rng.uniform(0.25, 4, n).astype(np.float32)).to(dev) if weighted else None
    return y, rw


def part_a():
    print("(a) one head (conv_1x1 + softmax cross-entropy + arg-max + correct count), forward + backward through the helpers, "
          "us per call: best of 5 runs of 50 calls [worst]")
    print("| n | cin -> C | weights | fusedLoss off us | on us | off / on | launches on |")
    print("|---|---|---|---|---|---|---|")
    for n, cin, c in SHAPES:
        x = (torch.randn(n, cin, device=dev) * 2 + 1).requires_grad_(True)
        for weighted in (False, True):
            y, rw = _labels(n, c, weighted)
            res = []
            for on in (False, True):
                st = U.VariableStore(dev, fusedLoss=on)

                def call():
                    head = U.conv_1x1_softmax_cross_entropy("L", x, cin, c, y, rw, False, st)
                    x.grad = None
                    head.loss.backward()

                res.append(best_of(call))
            off, on = res
            print("| %d | %d -> %d | %s | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f |" % (
                n, cin, c, "yes" if weighted else "no", off[0], off[1], on[0], on[1], off[0] / on[0], on[2]))


def part_b():
    lib = _lib.load()
    print("(b) kernel-only C-ABI calls back to back, us per call: best of 5 runs of 50 calls [worst]; the stock path is "
          "torch.addmm + cross_entropy + argmax forward and its autograd backward (dx, dW, db)")
    print("| n | cin -> C | fwd stock us | fwd op us | stock / op | bwd stock us | bwd op us | stock / op |")
    print("|---|---|---|---|---|---|---|---|")
    for n, cin, c in SHAPES:
        x = (torch.randn(n, cin, device=dev) * 2 + 1).requires_grad_(True)
        w = (torch.randn(cin, c, device=dev) / cin ** 0.5).requires_grad_(True)
        b = torch.randn(c, device=dev).requires_grad_(True)
        y, _ = _labels(n, c, False)
        y64 = y.to(torch.int64)
        loss, lse = torch.empty(1, device=dev), torch.empty(n, device=dev)
        meta, pred = torch.empty(2, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        g = torch.ones(1, device=dev)
        dx, dw, db = torch.empty(n, cin, device=dev), torch.empty(cin, c, device=dev), torch.empty(c, device=dev)
        ws = _ws(lib.mccnn_linear_xent_workspace_bytes(n, cin, c), dev)
        sh = _lib.stream_handle()
        p = lambda t: t.data_ptr()  # noqa: E731
        state = {}

        def fwd_ref():
            with torch.no_grad():
                z = torch.addmm(b, x, w)
                torch.nn.functional.cross_entropy(z, y64)
                z.argmax(1)

        def fwd_op():
            _lib.check(lib.mccnn_linear_xent_fwd(p(x), p(w), p(b), n, cin, c, p(y), None, p(loss), p(lse), p(meta), p(pred), None,
                                                 p(ws), ws.numel(), sh), "linear_xent_fwd")

        def bwd_ref():
            torch.autograd.grad(state["loss"], (x, w, b), retain_graph=True)

        def bwd_op():
            _lib.check(lib.mccnn_linear_xent_bwd(p(x), p(w), p(b), n, cin, c, p(y), None, p(lse), p(meta), p(g), p(dx), p(dw), p(db),
                                                 p(ws), ws.numel(), sh), "linear_xent_bwd")

        fr = best_of(fwd_ref)
        fo = best_of(fwd_op)     # (leaves the op's own lse and meta for the backward calls)
        state["loss"] = torch.nn.functional.cross_entropy(torch.addmm(b, x, w), y64)
        br = best_of(bwd_ref)
        bo = best_of(bwd_op)
        print("| %d | %d -> %d | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f [%.1f] | %.1f [%.1f] | %.2f |" % (
            n, cin, c, fr[0], fr[1], fo[0], fo[1], fr[0] / fo[0], br[0], br[1], bo[0], bo[1], br[0] / bo[0]))


def part_c(blocks=5, steps=200):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    net = MCClassS(1, B, K, 40, dev, fused=True, fusedLinear=True)
    P, Bi, F, y = synthetic_batch(B, N, 40, rng, dev)
    y = y.to(torch.int32)
    net(P, Bi, F, True)   # creates the variables
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    torch.autograd.set_multithreading_enabled(False)
    state = {"ph": net.hierarchy(P, Bi, F)}
    net.convBuilder.hostStepsAhead_ = 1
    state["fut"] = net.prefetch_hierarchy(P, Bi, after=True)

    def switch(on):
        net.store.fusedLoss_ = on

    def deep_step():
        ph_nxt = net.hierarchy(P, Bi, F, prefetched=state["fut"])
        state["fut"] = net.prefetch_hierarchy(P, Bi, after=True)
        head = net(P, Bi, F, True, hierarchy=state["ph"], nextHierarchy=ph_nxt, labels=y)
        opt.zero_grad(set_to_none=True)
        head.loss.backward()
        opt.step()
        state["ph"] = ph_nxt

    ms = {False: [], True: []}
    for on in (False, True):
        switch(on)
        for _ in range(20):
            deep_step()
    for _ in range(blocks):
        for on in (False, True):
            switch(on)
            for _ in range(10):
                deep_step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                deep_step()
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / steps * 1e3)
    print("(c) MCClassS cfg1 training step, fused glue and fusedLinear on (hierarchy two batches ahead + prefetch_step, Adam), "
          "ms per step over %d alternating blocks of %d steps" % (blocks, steps))
    print("| fusedLoss | best ms | worst ms |")
    print("|---|---|---|")
    for on in (False, True):
        print("| %s | %.3f | %.3f |" % ("on" if on else "off", min(ms[on]), max(ms[on])))
    print("best off / best on = %.3f" % (min(ms[False]) / min(ms[True])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["a", "b", "c", "all"])
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if args.part in ("a", "all"):
        part_a()
    if args.part in ("b", "all"):
        part_b()
    if args.part in ("c", "all"):
        part_c(steps=args.steps)


if __name__ == "__main__":
    main()
