"""A linear layer + the dense glue behind it as one op (VariableStore(fusedLinear=True), dense_glue.linear_bn_relu_dropout)
against the path it replaces -- conv_1x1 on rocBLAS + the fused glue -- measured in ONE process; the switch-off path is the
yardstick: python tools/linear_glue_time.py [--part a|b|c|all] (on the GPU box).

(a) One block forward + backward through the helpers, fusedLinear off against on, per shape: the blocks of an MCClassS
    32 x 1024 step plus three large ones. HIP events, best of five runs of 50 calls after a warm-up, worst in brackets;
    library launches per call (mccnn_debug_launch_count).
(b) Kernel-only C-ABI calls back to back, forward and backward, against torch.addmm + mccnn_bn_act_* on the same buffers:
    TFLOP/s of algorithmic work (forward 2 n cin cout, backward 4 n cin cout) and GB/s of algorithmic bytes (forward
    4 (n cin + cin cout + 2 n cout), backward 4 (n cin + cin cout + 2 n cout + n cin + cin cout)).
(c) The whole training step of tools/e2e_time.py's deepest loop (hierarchy two batches ahead + prefetch_step, Adam) with
    fused on and fusedLinear off and on, alternating blocks: five blocks of 200 steps each, best block and worst.
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
SHAPES = [(3517, 16, 32), (230, 32, 64), (32, 64, 32), (32, 32, 16), (131072, 16, 32), (100000, 64, 64), (8192, 384, 128)]


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


def part_a():
    print("(a) one block (conv_1x1 + batch norm + ReLU + dropout 0.8), forward + backward through the helpers, us per call: "
          "best of 5 runs of 50 calls [worst]")
    print("| n | cin -> cout | fusedLinear off us | on us | off / on | launches off | launches on |")
    print("|---|---|---|---|---|---|---|")
    for n, cin, cout in SHAPES:
        x = (torch.randn(n, cin, device=dev) * 2 + 3).requires_grad_(True)
        dy = torch.randn(n, cout, device=dev)
        res = []
        for fl in (False, True):
            st = U.VariableStore(dev, fused=True, fusedLinear=fl)

            def call():
                y = U.conv_1x1_batch_norm_RELU_drop_out("R", "R_Out", x, cin, cout, True, True, 0.8, st)
                x.grad = None
                y.backward(dy)

            res.append(best_of(call))
        off, on = res
        print("| %d | %d -> %d | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f | %.1f |" % (
            n, cin, cout, off[0], off[1], on[0], on[1], off[0] / on[0], off[2], on[2]))


def part_b():
    lib = _lib.load()
    print("(b) kernel-only C-ABI calls back to back, us per call: best of 5 runs of 50 calls [worst]; TFLOP/s and GB/s of "
          "algorithmic work of the new op")
    print("| n | cin -> cout | fwd addmm + bn_act us | fwd op us | TFLOP/s | GB/s | bwd mm + bn_act us | bwd op us | TFLOP/s | GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    T = 1 << 32
    for n, cin, cout in SHAPES:
        x = torch.randn(n, cin, device=dev) * 2 + 3
        w = torch.randn(cin, cout, device=dev) / cin ** 0.5
        b, g, be = torch.randn(cout, device=dev), torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
        mm, mv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
        z, y, dy, dz = (torch.empty(n, cout, device=dev) for _ in range(4))
        dy.normal_()
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        saved, dv = torch.empty(3, cout, device=dev), torch.empty(3, cout, device=dev)
        ws = _ws(max(lib.mccnn_linear_bn_act_workspace_bytes(n, cin, cout), lib.mccnn_bn_act_workspace_bytes(n, cout)), dev)
        sh = _lib.stream_handle()
        p = lambda t: t.data_ptr()  # noqa: E731

        def fwd_ref():
            torch.addmm(b, x, w, out=z)
            _lib.check(lib.mccnn_bn_act_fwd(p(z), n, cout, p(g), p(be), p(mm), p(mv), 0.99, 1e-3, 1, 1, T, 1.0, 0, p(y), p(saved),
                                            p(ws), ws.numel(), sh), "bn_act_fwd")

        def fwd_op():
            _lib.check(lib.mccnn_linear_bn_act_fwd(p(x), p(w), p(b), n, cin, cout, p(g), p(be), p(mm), p(mv), 0.99, 1e-3, 1, 1, T,
                                                   1.0, 0, p(z), p(y), 0, p(saved), p(ws), ws.numel(), sh), "linear_bn_act_fwd")

        def bwd_ref():
            _lib.check(lib.mccnn_bn_act_bwd(p(z), p(dy), n, cout, p(g), p(be), p(saved), 1, T, 1.0, 0, p(dz), p(dv[1]), p(dv[2]),
                                            p(ws), ws.numel(), sh), "bn_act_bwd")
            torch.mm(dz, w.t(), out=dx)
            torch.mm(x.t(), dz, out=dw)
            torch.sum(dz, 0, out=dv[0])

        def bwd_op():
            _lib.check(lib.mccnn_linear_bn_act_bwd(p(x), p(w), p(z), p(dy), 0, n, cin, cout, p(g), p(be), p(saved), 1, T, 1.0, 0,
                                                   p(dx), p(dw), p(dv[0]), p(dv[1]), p(dv[2]), p(ws), ws.numel(), sh),
                       "linear_bn_act_bwd")

        fr = best_of(fwd_ref)
        fo = best_of(fwd_op)     # (leaves the op's own z and saved for the backward calls)
        br = best_of(bwd_ref)
        bo = best_of(bwd_op)
        flop = 2.0 * n * cin * cout
        fbytes = 4.0 * (n * cin + cin * cout + 2 * n * cout)
        bbytes = fbytes + 4.0 * (n * cin + cin * cout)
        print("| %d | %d -> %d | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.0f | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.0f |" % (
            n, cin, cout, fr[0], fr[1], fo[0], fo[1], flop / (fo[0] * 1e-6) / 1e12, fbytes / (fo[0] * 1e-6) / 1e9,
            br[0], br[1], bo[0], bo[1], 2 * flop / (bo[0] * 1e-6) / 1e12, bbytes / (bo[0] * 1e-6) / 1e9))


def part_c(blocks=5, steps=200):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    net = MCClassS(1, B, K, 40, dev, fused=True, fusedLinear=True)
    P, Bi, F, y = synthetic_batch(B, N, 40, rng, dev)
    net(P, Bi, F, True)   # creates the variables
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    torch.autograd.set_multithreading_enabled(False)
    state = {"ph": net.hierarchy(P, Bi, F)}
    net.convBuilder.hostStepsAhead_ = 1
    state["fut"] = net.prefetch_hierarchy(P, Bi, after=True)

    def switch(on):
        net.fusedLinear = on
        net.store.fusedLinear_ = on

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
    print("(c) MCClassS cfg1 training step, fused glue on (hierarchy two batches ahead + prefetch_step, Adam), ms per step over "
          "%d alternating blocks of %d steps" % (blocks, steps))
    print("| fusedLinear | best ms | worst ms |")
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
