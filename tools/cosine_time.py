"""The cosine-distance loss of normal estimation as one op (VariableStore(fusedLoss=True), dense_glue.cosine_distance_loss)
against the torch code of the same definition (MCNetworkUtils._normal_head: two l2_normalize, multiply, reduce, 1 - ., the
live rule, the mean, and the atan2 angle metric), measured in ONE process; the torch path is the yardstick:
python tools/cosine_time.py [--part a|b|c|all] (on the GPU box).

(a) One head forward + backward through the helper (MCNetworkUtils.cosine_distance_loss), fusedLoss off against on, per shape
    (n, c); (32768, 3) is the MCNormS 32 x 1024 shape. HIP events, best of five runs of 50 calls after a warm-up, worst in
    brackets; library launches per call (mccnn_debug_launch_count).
(b) Kernel-only C-ABI calls back to back, forward and backward, against the torch code under no_grad and its autograd backward
    on the same buffers, with GB/s of algorithmic bytes (8 n c forward, 12 n c backward).
(c) An MCNormS training step, 32 x 1024 points (hierarchy a step ahead + prefetch_step, Adam, fused glue on), fusedLoss off
    and on alternating: five blocks of 200 steps each, best block and worst. Both ways the loop hands the normals to the network
    and takes the loss from its NormalHead.
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
from mcclass_s import MCNormS, synthetic_normals_batch  # noqa: E402

dev = torch.device("cuda", 0)
B, N, K = 32, 1024, 16
SHAPES = [(1024, 3), (32768, 3), (131072, 3), (32768, 16)]


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


def _rows(n, c, weighted):
    rng = np.random.default_rng(n + c)
    p = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)).to(dev)
    t = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)).to(dev)
    rw = torch.from_numpy((rng.uniform(0.25, 4, n) * (rng.random(n) > 0.1)).astype(np.float32)).to(dev) if weighted else None
    return p, t, rw


def part_a():
    print("(a) one head (cosine-distance loss + cosine and angle sums), forward + backward through the helper, us per call: "
          "best of 5 runs of 50 calls [worst]")
    print("| n | c | weights | fusedLoss off us | on us | off / on | launches on |")
    print("|---|---|---|---|---|---|---|")
    for n, c in SHAPES:
        for weighted in (False, True):
            p, t, rw = _rows(n, c, weighted)
            p.requires_grad_(True)
            res = []
            for on in (False, True):
                st = U.VariableStore(dev, fusedLoss=on)

                def call():
                    head = U.cosine_distance_loss(p, t, rw, store=st)
                    p.grad = None
                    head.loss.backward()

                res.append(best_of(call))
            off, on = res
            print("| %d | %d | %s | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f |" % (
                n, c, "yes" if weighted else "no", off[0], off[1], on[0], on[1], off[0] / on[0], on[2]))


def part_b():
    lib = _lib.load()
    print("(b) kernel-only C-ABI calls back to back, us per call: best of 5 runs of 50 calls [worst]; the stock path is the torch "
          "code of the helper under no_grad (forward) and its autograd backward (dpred); GB/s of 8 n c (forward) and 12 n c "
          "(backward) bytes at the op's best")
    print("| n | c | fwd stock us | fwd op us | stock / op | fwd GB/s | bwd stock us | bwd op us | stock / op | bwd GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for n, c in SHAPES:
        pr, t, _ = _rows(n, c, False)
        pr.requires_grad_(True)
        loss, sums = torch.empty(1, device=dev), torch.empty(2, device=dev)
        meta = torch.empty(1, dtype=torch.int32, device=dev)
        g = torch.ones(1, device=dev)
        dp = torch.empty(n, c, device=dev)
        ws = _ws(lib.mccnn_cosine_loss_workspace_bytes(n, c), dev)
        sh = _lib.stream_handle()
        p = lambda x: x.data_ptr()  # noqa: E731
        state = {}

        def fwd_ref():
            with torch.no_grad():
                U._normal_head(pr, t)

        def fwd_op():
            _lib.check(lib.mccnn_cosine_loss_fwd(p(pr), p(t), n, c, None, p(loss), p(sums), p(meta), _lib.ptr(ws), ws.numel(), sh),
                       "cosine_loss_fwd")

        def bwd_ref():
            torch.autograd.grad(state["loss"], (pr,), retain_graph=True)

        def bwd_op():
            _lib.check(lib.mccnn_cosine_loss_bwd(p(pr), p(t), n, c, None, p(meta), p(g), p(dp), sh), "cosine_loss_bwd")

        fr = best_of(fwd_ref)
        fo = best_of(fwd_op)     # (leaves the op's own meta for the backward calls)
        state["loss"] = U._normal_head(pr, t).loss
        br = best_of(bwd_ref)
        bo = best_of(bwd_op)
        print("| %d | %d | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f |" % (
            n, c, fr[0], fr[1], fo[0], fo[1], fr[0] / fo[0], 8.0 * n * c / fo[0] * 1e-3, br[0], br[1], bo[0], bo[1], br[0] / bo[0],
            12.0 * n * c / bo[0] * 1e-3))


def part_c(blocks=5, steps=200):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    net = MCNormS(1, B, K, dev, fused=True)
    P, Bi, F, Nrm = synthetic_normals_batch(B, N, rng, dev)
    net(P, Bi, F, True)   # creates the variables
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    torch.autograd.set_multithreading_enabled(False)
    state = {"ph": net.hierarchy(P, Bi, F)}
    net.convBuilder.hostStepsAhead_ = 1

    def switch(on):
        net.store.fusedLoss_ = on

    def deep_step():
        ph_nxt = net.hierarchy(P, Bi, F)
        head = net(P, Bi, F, True, normals=Nrm, hierarchy=state["ph"], nextHierarchy=ph_nxt)
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
    print("(c) MCNormS training step, %d x %d points, fused glue on (hierarchy a step ahead + prefetch_step, Adam), ms per step "
          "over %d alternating blocks of %d steps" % (B, N, blocks, steps))
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
