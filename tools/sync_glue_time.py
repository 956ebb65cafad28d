"""The dense glue with batch statistics across ranks (mccnn_bn_sync_*, VariableStore(fused=True, fusedSync=True)) against
what it stands beside, each pair measured in ONE process: python tools/sync_glue_time.py [--part a|b|both] (on the GPU box).

(a) Kernel-only, one rank (world = 1), through the C-ABI: stats + apply against mccnn_bn_act_fwd, sums + dx against
    mccnn_bn_act_bwd, at (3517, 32), (100000, 64) and (131072, 128), f32, relu, no dropout. The yardstick is the plain op.
    HIP events, best of five runs of 50 calls after a warm-up, worst in brackets.
(b) Two ranks: one glue block, forward + backward through the helpers, and an MCClassS cfg1 training step (each rank half
    of the 32 clouds; gradient all-reduce, Adam), with fusedSync off -- the torch sync path -- and on, alternating in one
    process group, five blocks each. With two GPUs: nccl, one GPU per rank. On a one-GPU machine: gloo ranks SHARING the
    GPU, which times the host path (collectives through host memory) and not RCCL. Rank 0 reports.
"""
import argparse
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N, K = 32, 1024, 16


def _events(call, calls=50, runs=5, warm=10):
    """-> (best us, worst us) per call."""
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / calls)
    return min(times), max(times)


def part_a():
    from mccnn_amd import _lib
    from mccnn_amd.MCConvModule import _ws
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    thr, st = 1 << 32, _lib.stream_handle()
    print("(a) kernel-only, world = 1, f32, us per call: best of 5 runs of 50 calls [worst]; the plain op is the yardstick")
    print("| n | c | plain fwd | stats + apply | ratio | plain bwd | sums + dx | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    for n, c in ((3517, 32), (100000, 64), (131072, 128)):
        x, dy = torch.randn(n, c, device=dev) * 2 + 3, torch.randn(n, c, device=dev)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        g, b, mm, mv, dg, db = (torch.ones(c, device=dev) for _ in range(6))
        saved, meta = torch.empty(2, c, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
        parts = torch.empty(1, 3 * c, device=dev)
        ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), dev)
        P = lambda t: t.data_ptr()  # noqa: E731

        def plain_fwd():
            lib.mccnn_bn_act_fwd(P(x), n, c, P(g), P(b), P(mm), P(mv), 0.99, 1e-3, 1, 1, thr, 1.0, 0, P(y), P(saved), P(ws), ws.numel(), st)

        def sync_fwd():
            lib.mccnn_bn_sync_stats(P(x), 0, n, c, 0, 1, P(parts), P(ws), ws.numel(), st)
            lib.mccnn_bn_sync_apply(P(x), 0, n, c, 0, 1, P(parts), P(g), P(b), P(mm), P(mv), 0.99, 1e-3, 1, thr, 1.0, 0, P(y), 0,
                                    P(saved), P(meta), st)

        def plain_bwd():
            lib.mccnn_bn_act_bwd(P(x), P(dy), n, c, P(g), P(b), P(saved), 1, thr, 1.0, 0, P(dx), P(dg), P(db), P(ws), ws.numel(), st)

        def sync_bwd():
            lib.mccnn_bn_sync_bwd_sums(P(x), 0, P(dy), 0, n, c, 0, 1, P(g), P(b), P(saved), P(meta), 1, thr, 1.0, 0, P(parts), P(dg),
                                       P(db), P(ws), ws.numel(), st)
            lib.mccnn_bn_sync_bwd_dx(P(x), 0, P(dy), 0, n, c, 0, 1, P(g), P(b), P(parts), P(saved), P(meta), 1, thr, 1.0, 0, P(dx),
                                     P(dg), st)

        sync_fwd()                                              # (saved and meta for the backward)
        pf, sf, pb, sb = _events(plain_fwd), _events(sync_fwd), _events(plain_bwd), _events(sync_bwd)
        print("| %d | %d | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f [%.1f] | %.1f [%.1f] | %.2f |" % (
            n, c, pf[0], pf[1], sf[0], sf[1], sf[0] / pf[0], pb[0], pb[1], sb[0], sb[1], sb[0] / pb[0]))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _alternate(store, run, blocks, steps, warm):
    """ms per call of run() with store.fusedSync_ off and on, alternating blocks -> {False: [...], True: [...]}."""
    ms = {False: [], True: []}
    for on in (False, True):
        store.fusedSync_ = on
        for _ in range(warm):
            run()
    for _ in range(blocks):
        for on in (False, True):
            store.fusedSync_ = on
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / steps * 1e3)
    return ms


def _rank(rank, world, port, backend, steps):
    import torch.distributed as dist
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    from mccnn_amd.dist import GradBucket
    from mcclass_s import MCClassS, synthetic_batch
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    gpu = rank if backend == "nccl" else 0
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        lib = _lib.load()
        say = print if rank == 0 else (lambda *a: None)
        say("(b) two ranks over %s%s: ms per call over 5 alternating blocks, best [worst]" % (
            backend, "" if backend == "nccl" else " SHARING one GPU -- this times the host path, not RCCL"))
        # one block, forward + backward through the helpers
        for n, c in ((3517, 32), (16384, 64)):
            st = U.VariableStore(dev, fused=True, fusedSync=False)
            x = (torch.randn(n + 100 * rank, c, device=dev) * 2 + 3).requires_grad_(True)
            dy = torch.randn_like(x)

            def block():
                y = U.batch_norm_RELU_drop_out("T", x, True, True, 0.7, st)
                x.grad = None
                y.backward(dy)

            before = lib.mccnn_debug_launch_count()
            ms = _alternate(st, block, 5, steps, 10)
            launched = lib.mccnn_debug_launch_count() - before
            say("| block (%d, %d) | fusedSync off %.3f [%.3f] | on %.3f [%.3f] | off / on %.2f | library launches %d |" % (
                n, c, min(ms[False]), max(ms[False]), min(ms[True]), max(ms[True]), min(ms[False]) / min(ms[True]), launched))
        # the MCClassS cfg1 training step, half of the clouds per rank
        torch.manual_seed(0)
        net = MCClassS(1, B // world, K, 40, dev, fused=True, fusedLinear=True, fusedSync=False)
        P, Bi, F, y = synthetic_batch(B // world, N, 40, np.random.default_rng(rank), dev)
        net(P, Bi, F, True)                                     # creates the variables
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        bucket = GradBucket(list(net.parameters()))

        def step():
            logits = net(P, Bi, F, True)
            loss = torch.nn.functional.cross_entropy(logits, y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            bucket.allreduce(average=True)
            opt.step()

        ms = _alternate(net.store, step, 5, max(steps // 4, 5), 5)
        say("| MCClassS cfg1 step | fusedSync off %.3f [%.3f] | on %.3f [%.3f] | off / on %.2f |" % (
            min(ms[False]), max(ms[False]), min(ms[True]), max(ms[True]), min(ms[False]) / min(ms[True])))
    finally:
        dist.destroy_process_group()


def part_b(steps):
    import torch.multiprocessing as mp
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, backend, steps)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=900)
        if p.exitcode != 0:
            for q in procs:
                if q.is_alive():
                    q.terminate()
            raise SystemExit("a rank ended with exit code %s" % p.exitcode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["a", "b", "both"])
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    if args.part in ("a", "both"):
        part_a()
    if args.part in ("b", "both"):
        part_b(args.steps)


if __name__ == "__main__":
    main()
