"""The dense glue over a concatenation (VariableStore(fused=True, fusedCat=True), dense_glue.bn_relu_dropout_cat) against
the path it replaces -- torch.cat, the contiguous op, column slices of its gradient made contiguous -- measured in ONE
process with the two settings alternating block by block; the off path is the yardstick:
    python tools/cat_glue_time.py [--part a|b|both] [--batch 16] [--points 8192] [--k 32] [--steps 200] [--bf16-rows]   (on the GPU box)

(a) Per glue shape: MCSeg's six blocks over a concatenation at the given size (rows per level from the built hierarchy),
    forward + backward through batch_norm_RELU_drop_out with fused_ on, fusedCat_ off against on. The segments' gradients
    are consumed as contiguous tensors on both paths (the convolution backward copies a non-contiguous one). HIP events,
    best of five blocks of 50 calls, worst in brackets; library launches per call (mccnn_debug_launch_count).
(b) The whole training step of examples/mcseg.py with every fused switch on, fusedCat off against on: five alternating
    blocks of --steps steps; a gain only if EVERY on block is below EVERY off block.
--bf16-rows: MCSeg(rows=torch.bfloat16), the cfg3 form. The depth-wise layers then return bf16 rows, so (a) times the six
    blocks with the segment types they have in that network -- bf16 throughout but for the f32 block of Conv_1 in
    DeConv_1_Reduce_In_BN -- and the off path is torch.cat of the typed segments (which widens a mixed list), the contiguous op
    and autograd's slices cast back; (b) is the step of examples/mcseg.py --bf16-rows.
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
from mcclass_s import NUM_PARTS, part_labels, synthetic_normals_batch  # noqa: E402
from mcseg import MCSeg  # noqa: E402

dev = torch.device("cuda", 0)


def cat_shapes(levels, k, bf16_rows=False):
    """(block name, rows, segment widths, segment types, y's type) of MCSeg's six blocks over a concatenation; bf16_rows: the
    types of MCSeg(rows=torch.bfloat16) -- every segment a depth-wise layer's output but the last of DeConv_1_Reduce_In_BN
    (Conv_1), y float32 into a matmul and bf16 into the depth-wise Up_3_4."""
    f, b = torch.float32, torch.bfloat16 if bf16_rows else torch.float32
    return [("Reduce_Pool_2_In_BN", levels[1], (2 * k, 2 * k), (b, b), f), ("Reduce_Pool_3_In_BN", levels[2], (4 * k, 4 * k), (b, b), f),
            ("Up_3_4_BN", levels[3], (8 * k, 8 * k), (b, b), b), ("DeConv_3_Reduce_In_BN", levels[2], (16 * k, 4 * k, 4 * k), (b, b, b), f),
            ("DeConv_2_Reduce_In_BN", levels[1], (8 * k, 2 * k, 2 * k), (b, b, b), f),
            ("DeConv_1_Reduce_In_BN", levels[0], (4 * k, 8 * k, k), (b, b, f), f)]


def time_block(n, widths, types=None, out=None, calls=50, blocks=5):
    """-> {fusedCat: (best us, worst us, library launches per call)} of forward + backward of one block, alternating."""
    lib = _lib.load()
    types = types or (torch.float32,) * len(widths)
    xs = [(torch.randn(n, w, device=dev) * 2 + 3).to(t).requires_grad_(True) for w, t in zip(widths, types)]
    dy = torch.randn(n, sum(widths), device=dev).to(out or torch.float32)
    stores = {c: U.VariableStore(dev, fused=True, fusedCat=c) for c in (False, True)}

    def call(st):
        y = U.batch_norm_RELU_drop_out("T", xs, True, False, None, st, outDtype=out)
        for x in xs:
            x.grad = None
        y.backward(dy)
        return [x.grad.contiguous() for x in xs]   # (what the layer in front of the block reads)

    times, launches = {False: [], True: []}, {}
    for c in (False, True):
        for _ in range(10):
            call(stores[c])
    for _ in range(blocks):
        for c in (False, True):
            torch.cuda.synchronize()
            before = lib.mccnn_debug_launch_count()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call(stores[c])
            e1.record()
            e1.synchronize()
            times[c].append(e0.elapsed_time(e1) * 1e3 / calls)
            launches[c] = (lib.mccnn_debug_launch_count() - before) / float(calls)
    return {c: (min(times[c]), max(times[c]), launches[c]) for c in (False, True)}


def part_a(levels, k, bf16_rows=False):
    print("(a) one block over a concatenation, forward + backward, us per call: best of 5 alternating blocks of 50 calls [worst]")
    print("| block | n | segments | fusedCat off us | on us | off / on | launches off | on | every on block below every off block |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, n, widths, types, out in cat_shapes(levels, k, bf16_rows):
        r = time_block(n, widths, types, out if bf16_rows else None)
        print("| %s | %d | %s | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f | %.1f | %s |" % (
            name, n, "+".join("%d%s" % (w, " bf16" if t == torch.bfloat16 else "") for w, t in zip(widths, types)), r[False][0], r[False][1], r[True][0], r[True][1], r[False][0] / r[True][0],
            r[False][2], r[True][2], "yes" if r[True][1] < r[False][0] else "no"))


def part_b(net, batch, blocks=5, steps=200):
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    torch.autograd.set_multithreading_enabled(False)
    P, Bi, F, cats, y = batch

    def step():
        head = net(P, Bi, F, cats, True, labels=y)
        opt.zero_grad(set_to_none=True)
        head.loss.backward()
        opt.step()

    ms = {False: [], True: []}
    for c in (False, True):
        net.store.fusedCat_ = c
        for _ in range(20):
            step()
    for _ in range(blocks):
        for c in (False, True):
            net.store.fusedCat_ = c
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms[c].append((time.perf_counter() - t0) / steps * 1e3)
    print("(b) MCSeg training step (fused, fusedLinear, fusedLoss on; Adam), ms per step over %d alternating blocks of %d steps" % (
        blocks, steps))
    print("| fusedCat | best ms | worst ms |")
    print("|---|---|---|")
    for c in (False, True):
        print("| %s | %.3f | %.3f |" % ("on" if c else "off", min(ms[c]), max(ms[c])))
    print("best off / best on = %.3f; every on block below every off block: %s" % (
        min(ms[False]) / min(ms[True]), "yes (a gain)" if max(ms[True]) < min(ms[False]) else "no (no gain)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["a", "b", "both"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--bf16-rows", action="store_true", help="MCSeg(rows=torch.bfloat16): bf16 and mixed-type segments")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    numCats = 4
    net = MCSeg(1, args.batch, args.k, numCats, NUM_PARTS, dev, fused=True, fusedCat=False, fusedLinear=True, fusedLoss=True,
                rows=torch.bfloat16 if args.bf16_rows else None)
    P, Bi, F, N = synthetic_normals_batch(args.batch, args.points, rng, dev)
    batch = (P, Bi, F, (Bi % numCats).reshape(-1), part_labels(N))
    with torch.no_grad():
        net(*batch[:4], True)   # creates the variables
    levels = [int(p.shape[0]) for p in net.lastHierarchy.points_]
    print("MCSeg %d x %d points, k = %d%s: levels %s" % (args.batch, args.points, args.k, ", bf16 rows" if args.bf16_rows else "", levels))
    if args.part in ("a", "both"):
        part_a(levels, args.k, args.bf16_rows)
    if args.part in ("b", "both"):
        part_b(net, batch, steps=args.steps)


if __name__ == "__main__":
    main()
