"""Segmentation counts on the device (VariableStore(fusedLoss=True), dense_glue.segmentation_counts, csrc/seg_counts.hip)
against the torch code of the same definition (MCNetworkUtils._seg_counts_torch: the live rule, four flat indices per row and
one integer scatter_add_), measured in ONE process; the torch path is the yardstick:
python tools/seg_counts_time.py [--part a|b|all] (on the GPU box).

Shapes (n rows, B clouds, C classes): (32768, 32, 50) and (131072, 16, 50) ShapeNet-style batches with contiguous clouds,
(100000, 1, 21) a ScanNet room with label 0 ignored and row weights, (131072, 64, 400) the shape without an LDS table.

(a) One call through the helper (MCNetworkUtils.segmentation_counts into a given `out`), fusedLoss off against on. HIP
    events, best of five runs of 50 calls after a warm-up, worst in brackets; library launches per call.
(b) Kernel-only C-ABI calls back to back with GB/s of the algorithmic bytes (8 n for pred and labels, 4 n more each for batch
    ids and weights), beside the torch code on the same buffers; and the LDS route beside the route without a table at the
    same n.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mccnn_amd.MCNetworkUtils as U  # noqa: E402
from mccnn_amd import _lib  # noqa: E402

dev = torch.device("cuda", 0)
#        n,      B,  C,  ignore, weights
SHAPES = [(32768, 32, 50, -1, False), (131072, 16, 50, -1, False), (100000, 1, 21, 0, True), (131072, 64, 400, -1, False)]


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


def _rows(n, B, C, weighted):
    """Labels in [0, C), predictions that hit half the rows, contiguous clouds of equal size (None for B = 1), weights with a
    tenth of zeros."""
    rng = np.random.default_rng(n + B + C)
    labels = rng.integers(0, C, n).astype(np.int32)
    pred = np.where(rng.random(n) < 0.5, labels, rng.integers(0, C, n)).astype(np.int32)
    bid = None if B == 1 else (np.arange(n, dtype=np.int64) * B // n).astype(np.int32)
    rw = (rng.random(n) > 0.1).astype(np.float32) if weighted else None
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    return t(pred), t(labels), t(bid), t(rw)


def _bytes(n, bid, rw):
    return 8.0 * n + (4.0 * n if bid is not None else 0.0) + (4.0 * n if rw is not None else 0.0)


def part_a():
    print("(a) one call through the helper into a given out, us per call: best of 5 runs of 50 calls [worst]")
    print("| n | B | C | route | fusedLoss off (torch) us | on (op) us | off / on | launches on |")
    print("|---|---|---|---|---|---|---|---|")
    lib = _lib.load()
    for n, B, C, ignore, weighted in SHAPES:
        pred, labels, bid, rw = _rows(n, B, C, weighted)
        out = torch.zeros((B, C, 3), dtype=torch.int64, device=dev)
        res = []
        for on in (False, True):
            st = U.VariableStore(dev, fusedLoss=on)
            res.append(best_of(lambda: U.segmentation_counts(pred, labels, C, bid, B, rw, ignore, out=out, store=st)))
        off, on = res
        print("| %d | %d | %d | %s | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f |" % (
            n, B, C, "LDS table" if lib.mccnn_seg_counts_lds_bytes(B, C) else "no table", off[0], off[1], on[0], on[1],
            off[0] / on[0], on[2]))


def part_b():
    lib = _lib.load()
    print("(b) kernel-only C-ABI calls back to back, us per call: best of 5 runs of 50 calls [worst]; GB/s of the algorithmic "
          "bytes at the op's best; the torch code of the helper on the same buffers beside it")
    print("| n | B | C | route | torch us | op us | torch / op | op GB/s |")
    print("|---|---|---|---|---|---|---|---|")
    sh = _lib.stream_handle()
    for n, B, C, ignore, weighted in SHAPES + [(131072, 16, 50, -1, True), (131072, 1, 2, -1, False)]:
        pred, labels, bid, rw = _rows(n, B, C, weighted)
        out = torch.zeros((B, C, 3), dtype=torch.int64, device=dev)

        def op():
            _lib.check(lib.mccnn_seg_counts_add(pred.data_ptr(), labels.data_ptr(), _lib.ptr(rw), _lib.ptr(bid), n, B, C, ignore,
                                                out.data_ptr(), sh), "seg_counts_add")

        ref = best_of(lambda: U._seg_counts_torch(pred, labels, C, bid, B, rw, ignore, out))
        got = best_of(op)
        print("| %d | %d | %d | %s%s | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.1f |" % (
            n, B, C, "LDS table" if lib.mccnn_seg_counts_lds_bytes(B, C) else "no table", ", weights" if weighted else "",
            ref[0], ref[1], got[0], got[1], ref[0] / got[0], _bytes(n, bid, rw) / got[0] * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["a", "b", "all"])
    args = ap.parse_args()
    if args.part in ("a", "all"):
        part_a()
    if args.part in ("b", "all"):
        part_b()


if __name__ == "__main__":
    main()
