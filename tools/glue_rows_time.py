"""The dense glue on bf16 rows (mccnn_bn_act_fwd_rows / _bwd_rows) against the float32 op in ONE process, the method of
tools/glue_time.py: HIP events, best of five runs of 50 calls after a warm-up, worst in brackets.
    python tools/glue_rows_time.py [--part a|b|both]      (on the GPU box)

(a) Kernel-only: back-to-back C-ABI calls, forward and backward separately, per shape and type combination; f32/f32 goes
    through the float32 entries. GB/s of algorithmic bytes: forward n c (2 s_x + s_y), backward n c (2 s_x + 2 s_dy + s_dx)
    (12 n c and 20 n c for f32). The line under the table names every combination that is slower than f32/f32 by more than
    the spread of the five runs of either.
(b) Through the helpers, forward + backward of one glue block on bf16 rows: the fused op bf16 -> bf16, the torch fallback
    on bf16 rows, and the float32 fused op with explicit casts around it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mccnn_amd.MCNetworkUtils as U  # noqa: E402
from mccnn_amd import _lib  # noqa: E402
from mccnn_amd.MCConvModule import _ws  # noqa: E402

dev = torch.device("cuda", 0)
SHAPES = [(3517, 32), (100000, 64), (131072, 32), (131072, 128)]
LARGE = SHAPES[1:]
COMBOS = [(0, 0, "f32/f32"), (0, 1, "f32->bf16"), (1, 0, "bf16->f32"), (1, 1, "bf16/bf16")]
T_ALL = 1 << 32


def timed(call, calls=50, runs=5):
    """-> (best us, worst us) per call."""
    for _ in range(10):
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


def kernel_times(n, c, xb, yb):
    """-> ((fwd best, worst), (bwd best, worst)) us of the C-ABI calls alone."""
    lib = _lib.load()
    bf = torch.bfloat16
    x = (torch.randn(n, c, device=dev) * 2 + 3).to(bf if xb else torch.float32)
    dy = torch.randn(n, c, device=dev).to(bf if yb else torch.float32)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    g, b, mm, mv = (torch.ones(c, device=dev), torch.zeros(c, device=dev), torch.zeros(c, device=dev), torch.ones(c, device=dev))
    saved, dgb = torch.empty((2, c), device=dev), torch.empty((2, c), device=dev)
    ws = _ws(lib.mccnn_bn_act_workspace_bytes(n, c), dev)
    st = _lib.stream_handle()
    p = lambda t: t.data_ptr()   # noqa: E731
    if not xb and not yb:
        fwd = lambda: lib.mccnn_bn_act_fwd(p(x), n, c, p(g), p(b), p(mm), p(mv), 0.99, 1e-3, 1, 1, T_ALL, 1.0, 0, p(y), p(saved),   # noqa: E731
                                           p(ws), ws.numel(), st)
        bwd = lambda: lib.mccnn_bn_act_bwd(p(x), p(dy), n, c, p(g), p(b), p(saved), 1, T_ALL, 1.0, 0, p(dx), p(dgb[0]), p(dgb[1]),   # noqa: E731
                                           p(ws), ws.numel(), st)
    else:
        fwd = lambda: lib.mccnn_bn_act_fwd_rows(p(x), xb, n, c, p(g), p(b), p(mm), p(mv), 0.99, 1e-3, 1, 1, T_ALL, 1.0, 0, p(y), yb,   # noqa: E731
                                                p(saved), p(ws), ws.numel(), st)
        bwd = lambda: lib.mccnn_bn_act_bwd_rows(p(x), xb, p(dy), yb, n, c, p(g), p(b), p(saved), 1, T_ALL, 1.0, 0, p(dx), p(dgb[0]),   # noqa: E731
                                                p(dgb[1]), p(ws), ws.numel(), st)
    assert fwd() == 0 and bwd() == 0
    return timed(fwd), timed(bwd)


def part_a():
    print("(a) kernel-only, C-ABI calls back to back, us per call: best of 5 runs of 50 calls [worst]; GB/s of algorithmic bytes")
    print("| n | c | types | fwd us | fwd GB/s | bwd us | bwd GB/s |")
    print("|---|---|---|---|---|---|---|")
    slower = []
    for n, c in SHAPES:
        base = None
        for xb, yb, name in COMBOS:
            f, w = kernel_times(n, c, xb, yb)
            sx, sy = 2 if xb else 4, 2 if yb else 4
            fb, wb = n * c * (2 * sx + sy), n * c * (2 * sx + 2 * sy + sx)
            print("| %d | %d | %s | %.1f [%.1f] | %.0f | %.1f [%.1f] | %.0f |" % (
                n, c, name, f[0], f[1], fb / (f[0] * 1e-6) / 1e9, w[0], w[1], wb / (w[0] * 1e-6) / 1e9))
            if base is None:
                base = (f, w)
            elif (n, c) in LARGE:
                for tag, t, t0 in (("fwd", f, base[0]), ("bwd", w, base[1])):
                    if t[0] - t0[0] > max(t[1] - t[0], t0[1] - t0[0]):
                        slower.append("%dx%d %s %s: %.1f against %.1f us" % (n, c, name, tag, t[0], t0[0]))
    print("slower than f32/f32 by more than the spread of either, large shapes: %s" % ("; ".join(slower) if slower else "none"))


def helper_time(n, c, form):
    """Forward + backward of one block on bf16 rows in, bf16 rows out -> (best us, worst us, library launches per call)."""
    lib = _lib.load()
    bf = torch.bfloat16
    st = U.VariableStore(dev, fused=form != "torch")
    x = (torch.randn(n, c, device=dev) * 2 + 3).to(bf).requires_grad_(True)
    dy = torch.randn(n, c, device=dev).to(bf)

    def call():
        if form != "f32 fused + casts":      # (the store's switch tells the fused op from the torch code)
            y = U.batch_norm_RELU_drop_out("T", x, True, False, None, st)
        else:
            y = U.batch_norm_RELU_drop_out("T", x.float(), True, False, None, st).to(bf)
        x.grad = None
        y.backward(dy)

    call()
    torch.cuda.synchronize()
    before = lib.mccnn_debug_launch_count()
    t = timed(call)
    return t[0], t[1], (lib.mccnn_debug_launch_count() - before) / 260.0


def part_b():
    print("(b) one glue block on bf16 rows through the helpers, forward + backward, us per call: best of 5 runs of 50 calls [worst]")
    print("| n | c | fused bf16/bf16 us | torch fallback us | f32 fused + casts us | torch / fused | casts / fused | fused launches |")
    print("|---|---|---|---|---|---|---|---|")
    for n, c in SHAPES:
        f = helper_time(n, c, "fused bf16/bf16")
        t = helper_time(n, c, "torch")
        k = helper_time(n, c, "f32 fused + casts")
        assert t[2] == 0.0, "the torch path launched library kernels"
        print("| %d | %d | %.1f [%.1f] | %.1f [%.1f] | %.1f [%.1f] | %.2f | %.2f | %.1f |" % (
            n, c, f[0], f[1], t[0], t[1], k[0], k[1], t[0] / f[0], k[0] / f[0], f[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["a", "b", "both"])
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.part in ("a", "both"):
        part_a()
    if args.part in ("b", "both"):
        part_b()


if __name__ == "__main__":
    main()
