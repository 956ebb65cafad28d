"""The pipelined training-loop step of a configuration's graph (mccnn_amd.workloads: cfg1 = MCClassS, 32 x 1024 points; cfg2 =
MCClassH, 32 x 4096 points) in three forms:
    edge          pdfMode='edge' on the native step executor -- the default, the yardstick
    point         pdfMode='point' op by op (pointNative=False)
    point-native  pdfMode='point' on the native step executor (pointNative=True)
ms per step and library launches per step. The loop is the deep form of tools/soak_network.py: the next batch's PointHierarchy
on its helper thread two batches ahead, prefetch_step(next hierarchy) right after reset(), host at most one step ahead.
    python tools/point_native_time.py [cfg1 cfg2] [--steps N]
Best of five blocks of N steps (default 200; wall clock around a device synchronisation), the worst in brackets."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from mccnn_amd import _lib  # noqa: E402
from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder  # noqa: E402
from mccnn_amd.workloads import CONFIGS, config_points  # noqa: E402

argv = sys.argv[1:]


def opt(name, dflt):
    if name in argv:
        v = int(argv[argv.index(name) + 1])
        del argv[argv.index(name):argv.index(name) + 2]
        return v
    return dflt


STEPS = opt("--steps", 200)
names = argv or ["cfg1", "cfg2"]
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
lib = _lib.load()
FORMS = (("edge", "edge", False), ("point", "point", False), ("point-native", "point", True))


def run(cfg, pdf_mode, point_native):
    torch.manual_seed(3)
    batches = []
    for k in range(3):   # three batches of the configuration's shape, other seeds
        p, b, B = config_points(cfg._replace(seed=cfg.seed + k))
        P, Bi = torch.from_numpy(p).to(dev), torch.from_numpy(b).to(dev)
        batches.append((P, Bi, B, torch.rand((len(p), 3), device=dev)))
    cb = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=cfg.relative, pdfMode=pdf_mode, pointNative=point_native)
    cb.hostStepsAhead_ = 1
    rows = {}

    def request(k):
        P, Bi, B, F0 = batches[k % 3]
        return PointHierarchy.prefetch(P, Bi, list(cfg.hierarchy), B, cfg.relative, after=True, features=F0)

    def adopt(k, pre):
        P, Bi, B, F0 = batches[k % 3]
        return PointHierarchy(P, F0, Bi, list(cfg.hierarchy), "PH", B, cfg.relative, prefetched=pre)

    def step(s, ph, then):
        cb.reset()
        then()
        outs = []
        for ci, c in enumerate(cfg.convs):
            key = (s % 3, ci)
            if key not in rows:
                n, m = int(ph.points_[c.lin].shape[0]), int(ph.points_[c.lout].shape[0])
                rows[key] = ((2 * torch.rand((n, c.fin), device=dev) - 1).requires_grad_(True),
                             2 * torch.rand((m, c.fout if c.combin else c.fin), device=dev) - 1)
            outs.append(cb.create_convolution(c.name, ph, c.lin, rows[key][0], c.fin, c.radius, ph, c.lout, c.combin, c.fout, c.window))
        torch.autograd.grad(outs, [rows[(s % 3, ci)][0] for ci in range(len(cfg.convs))] + list(cb.parameters()),
                            [rows[(s % 3, ci)][1] for ci in range(len(cfg.convs))], allow_unused=True)

    def block(s0, n):
        ready = adopt(s0, request(s0))
        ahead = request(s0 + 1)
        torch.cuda.synchronize()
        l0, t0 = lib.mccnn_debug_launch_count(), time.perf_counter()
        for s in range(s0, s0 + n):
            state = {}

            def start_next():
                state["nxt"] = adopt(s + 1, ahead)
                cb.prefetch_step(state["nxt"])
            step(s, ready, start_next)
            ready = state["nxt"]
            ahead = request(s + 2)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, (lib.mccnn_debug_launch_count() - l0) / float(n)

    block(0, 12)   # warm-up: variables, capacity guesses, the learned plan
    res = [block(12 + k * STEPS, STEPS) for k in range(5)]
    return min(r[0] for r in res), max(r[0] for r in res), res[-1][1], len(cb.cacheGeo_), len(cb.cachePointPDFs_)


for name in names:
    cfg = CONFIGS[name]
    for tag, pdf_mode, point_native in FORMS:
        best, worst, launches, geos, dens = run(cfg, pdf_mode, point_native)
        print("%s %-12s ms/step %.3f (worst of 5 blocks: %.3f)  launches/step %.1f  native geometries %d  densities %d"
              % (name, tag, best, worst, launches, geos, dens), flush=True)
