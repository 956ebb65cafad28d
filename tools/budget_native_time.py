"""The pipelined training-loop step of a configuration's graph (mccnn_amd.workloads: cfg1 = MCClassS, 32 x 1024 points; cfg3 =
MCSeg, 16 x 8192) with an edge budget on every layer: ms per step and library launches per step
    1. budget op by op            ConvolutionBuilder(maxEdges=B)                      -- the yardstick
    2. budget, native executor    ConvolutionBuilder(maxEdges=B, budgetNative=True)
    3. for orientation            ConvolutionBuilder(maxNeighbors=K, capNative=True), K = the cap most lists chose under B
B is half the uncapped edge total of the graph's longest list (printed with every list's total and the caps chosen). The loop
is the one of tools/cap_native_time.py: the next batch's PointHierarchy on its helper thread two batches ahead,
prefetch_step(next hierarchy) right after reset(), host at most one step ahead.
    python tools/budget_native_time.py [cfg1 cfg3] [--steps N]
The three forms are timed in ONE process, block by block in turn: five blocks of N steps each (wall clock around a device
synchronisation), the best and the worst block of every form reported."""
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
names = argv or ["cfg1", "cfg3"]
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
lib = _lib.load()


class Loop:
    """One builder and its pipelined loop over three batches of the configuration's shape."""

    def __init__(self, cfg, **builder_args):
        torch.manual_seed(3)
        self.cfg = cfg
        self.batches = []
        for k in range(3):
            p, b, B = config_points(cfg._replace(seed=cfg.seed + k))
            P, Bi = torch.from_numpy(p).to(dev), torch.from_numpy(b).to(dev)
            self.batches.append((P, Bi, B, torch.rand((len(p), 3), device=dev)))
        self.cb = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=cfg.relative, **builder_args)
        self.cb.hostStepsAhead_ = 1
        self.rows = {}
        self.next = 0

    def request(self, k):
        P, Bi, B, F0 = self.batches[k % 3]
        return PointHierarchy.prefetch(P, Bi, list(self.cfg.hierarchy), B, self.cfg.relative, after=True, features=F0)

    def adopt(self, k, pre):
        P, Bi, B, F0 = self.batches[k % 3]
        return PointHierarchy(P, F0, Bi, list(self.cfg.hierarchy), "PH", B, self.cfg.relative, prefetched=pre)

    def step(self, s, ph, then):
        cfg, cb, rows = self.cfg, self.cb, self.rows
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

    def block(self, n):
        """n pipelined steps -> (ms per step, launches per step)"""
        s0 = self.next
        self.next += n
        ready = self.adopt(s0, self.request(s0))
        ahead = self.request(s0 + 1)
        torch.cuda.synchronize()
        l0, t0 = lib.mccnn_debug_launch_count(), time.perf_counter()
        for s in range(s0, s0 + n):
            state = {}

            def start_next():
                state["nxt"] = self.adopt(s + 1, ahead)
                self.cb.prefetch_step(state["nxt"])
            self.step(s, ready, start_next)
            ready = state["nxt"]
            ahead = self.request(s + 2)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, (lib.mccnn_debug_launch_count() - l0) / float(n)


def cap_of(v):
    return int((v.value() if hasattr(v, "value") else v)[0])


for name in names:
    cfg = CONFIGS[name]
    # the uncapped edge totals of the graph's lists (first batch), from one uncapped step on the native executor
    plain = Loop(cfg)
    plain.block(2)
    totals = sorted(geo.edges() for geo in plain.cb.cacheGeo_.values())
    budget = max(1, totals[-1] // 2)
    del plain
    print("%s: uncapped edge totals of its %d lists %s -> maxEdges = %d" % (name, len(totals), totals, budget), flush=True)
    native = Loop(cfg, maxEdges=budget, budgetNative=True)
    native.block(12)   # warm-up: variables, capacity guesses, the learned plan
    caps = sorted(cap_of(v) for v in native.cb.chosenCaps_.values())
    common = max(set(caps), key=caps.count)
    print("%s: caps chosen under that budget %s -> maxNeighbors = %d for the capped form" % (name, caps, common), flush=True)
    forms = [("budget op by op", Loop(cfg, maxEdges=budget)), ("budget native", native),
             ("capNative K=%d" % common, Loop(cfg, maxNeighbors=common, capNative=True))]
    for label, loop in forms:
        if loop is not native:
            loop.block(12)
    res = {label: [] for label, _ in forms}
    for _k in range(5):
        for label, loop in forms:
            res[label].append(loop.block(STEPS))
    for label, loop in forms:
        r = res[label]
        print("%s %-16s ms/step %.3f (worst of 5 blocks of %d steps: %.3f)  launches/step %.1f  native geometries %d"
              % (name, label, min(x[0] for x in r), STEPS, max(x[0] for x in r), r[-1][1], len(loop.cb.cacheGeo_)), flush=True)
