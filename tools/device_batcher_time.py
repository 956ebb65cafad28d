#!/usr/bin/env python3
"""Time of one training batch: DeviceBatcher (mccnn_amd/device_batcher.py, built on the GPU) beside RaggedBatcher.get_next_batch
+ to_device (host NumPy, then the upload) over the same synthetic models, per sampling protocol and mixed.

    python tools/device_batcher_time.py [--runs 5] [--batches 50] [--host-batches 8] [--json out.json]

Shapes: 32 x 1024 and 32 x 4096 points out of 64 models of 10 000 points; one 100 000-point cloud with numPoints = 0
(ptDropOut 0.8: the uniform protocol keeps 80 000 points). Models carry normals, augment = True.
Columns, ms per batch:
  device   HIP events around `batches` calls of get_next_batch(check=False) on one stream, best of `runs` (worst beside
           it) after a warm-up run. The events span the host's planning as well: where the host is slower than the GPU
           this is the host's pace.
  plan     wall time of plan_batch alone (the host's whole contribution to a batch)
  kernel   HIP events around `batches` launches of one fixed plan (no planning): the device's own time
  host     RaggedBatcher.get_next_batch + to_device, wall time, median over `host-batches` batches
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd.batcher import RaggedBatcher
from mccnn_amd.device_batcher import DeviceBatcher, sample_plan


def make_models(count, n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        d = rs.randn(n, 3)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append({"pts": d * np.array([1.0, 0.6, 0.4]) + 0.01 * rs.randn(n, 3), "normals": d})
    return out


def next_batch(b, **kw):
    if not b.has_more_batches():
        b.start_iteration()
    return b.get_next_batch(**kw)


def time_device(db, runs, batches):
    ev = lambda: torch.cuda.Event(enable_timing=True)
    res = []
    for r in range(runs + 1):   # (run 0 is the warm-up)
        a, b = ev(), ev()
        torch.cuda.synchronize()
        a.record()
        for _ in range(batches):
            next_batch(db, check=False)
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) / batches)
    return min(res[1:]), max(res[1:])


def time_plan(db, batches):
    t = []
    for _ in range(batches):
        if not db.has_more_batches():
            db.start_iteration()
        t0 = time.perf_counter()
        db.plan_batch()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def time_kernel(db, runs, batches):
    if not db.has_more_batches():
        db.start_iteration()
    plan = db.plan_batch()
    res = []
    for r in range(runs + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(batches):
            sample_plan(db.store_, plan["slots"], plan["out_rows"])
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) / batches)
    return min(res[1:]), max(res[1:])


def time_host(rb, batches):
    t = []
    for _ in range(batches):
        if not rb.has_more_batches():
            rb.start_iteration()
        t0 = time.perf_counter()
        out = rb.to_device(rb.get_next_batch())
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
        del out
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--host-batches", type=int, default=8)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    small = make_models(64, 10000, 1)
    big = make_models(2, 100000, 2)
    shapes = [("32 x 1024", small, dict(numPoints=1024, ptDropOut=0.8, batchSize=32)),
              ("32 x 4096", small, dict(numPoints=4096, ptDropOut=0.8, batchSize=32)),
              ("1 x 100k, numPoints=0", big, dict(numPoints=0, ptDropOut=0.8, batchSize=1))]
    protos = [("uniform", [0]), ("split", [1]), ("gradient", [2]), ("lambert", [3]), ("occlusion", [4]), ("all five", [0, 1, 2, 3, 4])]
    rows = []
    print("%-24s %-10s %9s %9s %8s %9s %9s %9s %7s" % ("shape", "protocol", "device", "(worst)", "plan", "kernel", "(worst)", "host", "ratio"))
    for name, models, kw in shapes:
        for pname, allowed in protos:
            common = dict(allowedSamplings=allowed, augment=True, seed=5, **kw)
            db = DeviceBatcher(models, **common)
            best, worst = time_device(db, args.runs, args.batches)
            plan = time_plan(db, args.batches)
            kb, kw_ = time_kernel(db, args.runs, args.batches)
            host = time_host(RaggedBatcher(models, **common), args.host_batches)
            row = dict(shape=name, protocol=pname, device_ms=best, device_worst_ms=worst, plan_ms=plan, kernel_ms=kb, kernel_worst_ms=kw_,
                       host_ms=host, ratio=host / best)
            rows.append(row)
            print("%-24s %-10s %9.3f %9.3f %8.3f %9.3f %9.3f %9.2f %7.1f" % (name, pname, best, worst, plan, kb, kw_, host, host / best), flush=True)
            del db
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
