"""Voxel accuracy on the device (VariableStore(fusedLoss=True), dense_glue.voxel_counts, csrc/voxel_acc.hip) against the torch
code of the same definition (MCNetworkUtils._voxel_counts_torch) and against two host versions, measured in ONE process; the
fallback and the host versions are the yardsticks: python tools/voxel_acc_time.py [--part a|b|c|all] (on the GPU box).

Shapes, all with C = 21, labels by position with 20 % label 0 (ignored), predictions that hit 70 % of the rows:
  room     one 100 000-point room of workloads.make_room
  6 rooms  six of them as B = 6 (600 000 rows)
  32x1024  32 ellipsoid-and-box shapes of 1024 points (workloads.modelnet_like)
Per shape the occupied voxels, the workspace bytes and the probe steps the table's hash costs -- the mean distance of a key
from its home slot after all keys are in, simulated on the host with the kernel's hash (for linear probing that sum does not
depend on the order of arrival).

(a) One call through the helper into a given `out`, box given: fusedLoss off (torch code) against on (the op). HIP events,
    best of five runs of 50 calls after a warm-up, worst in brackets; library launches per call.
(b) Kernel-only C-ABI calls back to back: ws_clean = 1 (vote + score), ws_clean = 0 (clear + vote + score; the difference is
    the clear), and a call whose labels are all -1 on a clean table (the vote reads n labels and inserts nothing, the score
    pass loads cap empty keys: what the pass over the table costs on its own; vote + score less this is the vote's inserts
    and the occupied slots' scoring).
(c) The host: a vectorised NumPy version including the read-back of pred (wall clock, best of three), and the reference's
    loop restated (tests/voxel_acc_ref.reference_loop) on a 20 000-point room only -- it is quadratic.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mccnn_amd.MCNetworkUtils as U  # noqa: E402
from mccnn_amd import _lib, dense_glue, workloads  # noqa: E402

dev = torch.device("cuda", 0)
C = 21
RES = np.float32(0.05)


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


def _labels(pts, seed):
    rng = np.random.default_rng(seed)
    cell = np.floor(pts.astype(np.float64) / 0.4).astype(np.int64)
    lab = 1 + (cell[:, 0] + 3 * cell[:, 1] + 5 * cell[:, 2]) % (C - 1)
    lab[rng.random(len(lab)) < 0.2] = 0
    prd = np.where(rng.random(len(lab)) < 0.7, lab, rng.integers(0, C, len(lab)))
    return lab.astype(np.int32), prd.astype(np.int32)


def shapes():
    """-> [(name, points, pred, labels, batch ids or None, B, per-cloud minimum)]"""
    out = []
    room = workloads.make_room(100000, 1)
    out.append(("room", room, None, 1))
    rooms = np.concatenate([workloads.make_room(100000, 1 + k) for k in range(6)])
    out.append(("6 rooms", rooms, np.repeat(np.arange(6, dtype=np.int32), 100000), 6))
    pts, bids = workloads.modelnet_like(1024, 32, 3)
    out.append(("32x1024", pts, bids.reshape(-1), 32))
    res = []
    for name, pts, bid, B in out:
        lab, prd = _labels(pts, len(pts))
        mins = np.stack([pts[(bid == b) if bid is not None else slice(None)].min(0) for b in range(B)]).astype(np.float32)
        res.append((name, np.ascontiguousarray(pts, np.float32), prd, lab, bid, B, mins))
    return res


def host_keys(pts, bid, B, mins):
    b = np.zeros(len(pts), np.int64) if bid is None else bid.astype(np.int64)
    v = np.ceil((pts - mins[b]) / RES).astype(np.uint64)
    u = np.uint64
    return u(1 << 63) | (b.astype(u) << u(48)) | (v[:, 0] << u(32)) | (v[:, 1] << u(16)) | v[:, 2], b


def host_numpy(pts, pred_dev, lab, bid, B, mins, ignore=0, share=0.3):
    """The vectorised host version: read pred back, pack the keys, np.unique, two bincount histograms, the rule."""
    prd = pred_dev.cpu().numpy()
    keys, _ = host_keys(pts, bid, B, mins)
    uniq, inv = np.unique(keys, return_inverse=True)
    m = len(uniq)
    L = np.bincount(inv * C + lab, minlength=m * C).reshape(m, C)
    P = np.bincount(inv * C + prd, minlength=m * C).reshape(m, C)
    ul, up = L.argmax(1), P.argmax(1)
    valid = (L[:, ignore].astype(np.float64) / L.sum(1).astype(np.float64) < share) & (ul != ignore)
    cloud = ((uniq >> np.uint64(48)) & np.uint64(0x7fff)).astype(np.int64)
    cnt = np.zeros((B, C, 2), np.int64)
    np.add.at(cnt, (cloud[valid], ul[valid], 1), 1)
    hit = valid & (ul == up)
    np.add.at(cnt, (cloud[hit], ul[hit], 0), 1)
    return cnt


def probe_steps(uniq, cap):
    """Mean distance from the home slot over the occupied voxels: the kernel's hash and linear probing, on the host."""
    M = (1 << 64) - 1
    used = bytearray(cap)
    steps = 0
    for k in uniq.tolist():
        k ^= k >> 33
        k = (k * 0xff51afd7ed558ccd) & M
        k ^= k >> 33
        k = (k * 0xc4ceb9fe1a85ec53) & M
        k ^= k >> 33
        s = k & (cap - 1)
        while used[s]:
            s = (s + 1) & (cap - 1)
            steps += 1
        used[s] = 1
    return steps / float(len(uniq))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["a", "b", "c", "all"])
    args = ap.parse_args()
    lib = _lib.load()
    sh = _lib.stream_handle()
    rows = shapes()
    print("| shape | rows | B | occupied voxels | slots | workspace bytes | probe steps per voxel |")
    print("|---|---|---|---|---|---|---|")
    for name, pts, prd, lab, bid, B, mins in rows:
        uniq = np.unique(host_keys(pts, bid, B, mins)[0])
        cap = dense_glue.voxel_cap_rec(len(pts))
        print("| %s | %d | %d | %d | %d | %d | %.3f |" % (name, len(pts), B, len(uniq), cap, lib.mccnn_voxel_acc_workspace_bytes(len(pts), C),
                                                          probe_steps(uniq, cap)))
    for name, pts, prd, lab, bid, B, mins in rows:
        n = len(pts)
        P, p, l, b, mn = _dev(pts), _dev(prd), _dev(lab), _dev(bid), _dev(mins)
        out = torch.zeros((B, C, 2), dtype=torch.int64, device=dev)
        want = host_numpy(pts, p, lab, bid, B, mins)
        got = U.voxel_counts(P, p, l, C, b, B, mn, ignoreLabel=0, store=U.VariableStore(dev, fusedLoss=True))
        assert np.array_equal(got.cpu().numpy(), want), name
        print("%s: V %d of G %d valid voxels" % (name, int(want[:, :, 0].sum()), int(want[:, :, 1].sum())))
        if args.part in ("a", "all"):
            res = []
            for on in (False, True):
                st = U.VariableStore(dev, fusedLoss=on)
                res.append(best_of(lambda: U.voxel_counts(P, p, l, C, b, B, mn, ignoreLabel=0, out=out, store=st)))
            off, on = res
            print("(a) %s helper us per call: torch %.1f [%.1f] | op %.1f [%.1f] | torch / op %.1f | launches %.1f" % (
                name, off[0], off[1], on[0], on[1], off[0] / on[0], on[2]))
        if args.part in ("b", "all"):
            ws = torch.zeros(lib.mccnn_voxel_acc_workspace_bytes(n, C), dtype=torch.uint8, device=dev)
            dead = torch.full_like(l, -1)

            def call(labels, clean):
                _lib.check(lib.mccnn_voxel_acc_add(P.data_ptr(), p.data_ptr(), labels.data_ptr(), _lib.ptr(b), mn.data_ptr(), n, B, C, 0,
                                                   float(RES), 0.3, out.data_ptr(), None, ws.data_ptr(), ws.numel(), clean, sh), "voxel_acc_add")

            two, three, empty = best_of(lambda: call(l, 1)), best_of(lambda: call(l, 0)), best_of(lambda: call(dead, 1))
            print("(b) %s C-ABI us per call: vote + score %.1f [%.1f] | with the clear %.1f [%.1f] (clear %.1f) | all rows dead "
                  "(the pass over %d empty slots) %.1f [%.1f] | launches %.0f / %.0f" % (
                      name, two[0], two[1], three[0], three[1], three[0] - two[0], ws.numel() // (8 + 8 * C), empty[0], empty[1],
                      two[2], three[2]))
        if args.part in ("c", "all"):
            times = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_numpy(pts, p, lab, bid, B, mins)
                times.append((time.perf_counter() - t0) * 1e6)
            print("(c) %s vectorised NumPy on the host with the read-back of pred: %.0f us [%.0f]" % (name, min(times), max(times)))
    if args.part in ("c", "all"):
        import voxel_acc_ref as ref
        d, want, _ = ref.case("room")
        t0 = time.perf_counter()
        V, G, _, _ = ref.reference_loop(d["points"], d["pred"], d["labels"], d["C"], d["res"])
        t1 = time.perf_counter()
        assert np.array_equal(want[0, :, 1], G.astype(np.int64))
        t = {k: _dev(d[k]) for k in ("points", "pred", "labels", "mn")}
        out = torch.zeros((1, C, 2), dtype=torch.int64, device=dev)
        st = U.VariableStore(dev, fusedLoss=True)
        on = best_of(lambda: U.voxel_counts(t["points"], t["pred"], t["labels"], C, None, 1, t["mn"], ignoreLabel=0, out=out, store=st))
        print("(c) 20 000-point room: the reference's loop restated %.0f us (once) | the op through the helper %.1f [%.1f] us" % (
            (t1 - t0) * 1e6, on[0], on[1]))


if __name__ == "__main__":
    main()
