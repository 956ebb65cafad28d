"""The device batcher without a GPU: its NumPy float32 restatement (tests/device_batcher_ref.py, which the kernel is held to
bit for bit in tests/test_gpu_device_batcher.py) against the host loader the reference itself pins (mccnn_amd.sampling,
mccnn_amd.batcher.RaggedBatcher), the host bookkeeping of DeviceBatcher against RaggedBatcher's, the C surface, and the
stand-alone host checker of the draws (tools/batch_sample_check.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mccnn_amd import sampling
from mccnn_amd.batcher import RaggedBatcher
from mccnn_amd.device_batcher import DeviceBatcher, new_slots, SLOT_DTYPE
from tests import device_batcher_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slot(pts, protocol, view=None, rows=0, exact=0, seed=1):
    s = new_slots(1)[0]
    p = np.asarray(pts, np.float32)
    s["length"], s["n_sel"], s["protocol"], s["rows"], s["exact"], s["seed"] = len(p), len(p), protocol, rows, exact, seed
    s["bmin"], s["bmax"] = p.min(axis=0), p.max(axis=0)
    if view is not None:
        s["view"] = view
    return s


def _host_probabilities(monkeypatch, fn, *args):
    """The f64 probabilities a sampling.py protocol hands to its accept loop."""
    seen = {}

    def grab(prob, num_points, rs):
        seen["prob"] = np.array(prob, np.float64)
        return np.zeros(0, np.int64)
    monkeypatch.setattr(sampling, "_collect", grab)
    fn(np.random.RandomState(0), *args)
    return seen["prob"]


def _box_cloud(seed, n=10000):
    """f32 points uniform in a 2.0 x 1.0 x 0.5 box away from the origin (the same numbers feed the f64 functions)."""
    rs = np.random.RandomState(seed)
    return (rs.rand(n, 3) * np.array([2.0, 1.0, 0.5]) + np.array([-0.3, 0.2, 1.0])).astype(np.float32)


def test_split_and_gradient_probabilities_match_the_f64_loader(monkeypatch):
    pts = _box_cloud(11)
    p64 = pts.astype(np.float64)
    cmin, size, ax = sampling._bbox(p64)
    pos = (p64[:, ax] - cmin[ax]) / size[ax]
    assert not np.any(np.abs(pos - 0.5) <= 1e-6), "an input point sits on split's threshold"
    for proto, fn in ((1, sampling.sample_split), (2, sampling.sample_gradient)):
        want = _host_probabilities(monkeypatch, fn, p64)
        got = ref.probabilities(_slot(pts, proto), pts, None)
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want).max()
        print("protocol", proto, "max |prob f32 - prob f64|", err)
        assert err <= 1e-6


def test_lambert_probabilities_match_the_f64_loader(monkeypatch):
    """sqrt has an unbounded slope at 0: an f32 dot product that is off by e (|e| <= 3 * 2^-24 < 1.8e-7 for unit vectors)
    moves sqrt(d) by e / (2 sqrt(d)), which stays below 1e-6 only for d >= 8.1e-3 (or where both sides clip to 0). The
    inputs therefore hold no normal with -1e-6 < view . n < 1e-2, and the test asserts there is none."""
    rs = np.random.RandomState(12)
    view = sampling.random_view(rs).astype(np.float32)
    nr = rs.randn(40000, 3)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    d = nr.astype(np.float64) @ view.astype(np.float64)
    nr = nr[~((d > -1e-6) & (d < 1e-2))][:10000]
    d = nr.astype(np.float64) @ view.astype(np.float64)
    assert len(nr) == 10000 and not np.any((d > -1e-6) & (d < 1e-2))
    assert (d < 0).sum() > 3000 and (d > 0.5).sum() > 1000
    pts = _box_cloud(13)
    want = _host_probabilities(monkeypatch, sampling.sample_lambert, view.astype(np.float64), pts.astype(np.float64), nr.astype(np.float64))
    got = ref.probabilities(_slot(pts, 3, view), pts, nr)
    err = np.abs(got.astype(np.float64) - want).max()
    print("lambert max |prob f32 - prob f64|", err)
    assert err <= 1e-6


_ELLIPSOIDS = {}


def _ellipsoid(n):
    """randn directions scaled by (1.0, 0.6, 0.4), the unscaled direction as normal, 0.01 randn noise on the points; all
    sizes and their three views each from one RandomState(3). Computed once, never modified."""
    if not _ELLIPSOIDS:
        rs = np.random.RandomState(3)
        for m in (300, 2500, 10000, 100000):
            d = rs.randn(m, 3)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            pts = d * np.array([1.0, 0.6, 0.4]) + 0.01 * rs.randn(m, 3)
            views = [sampling.random_view(rs) for _ in range(3)]
            _ELLIPSOIDS[m] = (pts.astype(np.float32), d.astype(np.float32), [v.astype(np.float32) for v in views])
    return _ELLIPSOIDS[n]


@pytest.mark.parametrize("n", [300, 2500, 10000, 100000])
def test_occlusion_keep_mask_matches_the_f64_loader(monkeypatch, n):
    pts, nr, views = _ellipsoid(n)
    for view in views:
        seen = {}

        def grab(mask, num_points):
            seen["mask"] = np.array(mask)
            return np.zeros(0, np.int64)
        monkeypatch.setattr(sampling, "_cycle", grab)
        sampling.sample_occlusion(view.astype(np.float64), pts.astype(np.float64), nr.astype(np.float64), num_points=0)
        got = ref.occlusion_keep(_slot(pts, 4, view), pts, nr)
        diff = int((got != seen["mask"]).sum())
        print("n", n, "kept", int(seen["mask"].sum()), "differing", diff)
        assert seen["mask"].sum() > 0
        assert diff <= n // 1000


def test_split_accept_share():
    pts = _box_cloud(21)
    s = _slot(pts, 1, rows=len(pts), exact=0, seed=77)
    idx, st = ref.select(s, pts, None)
    assert st == ref.OK and np.all(np.diff(idx) > 0)
    ax, size, lo = ref._axis(s)
    upper = (pts[:, ax] - lo) / size > np.float32(0.5)
    acc = np.zeros(len(pts), bool)
    acc[idx] = True
    assert acc[upper].all()
    share = acc[~upper].mean()
    n_low = int((~upper).sum())
    print("lower half: %d points, accepted share %.4f" % (n_low, share))
    assert 4700 <= n_low <= 5300
    assert abs(share - 0.25) <= 0.025   # 4 sigma, sigma = sqrt(0.25 * 0.75 / 5000)


@pytest.mark.parametrize("n,K", [(10000, 1024), (1024, 1024), (1025, 1024), (2049, 1023), (7, 3)])
def test_uniform_is_one_index_per_stratum(n, K):
    for seed in (0, 5, 2 ** 32 - 1):
        idx = ref.uniform_indices(n, K, seed)
        t = np.arange(K)
        lo, hi = t * n // K, (t + 1) * n // K
        assert len(idx) == K and np.all(np.diff(idx) > 0)
        assert np.all(idx >= lo) and np.all(idx < hi) and np.all((hi - lo >= n // K) & (hi - lo <= -(-n // K)))
    if n > 4 * K:
        assert len(set(tuple(ref.uniform_indices(n, K, s)) for s in range(4))) == 4   # the seed matters


def test_uniform_with_fewer_points_than_rows_and_select_first():
    idx = ref.uniform_indices(50, 1024, 9)
    assert len(idx) == 1024 and idx.min() >= 0 and idx.max() < 50 and len(np.unique(idx)) > 40
    models = [{"pts": np.random.RandomState(k).rand(5000, 3)} for k in range(3)]
    db = DeviceBatcher(models, 1024, 0.9, 3, [0], uniformSelectFirst=True, seed=4, device="cpu")
    db.start_iteration()
    plan = db.plan_batch()
    cut = int(1024 * (2.0 - 0.9))
    assert list(plan["slots"]["n_sel"]) == [cut] * 3 and list(plan["slots"]["rows"]) == [1024] * 3
    for s in plan["slots"]:
        idx, st = ref.select(s, models[0]["pts"], None)
        assert st == ref.OK and len(idx) == 1024 and idx.max() < cut and np.all(np.diff(idx) > 0)
    # numPoints == 0: K = int(n * ptDropOut), known on the host
    db0 = DeviceBatcher(models, 0, 0.9, 3, [0], seed=4, device="cpu")
    db0.start_iteration()
    p0 = db0.plan_batch()
    assert list(p0["slots"]["rows"]) == [4500] * 3 and list(p0["slots"]["out_base"]) == [0, 4500, 9000] and not p0["exact"]


def _ellipsoid_models(count, seed):
    rs = np.random.RandomState(seed)
    models, cats = [], []
    for k in range(count):
        m = int(rs.randint(300, 900))
        d = rs.randn(m, 3)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts = d * np.array([1.0, 0.6, 0.4]) + 0.01 * rs.randn(m, 3)
        # f32-representable values, so that the f64 host loader and the f32 store see the same numbers
        models.append({"pts": pts.astype(np.float32).astype(np.float64), "normals": d.astype(np.float32).astype(np.float64)})
        cats.append(int(rs.randint(0, 5)))
    return models, cats


@pytest.mark.parametrize("maxPts", [0, 1500])
def test_host_bookkeeping_matches_ragged_batcher(maxPts):
    """Occlusion-only slots consume the main RandomState exactly as RaggedBatcher does (protocol choice, view, rotation), so
    a whole iteration stays in step: ids, numModelInBatch, slot indices, categories and -- through the restatement -- the
    rows of every slot. 10 models in batches of 4: the iteration ends in a part-filled batch; maxPtsxBatch = 1500 leaves
    slots empty in the middle of the iteration."""
    models, cats = _ellipsoid_models(10, 5)
    kw = dict(numPoints=0, ptDropOut=1.0, batchSize=4, allowedSamplings=[4], categories=cats, maxPtsxBatch=maxPts, augment=True, seed=7)
    rb = RaggedBatcher(models, **kw)
    db = DeviceBatcher(models, device="cpu", **kw)
    assert db.get_num_models() == rb.get_num_models() == 10
    rb.start_iteration()
    db.start_iteration()
    store_pts = np.concatenate([m["pts"] for m in models]).astype(np.float32)
    store_nr = np.concatenate([m["normals"] for m in models]).astype(np.float32)
    batches, short = 0, 0
    while rb.has_more_batches():
        assert db.has_more_batches()
        num, pts, bids, feats, labels, cat, ids = rb.get_next_batch()
        plan = db.plan_batch()
        assert plan["numModelInBatch"] == num and plan["ids"] == [int(i) for i in ids]
        assert list(plan["categories"]) == [int(c) for c in cat]
        slot_ids, rows = np.unique(bids[:, 0], return_counts=True)
        assert list(plan["slots"]["batch_id"]) == [int(b) for b in slot_ids]
        r = ref.run_plan(plan["slots"], store_pts, store_nr, plan["out_rows"])
        assert list(r["counts"]) == [int(c) for c in rows]
        assert np.all(r["status"] == ref.OK)
        # (the rotation is the host batcher's as well: the kept points are the same, so are their rotated coordinates)
        got = np.concatenate([r["pts"][b:b + c] for b, c in zip(plan["slots"]["out_base"], r["counts"])])
        assert np.abs(got - pts).max() < 1e-5
        batches += 1
        short += num < 4
    assert not db.has_more_batches()
    assert short >= 1 and batches >= (4 if maxPts else 3)


def test_plan_with_fixed_rows_and_trailing_empty_slots():
    models, cats = _ellipsoid_models(5, 6)
    db = DeviceBatcher(models, 256, 1.0, 4, [0, 1, 2, 3, 4], categories=cats, augment=True, augmentSmallRotations=True, seed=3, device="cpu")
    db.start_iteration()
    p1, p2 = db.plan_batch(), db.plan_batch()
    assert p1["numModelInBatch"] == 4 and p2["numModelInBatch"] == 1 and p2["out_rows"] == 256 and p1["exact"]
    assert list(p1["slots"]["out_base"]) == [0, 256, 512, 768] and p1["slots"].dtype == SLOT_DTYPE
    for s in p1["slots"]:
        R = s["rot"].astype(np.float64).reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6
        assert (np.abs(s["view"]).sum() > 0) == (s["protocol"] >= 3)
    assert len(set(p1["slots"]["seed"])) == 4
    with pytest.raises(RuntimeError):
        DeviceBatcher([{"pts": np.zeros((4, 3))}], 16, 1.0, 1, [3], device="cpu")   # lambert needs normals


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(mccnn_[a-z0-9_]+)\s*\(", txt))


def test_c_surface():
    import ctypes
    from mccnn_amd import build, _lib
    names = {"mccnn_batch_sample", "mccnn_batch_sample_chunk", "mccnn_batch_max_passes"}
    assert names <= declared_symbols() and names <= set(_lib.SIGNATURES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    assert names <= set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 15
    assert lib.mccnn_batch_sample_chunk() == 1024 and lib.mccnn_batch_max_passes() == ref.MAX_PASSES == 64
    hdr = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    body = hdr[hdr.index("typedef struct mccnn_batch_slot {"):hdr.index("} mccnn_batch_slot;")]
    fields = re.findall(r"\b(?:int|unsigned|float)\s+([a-z_0-9\[\], ]+);", body)
    flat = [re.sub(r"\[\d+\]", "", f.strip()) for grp in fields for f in grp.split(",")]
    assert flat == list(SLOT_DTYPE.names), (flat, SLOT_DTYPE.names)
    # argument errors are caught on the host, before any launch: a slot that would write past the output, a model past the store
    s = new_slots(1)
    s["length"], s["n_sel"], s["rows"] = 4, 4, 8
    call = lambda store_rows, out_rows: lib.mccnn_batch_sample(ctypes.c_void_p(256), None, store_rows, s.ctypes.data, 1, out_rows,
                                                              ctypes.c_void_p(256), ctypes.c_void_p(256), ctypes.c_void_p(256),
                                                              ctypes.c_void_p(256), ctypes.c_void_p(256), None)
    assert call(4, 7) == -1 and call(3, 8) == -1
    s["protocol"] = 3
    assert call(4, 8) == -1   # lambert without normals


def test_host_checker_builds_and_agrees_with_numpy(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "batch_sample_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "batch_sample_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 disagreements" in r.stdout, r.stdout + r.stderr
    lines = subprocess.run([exe, "--dump"], capture_output=True, text=True, check=True).stdout.splitlines()
    seen = {"U": 0, "D": 0}
    for line in lines:
        head, vals = line.split(":")
        kind, *a = head.split()
        vals = np.array([int(v) for v in vals.split()], np.int64)
        if kind == "U":
            n, K, seed = (int(x) for x in a)
            assert np.array_equal(ref.uniform_indices(n, K, seed), vals), head
        else:
            seed, t = (int(x) for x in a)
            probes = np.array([0, 1, 2, 3, 1023, 1024, 99999, 0x7FFFFFFE], np.uint64)
            want = ref.mix((ref.pass_hash(seed, t) + probes) & ref.U32) >> np.uint64(8)
            assert np.array_equal(want.astype(np.int64), vals), head
            u = ref.draws(seed, t, 1025)
            assert u.dtype == np.float32 and np.array_equal((u.astype(np.float64) * 2 ** 24).astype(np.int64)[[0, 1, 2, 3, 1023, 1024]], vals[:6])
        seen[kind] += 1
    assert seen["U"] == 32 and seen["D"] == 12
