"""The device batcher's kernel (mccnn_batch_sample) against its NumPy float32 restatement (tests/device_batcher_ref.py) on
explicit plans: source rows, batch ids, counts and status equal, coordinates bit-equal; then DeviceBatcher end to end.

W = mccnn_batch_sample_chunk() points per workgroup iteration. The store holds models of 1, W-1, W, W+1 and 2W+37 points
(so that none but the first starts at offset 0), one of 50 and one of 5000 points, all with normals, three features and a
label column."""
import numpy as np
import pytest

from mccnn_amd.device_batcher import DeviceBatcher, DeviceStore, new_slots, sample_plan
from tests import device_batcher_ref as ref

pytestmark = pytest.mark.gpu

_CACHE = {}


def _chunk():
    from mccnn_amd import _lib
    return _lib.load().mccnn_batch_sample_chunk()


def _models():
    """Ellipsoid shells with outward normals; computed once, never modified."""
    if "models" not in _CACHE:
        W = _chunk()
        rs = np.random.RandomState(17)
        models = []
        for n in (1, W - 1, W, W + 1, 2 * W + 37, 50, 5000):
            d = rs.randn(n, 3)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            pts = d * np.array([1.0, 0.6, 0.4]) + 0.01 * rs.randn(n, 3) + rs.rand(3)
            models.append({"pts": pts.astype(np.float32), "normals": d.astype(np.float32),
                           "features": rs.randn(n, 3).astype(np.float32), "labels": rs.randint(0, 9, (n, 1)).astype(np.int64)})
        _CACHE["models"] = models
    return _CACHE["models"]


def _store(mc):
    if "store" not in _CACHE:
        m = _models()
        _CACHE["store"] = (DeviceStore(m), np.concatenate([x["pts"] for x in m]), np.concatenate([x["normals"] for x in m]))
    return _CACHE["store"]


def _random_rotation(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q.astype(np.float32).reshape(9)


def _plan(store, entries, seed=1, exact=True):
    """entries: (model, protocol, rows) -> slots with random views, rotations and seeds, packed output rows. rows = None
    with exact=False: the slot's capacity (the model's length)."""
    rs = np.random.RandomState(seed)
    slots = new_slots(len(entries))
    base = 0
    for k, (model, proto, rows) in enumerate(entries):
        s = slots[k]
        store.fill_model(s, model)
        v = rs.randn(3)
        s["protocol"], s["view"], s["rot"] = proto, v / np.linalg.norm(v), _random_rotation(rs)
        s["seed"], s["batch_id"], s["exact"] = rs.randint(0, 2 ** 32, dtype=np.uint32), 2 * k + 1, int(exact)
        s["rows"] = int(s["length"]) if rows is None else rows
        s["out_base"] = base
        base += int(s["rows"])
    return slots, base


def _gpu(store, slots, out_rows, stream=None):
    import torch
    out = sample_plan(store, slots, out_rows, stream=stream)
    if stream is not None:
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    pts, bids, src, counts, status = (t.cpu().numpy() for t in out)
    return {"pts": pts, "bids": bids[:, 0], "src": src, "counts": counts, "status": status}


def _check(got, want, slots):
    print("counts", list(got["counts"]), "status", list(got["status"]))
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    w = want["written"]
    for s, c in zip(slots, want["counts"]):   # every row an exact slot owns is written, of the others the first `count`
        b = int(s["out_base"])
        assert w[b:b + (int(s["rows"]) if s["exact"] else int(c))].all()
    assert np.array_equal(got["src"][w], want["src"][w]), "source rows differ in %d rows" % int((got["src"][w] != want["src"][w]).sum())
    assert np.array_equal(got["bids"][w], want["bids"][w])
    a, b = got["pts"][w].view(np.uint32), want["pts"][w].view(np.uint32)
    assert np.array_equal(a, b), "coordinates differ in %d rows" % int((a != b).any(axis=1).sum())


def _compare(mc, entries, seed=1, exact=True, edit=None):
    store, P, Nr = _store(mc)
    slots, out_rows = _plan(store, entries, seed, exact)
    if edit is not None:
        edit(slots)
    want = ref.run_plan(slots, P, Nr, out_rows)
    got = _gpu(store, slots, out_rows)
    _check(got, want, slots)
    return slots, got, want


def test_every_protocol_on_every_model_in_one_batch(mc):
    """5 models (1, W-1, W, W+1, 2W+37 points) x 5 protocols = 25 mixed slots of 300 rows in one launch. The one-point model
    has a box of zero size: its probabilities and its projection are the degenerate values both sides define the same way,
    and its slots end in whichever status the restatement gives."""
    entries = [(m, p, 300) for m in range(5) for p in range(5)]
    slots, got, want = _compare(mc, entries)
    assert (want["status"] == ref.OK).sum() >= 18
    assert set(slots["protocol"][want["status"] == ref.OK]) == {0, 1, 2, 3, 4}


def test_more_slots_than_one_launch_takes(mc):
    entries = [(1 + (k % 4), k % 5, 64 + k) for k in range(37)]
    _compare(mc, entries, seed=2)


def test_rows_cut_the_first_pass_mid_wave_and_mid_chunk(mc):
    """The 5000-point model: split accepts ~62 % per pass, so 700 rows end inside the second chunk, 100 rows inside the
    second wave of the first chunk, 1 row at the first accepted point; 4000 rows need a second pass that is cut."""
    _compare(mc, [(6, 1, 700), (6, 1, 100), (6, 2, 1), (6, 1, 4000), (6, 3, 333), (4, 2, _chunk() + 1)], seed=3)


def test_three_or_more_passes(mc):
    """The 50-point model with 1024 rows: every pass yields at most 50."""
    slots, got, want = _compare(mc, [(5, 1, 1024), (5, 2, 1024), (5, 0, 1024), (5, 4, 1024)], seed=4)
    assert np.all(want["status"] == ref.OK) and np.all(want["counts"] == 1024)


def test_variable_counts(mc):
    """numPoints == 0: one pass, slots write from the prefix of their capacities, the counts cut the result."""
    K = int(5000 * 0.9)
    entries = [(6, 0, K), (6, 1, None), (4, 2, None), (3, 3, None), (6, 4, None), (0, 1, None), (2, 4, None)]
    slots, got, want = _compare(mc, entries, seed=5, exact=False)
    assert want["counts"][0] == K and 0 < want["counts"][1] < 5000 and np.all(want["status"] == ref.OK)


def test_no_facing_normal_and_the_pass_bound(mc):
    """Plain inputs, not faults: lambert with every normal turned away ends with NO_POINT after its first pass; a model
    whose only facing normal yields one row per pass is PASS_BOUND after 64 passes, through the ordinary loop exit. Both
    fill the rows they did not produce with the model's row 0."""
    view = np.array([0.0, 0.0, 1.0], np.float32)
    rs = np.random.RandomState(8)
    away = {"pts": rs.rand(200, 3).astype(np.float32), "normals": np.tile(-view, (200, 1))}
    one = {"pts": rs.rand(3, 3).astype(np.float32), "normals": np.stack([-view, view, -view])}
    store = DeviceStore([away, one])
    P, Nr = np.concatenate([away["pts"], one["pts"]]), np.concatenate([away["normals"], one["normals"]])
    slots, out_rows = _plan(store, [(0, 3, 128), (1, 3, 1024), (0, 4, 77), (1, 3, 64)], seed=6)
    slots["view"] = view
    slots["view"][2] = -view   # occlusion keeps the points whose normal looks AT the camera: none here either
    want = ref.run_plan(slots, P, Nr, out_rows)
    got = _gpu(store, slots, out_rows)
    _check(got, want, slots)
    assert list(got["status"]) == [ref.NO_POINT, ref.PASS_BOUND, ref.NO_POINT, ref.OK]
    assert list(got["counts"]) == [0, ref.MAX_PASSES, 0, 64]
    assert np.all(got["src"][:128] == 0) and np.all(got["src"][128 + 64:128 + 1024] == 200) and np.all(got["src"][128:128 + 64] == 201)


def test_occlusion_with_shared_pixels_and_equal_depths(mc):
    """A 150 x 150 lattice over a screen of ~83 pixels per unit length (about two lattice points per pixel and axis), every
    point twice at the same depth, a second layer 0.005 behind (inside the 0.01 window once depth is normalised) and a
    third 0.6 behind (hidden when the view is head-on: same pixels)."""
    g = np.stack(np.meshgrid(np.arange(150), np.arange(150), indexing="ij"), -1).reshape(-1, 2) / 149.0
    front = np.concatenate([g, np.zeros((len(g), 1))], axis=1)
    pts = np.concatenate([front, front, front + [0, 0, 0.005], front + [0, 0, 0.6]]).astype(np.float32)
    nr = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (len(pts), 1))
    store = DeviceStore([{"pts": pts, "normals": nr}])
    slots, out_rows = _plan(store, [(0, 4, None), (0, 4, None)], seed=7, exact=False)
    slots["view"][0] = [0.0, 0.0, 1.0]
    slots["view"][1] = np.array([0.3, 0.2, 0.9]) / np.linalg.norm([0.3, 0.2, 0.9])
    want = ref.run_plan(slots, pts, nr, out_rows)
    got = _gpu(store, slots, out_rows)
    _check(got, want, slots)
    n = len(g)
    assert want["counts"][0] == 3 * n   # both copies and the near layer; the far layer is hidden
    assert 0 < want["counts"][1] < len(pts)


def test_uniform_sizes(mc):
    """n > K, n == K (every point exactly once), n < K (with replacement), and a cut to the first n_sel points."""
    W = _chunk()

    def edit(slots):
        slots["n_sel"][3] = 1126
    slots, got, want = _compare(mc, [(4, 0, 1024), (2, 0, W), (5, 0, 1024), (6, 0, 1024), (0, 0, 5)], seed=9, edit=edit)
    store = _store(mc)[0]
    assert np.array_equal(got["src"][1024:1024 + W], store.offsets[2] + np.arange(W))
    seg = got["src"][1024 + W + 1024:1024 + W + 2048] - store.offsets[6]
    assert np.all(np.diff(seg) > 0) and seg.max() < 1126
    assert np.all(np.diff(got["src"][:1024]) > 0)


def test_two_builds_give_the_same_bytes_and_streams_do_not_matter(mc):
    import torch
    store, P, Nr = _store(mc)
    slots, out_rows = _plan(store, [(m, p, 500) for m in (3, 4, 6) for p in range(5)], seed=10)
    a = _gpu(store, slots, out_rows)
    b = _gpu(store, slots, out_rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    c = _gpu(store, slots, out_rows, stream=side)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def _batcher(**kw):
    args = dict(numPoints=256, ptDropOut=0.9, batchSize=4, allowedSamplings=[0, 1, 2, 3, 4], categories=[3, 1, 4, 1, 5, 9, 2], augment=True,
                augmentSmallRotations=True, augmentedFeatures=(0,), seed=11)
    args.update(kw)
    return DeviceBatcher(_models()[1:], **args)


def test_batcher_features_labels_and_trailing_empty_slots(mc):
    """Six models in batches of four: the second batch has two trailing empty slots. Features [N,3] with their one block
    rotated by the slot's matrix (a torch product: 4 eps max|value| sqrt(3)), labels and categories through the index."""
    import torch
    models = _models()[1:]
    P = np.concatenate([m["pts"] for m in models])
    Nr = np.concatenate([m["normals"] for m in models])
    Fe = np.concatenate([m["features"] for m in models])
    La = np.concatenate([m["labels"] for m in models])
    db, twin = _batcher(), _batcher()
    db.start_iteration()
    twin.start_iteration()
    sizes = []
    while db.has_more_batches():
        plan = twin.plan_batch()
        want = ref.run_plan(plan["slots"], P, Nr, plan["out_rows"])
        num, pts, bids, feats, labels, cats, ids = db.get_next_batch()
        torch.cuda.synchronize()
        N = num * 256
        sizes.append(num)
        assert np.all(want["status"] == ref.OK) and ids == plan["ids"]
        assert pts.shape == (N, 3) and pts.dtype == torch.float32 and bids.shape == (N, 1) and bids.dtype == torch.int32
        assert feats.shape == (N, 3) and feats.dtype == torch.float32 and labels.shape == (N, 1)
        assert np.array_equal(pts.cpu().numpy().view(np.uint32), want["pts"].view(np.uint32))
        assert np.array_equal(bids.cpu().numpy()[:, 0], want["bids"])
        assert np.array_equal(bids.cpu().numpy()[:, 0], np.repeat(np.arange(num), 256))
        rot = np.repeat(plan["slots"]["rot"].reshape(-1, 3, 3), 256, axis=0).astype(np.float64)
        f = Fe[want["src"]].astype(np.float64)
        f_want = np.einsum("ni,nij->nj", f, rot)
        tol = 4 * np.finfo(np.float32).eps * np.abs(f).max() * np.sqrt(3.0)
        err = np.abs(feats.cpu().numpy() - f_want).max()
        print("feature rotation max err %.3g (bound %.3g), launches %d" % (err, tol, db.lastLaunches_))
        assert err <= tol
        assert np.array_equal(labels.cpu().numpy(), La[want["src"]])
        assert cats.cpu().tolist() == plan["categories"]
        assert db.lastLaunches_ == 3   # the kernel and the two gathers
    assert sizes == [4, 2]


def test_batcher_variable_counts_and_status(mc):
    import torch
    models = _models()[1:]
    P = np.concatenate([m["pts"] for m in models])
    Nr = np.concatenate([m["normals"] for m in models])
    db, twin = _batcher(numPoints=0, pointCategories=True, augmentedFeatures=()), _batcher(numPoints=0, pointCategories=True, augmentedFeatures=())
    db.start_iteration()
    twin.start_iteration()
    plan = twin.plan_batch()
    want = ref.run_plan(plan["slots"], P, Nr, plan["out_rows"])
    out = db.get_next_batch(check=False)
    assert len(out) == 8
    num, pts, bids, feats, labels, cats, ids, status = out
    torch.cuda.synchronize()
    w = want["written"]
    assert pts.shape[0] == int(want["counts"].sum()) == int(w.sum()) and cats.shape == (pts.shape[0], 1)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), want["pts"][w].view(np.uint32))
    assert np.array_equal(bids.cpu().numpy()[:, 0], want["bids"][w])
    assert np.array_equal(status.cpu().numpy(), want["status"])
    assert np.array_equal(cats.cpu().numpy()[:, 0], np.repeat(plan["categories"], want["counts"]))
    # check=True raises the host batcher's error for a slot that can select nothing
    view = np.array([0.0, 0.0, 1.0])
    away = [{"pts": np.random.RandomState(1).rand(64, 3), "normals": np.tile(-view, (64, 1))}]
    bad = DeviceBatcher(away, 32, 1.0, 1, [3], seed=1)
    bad.start_iteration()
    plan = bad.plan_batch()
    plan["slots"]["view"] = view
    with pytest.raises(RuntimeError, match="no point can be selected"):
        bad.build_batch(plan)


def test_network_layer_over_a_device_built_batch(mc):
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    db = _batcher(augmentedFeatures=())
    db.start_iteration()
    num, pts, bids, feats, labels, cats, ids = db.get_next_batch()
    ph = PointHierarchy(pts, feats, bids, [0.25], "PH", 4, True)
    cb = ConvolutionBuilder(KDEWindow=0.2, relativeRadius=True)
    cb.reset()
    out = cb.create_convolution("C", ph, 0, feats, 3, 0.3, outNumFeatures=8, multiFeatureConv=True)
    torch.cuda.synchronize()
    assert out.shape == (num * 256, 8) and bool(torch.isfinite(out).all())
    assert float(out.detach().abs().max()) > 0
