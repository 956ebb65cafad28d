"""Cases, the op-by-op driver and the comparisons shared by tests/ref_runner.py (runs the REFERENCE's own kernels, built
by oracle/ref_build.py, in a child process), tests/test_gpu_reference.py and tests/test_oracle_pinned_cpu.py.

Pinning is op by op ON IDENTICAL INPUTS: whoever runs (`ops`: the oracle, the reference binding or the HIP ops), each op
is fed the ORACLE's outputs of the preceding ops (`src`), not its own, so that the reference's two arrival-order
nondeterminisms -- the order inside a grid cell (sort_gpu.cu:170) and the Poisson output order
(poisson_sampling.cu:115) -- cannot cascade into later ops.

Inputs are regenerated from seeds (tests.helpers); only recorded reference OUTPUTS are ever stored.
"""
import numpy as np

from tests.helpers import make_cloud, make_mlp, conv_nb, assert_float_close

RTOL = 1e-4   # north star: float outputs within 1e-4 relative, norm-wise and per element (tests.helpers)
WINDOW = 0.2
GRADS = ["featGrad", "dw1", "db1", "dw2", "db2", "dw3", "db3"]


def _conv(name, fin, fout, combin, avg, bf16=False, nostate=False):
    return dict(name=name, fin=fin, fout=fout, combin=combin, avg=avg, bf16=bf16, nostate=nostate)


def _lattice(seed, n, B):
    """Coordinates are multiples of 1/64 in [0, 1], half of the points on multiples of 4/64 (the cell faces of a 16^3
    grid and, along an axis, partners at distance EXACTLY 4/64), with duplicates; both box corners are present, so the
    box is [0, 1]^3 bit for bit. Differences, their squares and the sums of three squares are exact in f32 (numerators
    below 2^14 over 2^12) with or without fused multiply-adds, so every `dist < radius` and every floor((p - min) /
    cell) is decided ON the boundary, identically under any contraction."""
    rng = np.random.default_rng(seed)
    pts, bids = [], []
    for b in range(B):
        coarse = rng.integers(0, 17, size=(n // 2, 3)) * 4
        fine = rng.integers(0, 65, size=(n - n // 2 - 2 - 40, 3))
        dup = coarse[rng.integers(0, len(coarse), 40)]
        p = np.concatenate([[[0, 0, 0], [64, 64, 64]], coarse, fine, dup]).astype(np.float32) / np.float32(64.0)
        rng.shuffle(p)
        pts.append(p)
        bids.append(np.full((len(p), 1), b, np.int32))
    return np.concatenate(pts).astype(np.float32), np.concatenate(bids).astype(np.int32)


def _g(name, n_per, B, kind, ragged, radius, scaleInv, fin, prad):
    return dict(name=name, cloud=("make_cloud", n_per, B, 11, kind, ragged), B=B, radius=radius, scaleInv=scaleInv,
                fin=fin, prads=[prad], convs=[])


def _c(name, fin, fout, combin, avg, scaleInv, radius, **kw):
    # the cloud of tests/test_gpu_parity.py::test_spatial_conv_fwd_bwd
    return dict(name="conv_" + name, cloud=("make_cloud", 1500, 2, 21, "clustered", True), B=2, radius=radius,
                scaleInv=scaleInv, fin=fin, prads=[], convs=[_conv(name, fin, fout, combin, avg, **kw)], signed=True)


CASES = [
    # the geometry cases of tests/test_gpu_parity.py::CASES (name, n_per, B, kind, ragged, radius, scaleInv, Fin, poisson radius)
    _g("cfg0_uniform4096", 4096, 1, "uniform", False, 0.1, True, 3, 0.1),
    _g("batched_sphere", 1024, 8, "sphere", False, 0.2, True, 1, 0.1),
    _g("ragged_clustered", 700, 5, "clustered", True, 0.15, True, 4, 0.05),
    _g("abs_radius_batched", 1500, 3, "uniform", True, 0.12, False, 3, 0.2),
    _g("single_cell", 300, 4, "uniform", False, 1.2, True, 2, 1.3),
    _g("tiny", 3, 2, "uniform", False, 0.5, True, 1, 0.5),
    # 2.56 M cells: the reference's two-level scan (512 cells per block, 512 blocks per second-level block, the third
    # level a loop of atomic adds over up to 512 entries: sort_gpu.cu:137-145, 456-468) covers 5000 / 10 blocks
    _g("fine_grid_3level_scan", 1500, 5, "uniform", True, 0.0125, True, 1, 0.0125),
    dict(name="dense_blob", cloud=("dense_blob",), B=1, radius=0.1, scaleInv=True, fin=2, prads=[0.1], convs=[]),
    dict(name="pooling_centres", cloud=("make_cloud", 2000, 3, 5, "uniform", False), B=3, radius=0.2, scaleInv=True, fin=2,
         prads=[], convs=[], centres="jittered"),
    dict(name="empty_rows", cloud=("make_cloud", 1200, 1, 33, "clustered", True), B=1, radius=0.2, scaleInv=False, fin=1,
         prads=[], convs=[_conv("1to16", 1, 16, True, True)], centres="far", signed=True),
    dict(name="translated_500", cloud=("make_cloud", 3000, 2, 17, "uniform", False), B=2, radius=0.1, scaleInv=False,
         fin=1, prads=[0.2], convs=[], translate=500.0),
    dict(name="lattice_abs", cloud=("lattice", 2000, 2, 41), B=2, radius=4 / 64, scaleInv=False, fin=2,
         prads=[4 / 64, 8 / 64], convs=[_conv("2to5", 2, 5, True, True)], signed=True),
    dict(name="lattice_scaleinv", cloud=("lattice", 3000, 1, 43), B=1, radius=4 / 64, scaleInv=True, fin=1,
         prads=[4 / 64, 8 / 64], convs=[_conv("1to16", 1, 16, True, True)], signed=True),
    # small enough to be kept as a fixture: a ragged batch with a combining and a depth-wise layer
    dict(name="small_ragged_conv", cloud=("make_cloud", 150, 3, 19, "clustered", True), B=3, radius=0.2, scaleInv=True,
         fin=8, prads=[0.2], convs=[_conv("8to3", 8, 3, True, True), _conv("dw8_noavg", 8, 8, False, False)], signed=True),
    # convolution shapes of tests/test_gpu_parity.py::CONV_CASES, one per kernel family
    _c("3to8", 3, 8, True, True, True, 0.1),
    _c("1to16", 1, 16, True, True, True, 0.15),
    _c("2to5_padded", 2, 5, True, True, True, 0.15),
    _c("8to3_generic", 8, 3, True, True, True, 0.15),
    _c("dw32", 32, 32, False, True, True, 0.15),
    _c("dw8_noavg_abs", 8, 8, False, False, False, 0.12),
    _c("1to13_noavg_abs", 1, 13, True, False, False, 0.12),
    _c("1to64_nostate", 1, 64, True, True, True, 0.15, nostate=True),
    _c("dw32_bf16rows", 32, 32, False, True, True, 0.15, bf16=True),
    # depth-wise widths that are no multiple of 8: the scalar instantiations of the HIP streaming kernels
    _c("dw12_padded", 12, 12, False, True, True, 0.15),
    _c("dw4_noavg_abs", 4, 4, False, False, False, 0.12),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
#: the smallest cases, whose reference outputs are kept as fixtures tests/golden/ref_<name>.npz
GOLDEN_CASES = ["tiny", "small_ragged_conv", "lattice_abs", "lattice_scaleinv"]


def bf16_round(a):
    """float32 -> the float32 values of its bfloat16 rounding, round to nearest even (as tests/test_gpu_configs.py)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def make_inputs(case):
    kind = case["cloud"][0]
    if kind == "make_cloud":
        _, n_per, B, seed, ckind, ragged = case["cloud"]
        pts, bids = make_cloud(n_per, B, seed, ckind, ragged)
    elif kind == "lattice":
        _, n, B, seed = case["cloud"]
        pts, bids = _lattice(seed, n, B)
    elif kind == "dense_blob":  # tests/test_gpu_parity.py::test_dense_cells
        rng = np.random.default_rng(13)
        blob = (0.5 + 0.012 * rng.normal(size=(900, 3))).astype(np.float32)
        rest = rng.random((400, 3), dtype=np.float32)
        pts = np.concatenate([blob, rest]).astype(np.float32)
        rng.shuffle(pts)
        bids = np.zeros((len(pts), 1), np.int32)
    else:
        raise ValueError(kind)
    if case.get("translate"):
        pts = (pts + np.float32(case["translate"])).astype(np.float32)
    rng = np.random.default_rng(3)
    feats = rng.random((len(pts), case["fin"]))
    feats = ((2 * feats - 1) if case.get("signed") else feats).astype(np.float32)
    centres, cb = pts, bids
    if case.get("centres") == "jittered":   # a pooling search: fewer, unsorted centres, some of them outside the box
        r9 = np.random.default_rng(9)
        sel = np.sort(r9.choice(len(pts), 500, replace=False))
        centres = (pts[sel] + 0.01 * r9.normal(size=(500, 3))).astype(np.float32)
        cb = bids[sel]
    elif case.get("centres") == "far":      # rows without an edge at the start, in the middle and at the end
        far = np.array([[9.0, 9.0, 9.0]], np.float32)
        centres = np.concatenate([far, far + 1, pts[:300], far + 2, far + 3, far + 4, pts[300:500], far + 5]).astype(np.float32)
        cb = np.zeros((len(centres), 1), np.int32)
    inp = dict(pts=pts, bids=bids, feats=feats, centres=centres, cb=cb, convs=[])
    r5 = np.random.default_rng(5)
    inp["g3"] = (2 * r5.random((len(pts), 3)) - 1).astype(np.float32)
    inp["gF"] = (2 * r5.random(feats.shape) - 1).astype(np.float32)
    for ci, cv in enumerate(case["convs"]):
        outF = cv["fout"] if cv["combin"] else cv["fin"]
        og = (2 * np.random.default_rng(11 + ci).random((len(centres), outF)) - 1).astype(np.float32)
        inp["convs"].append(dict(w=make_mlp(conv_nb(cv["fin"], cv["fout"], cv["combin"]), 7), og=bf16_round(og) if cv["bf16"] else og))
    if any(cv["bf16"] for cv in case["convs"]):
        inp["feats"] = bf16_round(inp["feats"])
    return inp


def run_ops(ops, case, inp, src=None):
    """Every op of the chain once, through `ops` (NumPy in, NumPy out, the oracle's method names). src: the oracle's
    outputs of the same case; each op then reads ITS inputs from src. Without src the chain feeds on itself."""
    B, radius, sI = case["B"], case["radius"], case["scaleInv"]
    pts, bids, feats = inp["pts"], inp["bids"], inp["feats"]
    o = {}
    s = o if src is None else src
    o["aabbMin"], o["aabbMax"] = ops.compute_aabb(pts, bids, B, sI)
    mn, mx = s["aabbMin"], s["aabbMax"]
    o["keys"], o["indexs"] = ops.sort_points_step1(pts, bids, mn, mx, B, radius, sI)
    o["sortPts"], o["sortBatchs"], o["sortFeatures"], o["cellIndexs"] = ops.sort_points_step2(
        pts, bids, feats, s["keys"], s["indexs"], mn, mx, B, radius, sI)
    o["step2GradPts"], o["step2GradFeats"] = ops.sort_points_step2_grad(s["indexs"], inp["g3"], inp["gF"])
    o["featsBack"] = ops.sort_features_back(inp["gF"], s["indexs"])
    o["featsSorted"] = ops.sort_features(inp["gF"], s["indexs"])
    o["startIndexs"], o["packedNeighs"] = ops.find_neighbors(inp["centres"], inp["cb"], s["sortPts"], s["cellIndexs"],
                                                             mn, mx, radius, B, sI)
    o["pdfs"] = ops.compute_pdf(s["sortPts"], s["sortBatchs"], mn, mx, s["startIndexs"], s["packedNeighs"], WINDOW,
                                radius, B, sI)
    for j, prad in enumerate(case["prads"]):
        p = "p%d_" % j
        if src is None:  # a second grid at the Poisson radius, like PointHierarchy.__init__ (MCConvBuilder.py:101-116)
            k2, i2 = ops.sort_points_step1(pts, bids, mn, mx, B, prad, sI)
            p2, b2, f2, c2 = ops.sort_points_step2(pts, bids, feats, k2, i2, mn, mx, B, prad, sI)
            o["_" + p + "grid"] = (i2, p2, b2, f2, c2)
        i2, p2, b2, f2, c2 = s["_" + p + "grid"]
        o[p + "samplePts"], o[p + "sampleBatchs"], o[p + "sampleIndexs"] = ops.poisson_sampling(p2, b2, c2, mn, mx, prad, B, sI)
        si = s[p + "sampleIndexs"]
        o[p + "transformedIndexs"] = ops.transform_indexs(si, i2)
        o[p + "sampleFeatures"] = ops.get_sampled_features(si, f2)
        gs = inp["gF"][:len(si)]
        o[p + "sampleFeaturesGrad"] = ops.get_sampled_features_grad(si, f2, gs)
    for cv, ci in zip(case["convs"], inp["convs"]):
        w = ci["w"]
        a = (s["sortPts"], s["sortFeatures"], s["sortBatchs"], s["pdfs"], inp["centres"], s["startIndexs"],
             s["packedNeighs"], mn, mx, w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
        kw = dict(bf16=cv["bf16"], nostate=cv["nostate"]) if getattr(ops, "IS_HIP", False) else {}
        c = "c_%s_" % cv["name"]
        o[c + "out"] = ops.spatial_conv(*a, cv["fout"], cv["combin"], B, radius, sI, cv["avg"], **kw)
        g = ops.spatial_conv_grad(*a, ci["og"], cv["fout"], cv["combin"], B, radius, sI, cv["avg"], **kw)
        for nm, v in zip(GRADS, g):
            o[c + nm] = np.asarray(v)
    return o


def public(o):
    """What is stored of a run: everything but the private feed entries."""
    return {k: np.asarray(v) for k, v in o.items() if not k.startswith("_")}


# ------------------------------------------------------------------------------------------------- comparisons
EXACT = ["aabbMin", "aabbMax",                                   # pure min / max
         "keys",                                                  # the cell of every point
         "sortPts", "sortBatchs", "sortFeatures", "cellIndexs",   # step 2 on the oracle's indexs: copies and the cell table
         "step2GradPts", "step2GradFeats", "featsBack", "featsSorted",
         "startIndexs", "packedNeighs"]                           # rows as written: one thread fills a row in cell-visit order


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    assert a.dtype == b.dtype, "%s: dtype %s vs %s" % (what, a.dtype, b.dtype)
    assert np.array_equal(a, b), "%s differs in %d of %d elements" % (what, int((a != b).sum()), a.size)


def _bf16_close(got, ref32, what):
    # rows stored in bf16 (tests/test_gpu_configs.py::bf16_close): equal to the rounded f32 rows or one bf16 step apart
    ref = bf16_round(ref32)
    scale = float(np.abs(ref32).max())
    diff = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(diff <= 2.0 ** -7 * np.abs(ref) + 1e-6 * scale), what
    return float(diff.max() / max(scale, 1e-30))


def compare(case, got, ref, what, arrival_order_free, got_bf16_rows=False):
    """Holds `got` to `ref` (dicts of run_ops) and returns {output: max |diff| / max |ref|} of the float comparisons.
    arrival_order_free: one side is the reference, whose order inside a cell and whose Poisson output order are
    whatever the atomics gave: `indexs` is then checked as a valid outcome with the same cell contents, and the Poisson
    outputs are compared after sorting by sampled index. Nothing else is order-free, and no element is exempt."""
    errs = {}
    tag = "%s [%s]: " % (case["name"], what)
    for k in EXACT:
        _same(got[k], ref[k], tag + k)
    n = len(ref["keys"])
    if arrival_order_free:
        for side in (got, ref):
            idx, keys = side["indexs"], ref["keys"]
            assert idx.shape == (n,) and np.array_equal(np.sort(idx), np.arange(n)), tag + "indexs is not a permutation"
            sk = np.empty(n, keys.dtype)
            sk[idx] = keys
            assert np.all(np.diff(sk) >= 0), tag + "keys[indexs] decreases"
        pair = lambda d: np.stack([ref["keys"], d["indexs"]], 1)[np.lexsort((d["indexs"], ref["keys"]))]
        _same(pair(got), pair(ref), tag + "positions per cell")
    else:
        _same(got["indexs"], ref["indexs"], tag + "indexs")
    errs["pdfs"] = assert_float_close(got["pdfs"], ref["pdfs"], RTOL, tag + "pdfs")
    for j in range(len(case["prads"])):
        p = "p%d_" % j
        g = {k: got[p + k] for k in ("samplePts", "sampleBatchs", "sampleIndexs")}
        r = {k: ref[p + k] for k in ("samplePts", "sampleBatchs", "sampleIndexs")}
        assert len(g["sampleIndexs"]) == len(r["sampleIndexs"]), tag + p + "sample count %d vs %d" % (
            len(g["sampleIndexs"]), len(r["sampleIndexs"]))
        if arrival_order_free:
            og_, or_ = np.argsort(g["sampleIndexs"], kind="stable"), np.argsort(r["sampleIndexs"], kind="stable")
            g, r = {k: v[og_] for k, v in g.items()}, {k: v[or_] for k, v in r.items()}
        for k in g:
            _same(g[k], r[k], tag + p + k)
        for k in ("transformedIndexs", "sampleFeatures", "sampleFeaturesGrad"):
            _same(got[p + k], ref[p + k], tag + p + k)
    for cv in case["convs"]:
        c = "c_%s_" % cv["name"]
        rows = ("out", "featGrad") if (got_bf16_rows and cv["bf16"]) else ()
        for nm in ["out"] + GRADS:
            if nm in rows:
                errs[c + nm] = _bf16_close(got[c + nm], ref[c + nm], tag + c + nm)
            else:
                errs[c + nm] = assert_float_close(got[c + nm], ref[c + nm], RTOL, tag + c + nm)
    return errs


def boundary_census(case, inp, o):
    """How many decisions of a case sit exactly ON a boundary (oracle outputs o): ordered pairs at distance == radius
    (so `<` against `<=` changes the neighbour list) and coordinates with (p - min) / cell an exact integer."""
    mn, mx = o["aabbMin"].astype(np.float32), o["aabbMax"].astype(np.float32)
    nc = o["cellIndexs"].shape[1]
    on_face = at_radius = 0
    for b in range(case["B"]):
        ext = np.float32((mx[b] - mn[b]).max())
        cell = np.float32(ext / np.float32(nc))
        rad = np.float32(np.float32(case["radius"]) * ext) if case["scaleInv"] else np.float32(case["radius"])
        P = inp["pts"][inp["bids"][:, 0] == b]
        q = ((P - mn[b]) / cell).astype(np.float32)
        on_face += int(np.any(q == np.floor(q), axis=1).sum())
        d = P[:, None, :] - P[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(np.float32)
        at_radius += int((np.sqrt(d2).astype(np.float32) == rad).sum())
    return on_face, at_radius
