"""pdfMode='point' on the GPU: compute_pdf_points against the float64 reference over the ORACLE's rows (tests/point_pdf_ref.py)
-- counts bit for bit, density within the project's bar -- on geometries that reach every regime of the window sweep;
expand_pdf bit for bit; both tied to the oracle's own compute_pdf where the two definitions coincide; the builder end to end.

Largest density error seen (max |diff| / max |ref|, MI355X): see NOTES.md, "Per-point KDE"."""
import numpy as np
import pytest

from tests import neighbor_cap_ref as geo
from tests import point_pdf_ref as ref
from tests.helpers import assert_float_close

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # the project's bar for float outputs (norm-wise and per element: tests/helpers.py)
WINDOW = 0.25
SELF_TERM = (0.39894228 / WINDOW) ** 3

_REFS = {}   # case name -> the oracle's grid and the reference density: computed once, never modified


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _reference(oracle, name, pts, bids, B, radius, scaleInv, window=WINDOW):
    if name not in _REFS:
        mn, mx, sP, sB, cells, idx = ref.sorted_grid(oracle, pts, bids, B, radius, scaleInv)
        density, counts = ref.density_ref(oracle, sP, sB, cells, mn, mx, window, radius, B, scaleInv)
        _REFS[name] = dict(mn=mn, mx=mx, sP=sP, sB=sB, cells=cells, idx=idx, density=density, counts=counts)
    return _REFS[name]


def _gpu_grid(mc, pts, bids, B, radius, scaleInv):
    P, Bi = _wrap(pts), _wrap(bids)
    mn, mx = mc.compute_aabb(P, Bi, B, scaleInv)
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, B, radius, scaleInv)
    return dict(P=P, Bi=Bi, mn=mn, mx=mx, sP=sP, sB=sB, cells=cells, idx=idx)


def _check_density(mc, oracle, name, pts, bids, B, radius, scaleInv, window=WINDOW):
    r = _reference(oracle, name, pts, bids, B, radius, scaleInv, window)
    h = _gpu_grid(mc, pts, bids, B, radius, scaleInv)
    assert np.array_equal(_unwrap(h["sP"]), r["sP"]) and np.array_equal(_unwrap(h["cells"]), r["cells"])
    density, counts = mc.compute_pdf_points(h["sP"], h["sB"], h["cells"], h["mn"], h["mx"], window, radius, B, scaleInv)
    n = len(pts)
    assert density.shape == (n, 1) and counts.shape == (n, 1)
    assert str(density.dtype) == "torch.float32" and str(counts.dtype) == "torch.int32"
    d, c = _unwrap(density), _unwrap(counts)
    bad = int((c != r["counts"]).sum())
    scale = max(float(np.abs(r["density"]).max()), 1e-30)
    err = float(np.abs(d - r["density"]).max() / scale)
    print("%s: n %d  max count %d  empty %d  density max |diff| / max |ref| = %.2e" % (
        name, n, int(r["counts"].max()), int((r["counts"] == 0).sum()), err))
    assert bad == 0, "counts differ from the oracle's row lengths at %d points" % bad
    assert_float_close(d, r["density"], RTOL, name + " density")
    return r, h, density, counts


# ------------------------------------------------------------------------------------------------- 1. the window sweep
@pytest.mark.parametrize("name", ["mixed", "mid_windows", "big_windows", "many_centres"])
def test_density_and_counts_on_the_search_geometries(mc, oracle, name):
    """mixed: two clouds, relative radius; mid_windows: windows of 257..512 points (two LDS segments); big_windows: more
    than 512 points per window and rows of more than 1000 hits (up to five segments); many_centres: two clouds, absolute
    radius, 6000 points. Every value is at least the self term, so nothing cancels."""
    g = geo.GEOMETRIES[name]()
    r, h, density, counts = _check_density(mc, oracle, name, g["pts"], g["bids"], g["B"], g["radius"], g["scaleInv"])
    assert r["counts"].min() >= 1 and float(r["density"].min()) >= SELF_TERM * (1 - 1e-6)
    if name == "big_windows":
        assert r["counts"].max() > 1000
    if name == "mid_windows":
        assert r["counts"].max() > 200


@pytest.mark.parametrize("n,radius,scaleInv", [(8201, 0.08, False), (16390, 0.0625, True), (32771, 0.05, False)])
def test_every_group_size(mc, oracle, n, radius, scaleInv):
    """Levels of 8192 / 16384 / 32768 points and more put 2 / 4 / 8 consecutive points on a wave (smaller ones: one); each
    N here leaves the last wave's group part empty, and the members of a wave fall into several cells."""
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3), dtype=np.float32)
    bids = np.zeros((n, 1), np.int32)
    r, *_ = _check_density(mc, oracle, "group_%d" % n, pts, bids, 1, radius, scaleInv)
    assert 8 <= r["counts"].mean() <= 40


# ------------------------------------------------------------------------------------------------- 2. the reference's kernel
@pytest.mark.parametrize("radius,scaleInv", [(0.1, False), (2.0, True)])
def test_expansion_equals_the_oracles_compute_pdf_inside_the_ball(mc, oracle, radius, scaleInv):
    """Clouds inside every one of their balls: expand_pdf(compute_pdf_points) over the points' own list IS compute_pdf. The
    one-point cloud under the relative radius has zero extent: R = 0, counts 0, density 0 and no edge."""
    pts, bids, B, sizes = ref.small_clouds()
    r, h, density, counts = _check_density(mc, oracle, "small_%s" % scaleInv, pts, bids, B, radius, scaleInv)
    start, packed = ref.point_rows(oracle, r["sP"], r["sB"], r["cells"], r["mn"], r["mx"], radius, B, scaleInv)
    exp = oracle.compute_pdf(r["sP"], r["sB"], r["mn"], r["mx"], start, packed, WINDOW, radius, B, scaleInv)
    b = np.asarray(r["sB"]).reshape(-1)
    want = np.asarray(sizes)[b]
    if scaleInv:
        want = np.where(want == 1, 0, want)
        assert float(_unwrap(density)[b == 1, 0][0]) == 0.0
    assert np.array_equal(_unwrap(counts).reshape(-1), want) and len(packed) == int(want.sum())
    st, pk = mc.find_neighbors(h["sP"], h["sB"], h["sP"], h["cells"], h["mn"], h["mx"], radius, B, scaleInv)
    assert np.array_equal(_unwrap(st), start) and np.array_equal(_unwrap(pk), packed)
    pdfs = mc.expand_pdf(density, st, pk)
    assert pdfs.shape == (len(packed), 1)
    assert_float_close(_unwrap(pdfs), exp, RTOL, "expand_pdf(compute_pdf_points) vs the oracle's compute_pdf")


# ------------------------------------------------------------------------------------------------- 3. degenerate inputs
def test_a_batch_id_without_points(mc, oracle):
    rng = np.random.default_rng(7)
    pts = np.concatenate([rng.random((150, 3), dtype=np.float32), rng.random((90, 3), dtype=np.float32) + np.float32(0.5)])
    bids = np.concatenate([np.zeros((150, 1), np.int32), np.full((90, 1), 2, np.int32)])
    for scaleInv in (True, False):
        _check_density(mc, oracle, "gap_%s" % scaleInv, pts, bids, 3, 0.3, scaleInv)


def test_a_single_point(mc, oracle):
    pts, bids = np.asarray([[0.25, 0.5, 0.75]], np.float32), np.zeros((1, 1), np.int32)
    r, h, density, counts = _check_density(mc, oracle, "one_abs", pts, bids, 1, 0.1, False)
    assert int(_unwrap(counts)[0, 0]) == 1 and abs(float(_unwrap(density)[0, 0]) / SELF_TERM - 1) <= RTOL
    r, h, density, counts = _check_density(mc, oracle, "one_rel", pts, bids, 1, 0.1, True)      # zero extent: R = 0
    assert int(_unwrap(counts)[0, 0]) == 0 and float(_unwrap(density)[0, 0]) == 0.0


def test_coincident_points(mc, oracle):
    """200 points in one place (a second cloud gives the batch's box an extent): every ball holds all 200 at distance 0."""
    rng = np.random.default_rng(9)
    pts = np.concatenate([np.full((200, 3), 0.5, np.float32), rng.random((5, 3), dtype=np.float32) + np.float32(1.0)])
    bids = np.concatenate([np.zeros((200, 1), np.int32), np.ones((5, 1), np.int32)])
    r, h, density, counts = _check_density(mc, oracle, "coincident", pts, bids, 2, 0.1, False)
    own = _unwrap(h["sB"]).reshape(-1) == 0
    assert own.sum() == 200 and np.all(_unwrap(counts).reshape(-1)[own] == 200)
    assert_float_close(_unwrap(density)[own], np.full((200, 1), 200 * SELF_TERM), RTOL, "200 self terms")


# ------------------------------------------------------------------------------------------------- 4. reproducible
def test_two_runs_give_the_same_bytes(mc, oracle):
    g = geo.GEOMETRIES["big_windows"]()
    h = _gpu_grid(mc, g["pts"], g["bids"], g["B"], g["radius"], g["scaleInv"])
    run = lambda: mc.compute_pdf_points(h["sP"], h["sB"], h["cells"], h["mn"], h["mx"], WINDOW, g["radius"], g["B"], g["scaleInv"])
    (d0, c0), (d1, c1) = run(), run()
    assert _unwrap(d0).tobytes() == _unwrap(d1).tobytes() and _unwrap(c0).tobytes() == _unwrap(c1).tobytes()


# ------------------------------------------------------------------------------------------------- 5. the expansion
def test_expand_pdf_bit_for_bit(mc, oracle):
    """A list whose centres are not the points: `mixed`, 1020 centres, the last 20 out of reach (empty rows)."""
    import torch
    g = geo.GEOMETRIES["mixed"]()
    r = _reference(oracle, "mixed", g["pts"], g["bids"], g["B"], g["radius"], g["scaleInv"])
    start, packed = oracle.find_neighbors(g["centres"], g["cbids"], r["sP"], r["cells"], r["mn"], r["mx"], g["radius"], g["B"],
                                          g["scaleInv"])
    k = ref.row_lengths(start, len(packed))
    assert len(k) == 1020 and (k[-20:] == 0).all() and len(packed) > 0
    density = r["density"].astype(np.float32)
    exp = ref.expand_ref(density, start, packed)
    got = mc.expand_pdf(_wrap(density), _wrap(start), _wrap(packed))
    assert got.shape == (len(packed), 1) and got.dtype == torch.float32
    assert _unwrap(got).tobytes() == exp.tobytes()
    # E = 0: every centre out of reach
    far = np.full((4, 3), 9.0, np.float32)
    st0, pk0 = oracle.find_neighbors(far, np.zeros((4, 1), np.int32), r["sP"], r["cells"], r["mn"], r["mx"], g["radius"], g["B"],
                                     g["scaleInv"])
    assert len(pk0) == 0
    got0 = mc.expand_pdf(_wrap(density), _wrap(st0), _wrap(np.asarray(pk0, np.int32).reshape(0, 2)))
    assert got0.shape == (0, 1) and got0.dtype == torch.float32


# ------------------------------------------------------------------------------------------------- 6. the builder
def _graph(MB, cb, ph, F, **kw):
    """Same level (2 -> 8 features), pooling to level 1 and upsampling back (depth-wise, 8 features)."""
    a = cb.create_convolution("Same", ph, 0, F, 2, 0.2, outNumFeatures=8, multiFeatureConv=True, **kw)
    b = cb.create_convolution("Pool", ph, 0, a, 8, 0.3, outPointLevel=1, **kw)
    return cb.create_convolution("Up", ph, 1, b, 8, 0.3, outPointLevel=0, **kw)


def test_builder_end_to_end(mc, oracle):
    import torch
    import mccnn_amd.MCConvBuilder as MB
    from tests.helpers import make_cloud
    B = 2
    pts, bids = make_cloud(512, B, 21, "clustered")
    rng = np.random.default_rng(22)
    feats = (2 * rng.random((len(pts), 2)) - 1).astype(np.float32)
    og = (2 * rng.random((len(pts), 8)) - 1).astype(np.float32)
    torch.manual_seed(4)
    dev = torch.device("cuda", 0)
    res = {}
    ops = ref.PointPdfOracleOps(oracle)
    gb = MB.ConvolutionBuilder(KDEWindow=WINDOW, pdfMode='point')
    cbuild = MB.ConvolutionBuilder(KDEWindow=WINDOW, pdfMode='point', ops=ops)
    for tag, cb, dv, kw in (("gpu", gb, dev, {}), ("cpu", cbuild, torch.device("cpu"), {"ops": ops})):
        P, Bi = torch.from_numpy(pts).to(dv), torch.from_numpy(bids).to(dv)
        F = torch.from_numpy(feats).to(dv).requires_grad_(True)
        ph = MB.PointHierarchy(P, F, Bi, [0.1], "PH", B, **kw)
        if tag == "cpu":
            cb.load_state_dict({k: v.detach().cpu().clone() for k, v in gb.state_dict().items()})
        cb.opTrace_ = []
        out = _graph(MB, cb, ph, F)
        out.backward(torch.from_numpy(og).to(dv))
        res[tag] = (out.detach().cpu().numpy(), F.grad.detach().cpu().numpy(),
                    {k: v.grad.detach().cpu().numpy() for k, v in cb.named_parameters()}, list(cb.opTrace_),
                    [int(p.shape[0]) for p in ph.points_])
    (go, gf, gw, gtr, gsz), (co, cf, cw, ctr, csz) = res["gpu"], res["cpu"]
    assert gsz == csz and gsz[0] == len(pts) and 1 < gsz[1] < len(pts)
    pick = lambda tr: [r for r in tr if r[0] in ("compute_pdf_points", "expand_pdf", "compute_pdf")]
    assert pick(gtr) == pick(ctr) and [r[0] for r in pick(gtr)] == ["compute_pdf_points", "expand_pdf", "compute_pdf_points",
                                                                   "expand_pdf", "compute_pdf_points", "expand_pdf"]
    assert not gb.cacheGeo_ and len(gb.cachePointPDFs_) == 3, "a 'point' layer takes the op-by-op path"
    assert_float_close(go, co, RTOL, "output")
    assert_float_close(gf, cf, RTOL, "feature gradient")
    assert set(gw) == set(cw) and len(gw) == 18
    for k in sorted(cw):
        assert_float_close(gw[k], cw[k], RTOL, k)
    # an 'edge' layer inside the 'point' builder: the default builder's bytes (both take the native executor for it); the
    # 'point' graph over the grid and list that geometry owns still agrees with the oracle's
    P, Bi, F = torch.from_numpy(pts).to(dev), torch.from_numpy(bids).to(dev), torch.from_numpy(feats).to(dev)
    ph = MB.PointHierarchy(P, F, Bi, [0.1], "PH", B)
    db = MB.ConvolutionBuilder(KDEWindow=WINDOW)
    db.load_state_dict({k: v.detach().clone() for k, v in gb.state_dict().items()})
    gb.reset()
    with torch.no_grad():
        want = db.create_convolution("Same", ph, 0, F, 2, 0.2, outNumFeatures=8, multiFeatureConv=True)
        got = gb.create_convolution("Same", ph, 0, F, 2, 0.2, outNumFeatures=8, multiFeatureConv=True, pdfMode='edge')
        assert _unwrap(got).tobytes() == _unwrap(want).tobytes()
        again = _graph(MB, gb, ph, F)
    assert "PH|0|0.2|True|PH|0|0.25|True" in gb.cachePDFs_ and "PH|0|0.2|True|PH|0|0.25|True|pt" in gb.cachePDFs_
    assert_float_close(_unwrap(again), co, RTOL, "output over a native geometry's grid and list")
