"""Combining layers (combin=True) across every (Fin, Fout) route of csrc/conv.hip: the lattice of tests/combin_cases.py (each
case's comment names the kernel line it exists for) on the op surface (MCConvModule.spatial_conv with the oracle's PDFs, so
that the convolution alone is compared) and on the native step executor, against the CPU oracle at RTOL = 1e-4 norm-wise and
per element (tests/helpers.py::assert_float_close). tests/test_oracle_combin_cpu.py pins the oracle at the same shapes
against float64 autograd of the definition.

Geometries (built once per session, the oracle's values cached per (geometry, shape)):
  A  the parity cloud make_cloud(1500, 2, 21, "clustered", True), radius 0.15 relative, avg: 1 878 points, 155 372 edges, the
     longest row 183 > 64 (rows cross the 64-edge chunks: carry in the forward scan), ~2 400 chunks (many waves and partial rows)
  P  the pooling geometry of tests/test_gpu_conv_alignment.py (combin_cases.pooling_cloud): 909 points, 300 centres, 21 946
     edges, 6 centres without neighbours, 38 points nobody reaches. n = 909: n * Fin * 4 % 16 is 0 for Fin = 4, 16 and not for
     Fin = 2, 3, 7, 9, so both ways of clearing feat_grad occur (a ClearSpan inside reduce_partials / a launch_zero_words)
  W  make_cloud(150, 2, 22, "clustered", True), radius 0.3: 159 points, 1 887 edges, for the layers of 50..65 blocks
  E  make_cloud(600, 2, 21, "clustered", True), radius 0.15: 1 086 points, 42 392 edges, longest row 82 (native executor)

Which kernels a case runs is decided by constants alone (combin_cases.py has them): Fin = 1 -> conv_f1.hip while nb <= 64;
Fin = 2..4 -> <true, 3, false>, per-block planes while nb <= 4; Fin > 4 -> <true, 0, false>. THE BACKWARD ROUTE OF THE WIDE
LAYERS IS NOT OBSERVABLE from outside; it follows from conv_bwd_impl: `lds = (nb * MCCNN_WQ_BWD + 4 * 192) * 4`,
`mfma = use_mfma(...) && lds <= 64 * 1024`: 65 472 bytes at nb = 50 (MFMA sweep / f1_backward), 66 720 at nb = 51
(conv_bwd_valu, behind a forward that is still conv_stream / f1_forward and still writes the state records: what
mccnn_spatial_conv_state_bytes > 0 shows, asserted below up to nb = 64, and 0 at 65).
The feature gradient of Fin = 2..4 has two forms: float atomics (scatter_edge_featgrad; the list object carries no transposed
list) and a gather over the transposed list (gather_edge_featgrad<Fin>; MCConvModule._transposed_neighbors was called on the
list object). Both are run explicitly, on two copies of the list.
Nine shapes of the lattice are refused by the reference's shape rule (8 * nb % Fin != 0, combin_cases.py "THE SHAPE RULE"): for
those the test asserts the refusal, and the accepted shape next to each in the table runs the kernel lines it was meant for.

Every call runs with NaNs (all bits set) in the blocks its outputs are about to receive AND in the library's scratch pool
(per-edge planes, partial rows, records): found necessary by mutation -- with `a.nb <= MCCNN_DF_PLANES` turned into `<` in
conv_bwd_mfma alone (host side unchanged) the sums of 2 -> 16 and 4 -> 8 came out right as long as the planes nobody wrote
happened to hold zeros. Mutants tried (each fails cases here and none of the combining cases the suite had before):
`(q == f / 8) ? 0.f : old` -> `(q == 0)`: 9 -> 8, 12 -> 2, 16 -> 3, 20 -> 2; `sfg = fmaf(g[n], o[n], sfg)` -> `sfg = g[n] * o[n]`
(the fold): 5 -> 7, 6 -> 3, 7 -> 7, 5 -> 80 (not 6 -> 67: its backward is conv_bwd_valu, as the constants say); acc cleared at
every block of conv_stream<true, 0, false>: every Fin > 4 shape but 8 -> 1 / 8 -> 64; the planes test above: 2 -> 16, 4 -> 8.

MEASURED on an MI355X: see MEASURED below.
"""
import numpy as np
import pytest

from tests import combin_cases as cc
from tests.helpers import make_cloud, make_mlp, conv_nb, run_chain, assert_float_close

pytestmark = pytest.mark.gpu

RTOL = 1e-4
GPU_TOL = 2e-5     # two GPU implementations that share every pre-activation (tests/test_gpu_parity.py::test_spatial_conv_fwd_bwd)
NAMES = ["out", "featGrad", "dw1", "db1", "dw2", "db2", "dw3", "db3"]

MEASURED = """
MI355X, one run of the whole suite. 56 tests, 7 to 9 seconds together: the first one ~3 s (geometry A, the library's first
call), every other one under 0.3 s (the oracle takes ~0.1 s per shape on A). Geometries as asserted: A 1 878 points / 155 372
edges / longest row 183; W 159 / 1 887 / 31; P 909 points, 300 centres, 21 946 edges, longest row 157, 6 empty rows, 38
unreached points; E 1 086 / 42 392 / 82.
Worst max|diff| / max|ref| over the cases of each column (28 accepted shapes in a; the nine refused ones raise):

              a. lattice (A, W)                              b. forms (A)                    c. rows (P)  d. offset (P)          e. native (E)
              vs oracle  no state   vs VALU    Fin = 1 vs    scatter    gather     gather    vs oracle    vs oracle  offset     vs oracle graph
                         vs state   kernels    general MFMA  vs oracle  vs oracle  vs scatter                         vs aligned
    out       2.5e-6     0 (bits)   3.0e-7     2.0e-7        1.2e-6     1.2e-6     0 (bits)  1.6e-6       8.1e-7     0 (bits)   2.2e-6
    featGrad  2.9e-6     6.7e-7     1.9e-6     8.6e-7        1.2e-6     1.2e-6     3.3e-7    8.2e-7       7.3e-7     3.3e-7     1.0e-6
    dw1       4.7e-7     0 (bits)   4.7e-7     1.9e-7        3.1e-7     3.1e-7     0 (bits)  2.6e-7       2.2e-7     0 (bits)   1.3e-6
    db1       3.7e-7     0 (bits)   4.3e-7     1.7e-7        3.7e-7     3.7e-7     0 (bits)  3.9e-7       2.5e-7     0 (bits)   9.6e-7
    dw2       3.4e-7     0 (bits)   3.1e-7     1.7e-7        2.2e-7     2.2e-7     0 (bits)  3.3e-7       3.3e-7     0 (bits)   1.1e-6
    db2       3.5e-7     0 (bits)   3.8e-7     1.2e-7        3.5e-7     3.5e-7     0 (bits)  3.5e-7       3.3e-7     0 (bits)   9.6e-7
    dw3       4.6e-7     0 (bits)   5.2e-7     9.5e-8        3.1e-7     3.1e-7     0 (bits)  2.7e-7       1.8e-7     0 (bits)   1.2e-6
    db3       4.3e-7     0 (bits)   4.7e-7     1.6e-7        4.3e-7     4.3e-7     0 (bits)  3.4e-7       3.4e-7     0 (bits)   9.6e-7

"vs oracle" of a covers every variant run there (state kept / not kept, gather, VALU, general MFMA). The feature gradient is the
one tensor that differs between runs of one form (float atomics: scatter_edge_featgrad, and the Fin = 1 / Fin > 4 edge sums);
the gathered one is bit-identical over two runs, and the six parameter gradients are bit-identical between the scatter and the
gather form and between a backward pass that reads the forward's records and one that recomputes them (asserted in b; observed
in a and d). The native executor evaluates its own single-precision KDE: hence ~1e-6 there.
Oracle against float64 at these shapes: tests/test_oracle_combin_cpu.py (worst 2.7e-6, 6 % of the per-element band).
"""

_GEO, _REF = {}, {}
ident = lambda a: a


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """The NaN blocks of _run leave cached blocks of many odd sizes in torch's allocator, and a later module measures what a
    layer holds with torch.cuda.memory_allocated() (tests/test_gpu_f1_recin.py: a cached block a little larger than a request
    is handed out whole and counted whole -- it came out 46 KB off behind this module). Drop this module's tensors and the
    cache when it is done."""
    yield
    import torch
    _GEO.clear()
    _REF.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.detach().float().cpu().numpy()


def _geo(oracle, which):
    """the oracle's chain on geometry `which`, its structural facts, and the device copies the GPU calls read"""
    if which in _GEO:
        return _GEO[which]
    centres = cb = None
    if which == "A":
        pts, bids, B, radius, scaleInv = cc.cloud_A()
    elif which == "W":
        pts, bids, B, radius, scaleInv = cc.cloud_W()
    else:
        pts, bids, centres, cb, _ = cc.pooling_cloud()
        B, radius, scaleInv = 1, 0.2, False
    o = run_chain(oracle, ident, ident, pts, bids, np.zeros((len(pts), 1), np.float32), B, radius, scaleInv, fout=1,
                  centres=centres, centre_bids=cb)
    C = pts if centres is None else centres
    n, m, e = len(pts), len(C), len(o["packedNeighs"])
    deg = np.diff(np.append(o["startIndexs"].reshape(-1), e))
    tdeg = np.bincount(o["packedNeighs"][:, 0], minlength=n)
    facts = (n, m, e, int(deg.max()), int((deg == 0).sum()), int((tdeg == 0).sum()))
    print("geometry %s: n, m, e, longest row, empty rows, unreached points = %s" % (which, facts))
    assert facts == {"A": (1878, 1878, 155372, 183, 0, 0), "W": (159, 159, 1887, 31, 0, 0), "P": (909, 300, 21946, 157, 6, 38)}[which]
    if which != "W":
        assert deg.max() > 64 and e > 4 * 64     # rows longer than a 64-edge chunk, several waves
    G = dict(which=which, o=o, C=C, B=B, radius=radius, scaleInv=scaleInv, n=n, m=m, e=e, deg=deg, tdeg=tdeg)
    _GEO[which] = G
    return G


def _dev(mc, G):
    """device tensors of the geometry; the neighbour list twice: `packed` never gets a transposed list (atomics),
    `packed_t` carries one (gather)"""
    if "dev" not in G:
        o = G["o"]
        D = {k: _t(o[s]) for k, s in (("sP", "sortPts"), ("sB", "sortBatchs"), ("pdfs", "pdfs"), ("start", "startIndexs"),
                                       ("packed", "packedNeighs"), ("mn", "aabbMin"), ("mx", "aabbMax"))}
        D["C"] = _t(G["C"])
        D["packed_t"] = D["packed"].clone()
        mc._transposed_neighbors(D["packed_t"], G["n"])
        G["dev"] = D
    return G["dev"]


def _ref(oracle, G, fin, fout):
    """features, out-gradient, kernel MLP and the oracle's output and seven gradients for one shape on one geometry"""
    key = (G["which"], fin, fout)
    if key not in _REF:
        o = G["o"]
        feats, og = cc.layer_inputs(G["n"], G["m"], fin, fout)
        w = make_mlp(conv_nb(fin, fout, True), 7)
        args = (o["sortPts"], feats, o["sortBatchs"], o["pdfs"], G["C"], o["startIndexs"], o["packedNeighs"], o["aabbMin"],
                o["aabbMax"], w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
        out = oracle.spatial_conv(*args, fout, True, G["B"], G["radius"], G["scaleInv"], True)
        grads = oracle.spatial_conv_grad(*args, og, fout, True, G["B"], G["radius"], G["scaleInv"], True)
        _REF[key] = dict(feats=feats, og=og, w=w, want=[np.asarray(out)] + [np.asarray(g) for g in grads])
    return _REF[key]


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device="cuda")


def _ws_poison(mc, nbytes):
    """all bits set in every scratch buffer of the library's pool, and in a block of the size the pool would allocate next"""
    import torch
    for buf in list(mc._WS_POOL.values()):
        buf.fill_(255)
    nbytes = max(int(nbytes), 256)
    return torch.full((nbytes + nbytes // 4,), 255, dtype=torch.uint8, device="cuda")


def _run(mc, G, R, fin, fout, state=True, impl=0, gather=False, feats=None, og=None):
    """MCConvModule.spatial_conv forward + the seven gradients -> [out, featGrad, dw1, db1, dw2, db2, dw3, db3]. The blocks the
    op's torch.empty() calls are about to receive held NaNs: a row, a padded neuron or a plane nobody writes shows."""
    import torch
    from mccnn_amd import _lib
    D = _dev(mc, G)
    packed = D["packed_t"] if gather else D["packed"]
    assert (getattr(packed, "_mccnn_transposed", None) is not None) == gather
    n, m, e, nn = G["n"], G["m"], G["e"], 8 * conv_nb(fin, fout, True)
    tw = {k: _t(v).requires_grad_(True) for k, v in R["w"].items()}
    F = (_t(R["feats"]) if feats is None else feats).requires_grad_(True)
    g = _t(R["og"]) if og is None else og
    mc.KEEP_CONV_STATE = state
    mc.debug_conv_impl(impl)
    lib = _lib.load()
    try:
        # the library's scratch memory (per-edge planes, partial rows, records) is a grow-only pool that keeps what the last
        # call left: all bits set (a NaN as float, -1 as int) before either pass, so that a plane or a row a kernel reads
        # without having written it shows whatever ran before. (The pool is per host thread, and autograd runs the backward
        # pass on a thread of its own: every buffer there is gets filled, and a buffer that is about to be made or to grow
        # takes, as far as the allocator can be steered, a block that held the same bits.)
        junk = [_nan(m, fout), _nan(n, fin), _ws_poison(mc, lib.mccnn_spatial_conv_fwd_workspace_bytes(m, e, fin, fout, 1))]
        torch.cuda.synchronize()
        del junk
        out = mc.spatial_conv(D["sP"], F, D["sB"], D["pdfs"], D["C"], D["start"], packed, D["mn"], D["mx"], tw["w1"], tw["w2"],
                              tw["w3"], tw["b1"], tw["b2"], tw["b3"], fout, True, G["B"], G["radius"], G["scaleInv"], True)
        junk = [_nan(n, fin), _nan(22 * nn), _nan(m, fout),     # (22 nn: the six parameter gradients are one buffer)
                _ws_poison(mc, lib.mccnn_spatial_conv_bwd_workspace_bytes(n, m, e, fin, fout, 1))]
        torch.cuda.synchronize()
        del junk
        grads = torch.autograd.grad([out], [F, tw["w1"], tw["b1"], tw["w2"], tw["b2"], tw["w3"], tw["b3"]], [g])
        torch.cuda.synchronize()
    finally:
        mc.KEEP_CONV_STATE = True
        mc.debug_conv_impl(0)
    assert (getattr(packed, "_mccnn_transposed", None) is not None) == gather
    return [out.detach()] + [x.detach() for x in grads]


def _flat(nm, a):
    a = a if isinstance(a, np.ndarray) else _np(a)
    return a if nm in ("out", "featGrad") else a.reshape(-1)


def _against(got, want, tol, what, errs, col):
    """all eight tensors of `got` against `want` (norm-wise and per element); the worst figures per column go to errs"""
    for nm, a, b in zip(NAMES, got, want):
        a, b = _flat(nm, a), _flat(nm, b)
        assert np.isfinite(a).all(), "%s: %s is not finite" % (what, nm)
        e = float(np.abs(a.astype(np.float64) - b).max() / max(float(np.abs(b).max()), 1e-30))
        errs[(col, nm)] = max(errs.get((col, nm), 0.0), e)
        assert_float_close(a, b, tol, "%s: %s" % (what, nm))


def _padding_is_zero(got, fin, fout, what):
    """padded output neurons: the library writes zeros (the reference leaves them uninitialised)"""
    neurons = fin * fout
    dw3, db3 = _np(got[6]).reshape(-1), _np(got[7]).reshape(-1)
    assert np.all(dw3[neurons * 8:] == 0), what + ": dw3 of a padded neuron is not zero"
    assert np.all(db3[neurons:] == 0), what + ": db3 of a padded neuron is not zero"


def _report(tag, case, errs):
    print("LATTICE %s %s: %s" % (tag, cc.case_id(case), " ".join("%s/%s=%.1e" % (c, nm, v) for (c, nm), v in sorted(errs.items()))))


# ------------------------------------------------------------------------------------------------- a. the lattice
@pytest.mark.parametrize("case", cc.LATTICE, ids=[cc.case_id(c) for c in cc.LATTICE])
def test_lattice_against_the_oracle(mc, oracle, case):
    """Every shape of the table on geometry A (W for the wide ones): the default kernels with and without the forward's state
    (KEEP_CONV_STATE: records reused / recomputed by the backward pass), Fin = 2..4 in both forms of the feature gradient,
    against the oracle at 1e-4; against the VALU kernels (debug_conv_impl(1)) and, for Fin = 1, the general MFMA kernels
    (mask 2) at 2e-5; padded neurons exactly zero. The state bytes show which forward a wide layer took."""
    from mccnn_amd import _lib
    fin, fout, nb, _last, _r0, _why, which = case
    cc.check_table()
    G = _geo(oracle, which)
    what = cc.case_id(case)
    if not cc.accepted(case):
        # the reference's shape rule (spatial_conv.cc:290): 8 * nb is no multiple of Fin. The op refuses the layer before
        # anything is launched (the C ABI too: tests/test_oracle_combin_cpu.py); combin_cases.py names the accepted shape
        # that runs the kernel lines this one was meant for.
        feats, og = cc.layer_inputs(G["n"], G["m"], fin, fout)
        with pytest.raises(mc.InvalidArgumentError, match="multiple of the number of features"):
            _run(mc, G, dict(feats=feats, og=og, w=make_mlp(nb, 7)), fin, fout)
        return
    R = _ref(oracle, G, fin, fout)
    sbytes = _lib.load().mccnn_spatial_conv_state_bytes(G["m"], G["e"], fin, fout, 1)
    assert (sbytes > 0) == (nb <= cc.LDS_MAX_NB), (what, sbytes)
    assert sbytes == 0 or sbytes >= 16 * G["e"]        # one record per edge
    errs = {}
    kept = _run(mc, G, R, fin, fout, state=True)
    _against(kept, R["want"], RTOL, what + " (state kept)", errs, "oracle")
    _padding_is_zero(kept, fin, fout, what + " (state kept)")
    redone = _run(mc, G, R, fin, fout, state=False)
    _against(redone, R["want"], RTOL, what + " (no state)", errs, "oracle")
    _padding_is_zero(redone, fin, fout, what + " (no state)")
    _against(redone, [_np(x) for x in kept], GPU_TOL, what + " no state vs state", errs, "nostate")
    if 2 <= fin <= 4:
        gath = _run(mc, G, R, fin, fout, gather=True)
        _against(gath, R["want"], RTOL, what + " (gather)", errs, "oracle")
        _padding_is_zero(gath, fin, fout, what + " (gather)")
    for mask, label in [(1, "valu")] + ([(2, "general")] if fin == 1 else []):
        other = _run(mc, G, R, fin, fout, impl=mask)
        _against(other, R["want"], RTOL, "%s (%s kernels)" % (what, label), errs, "oracle")
        _padding_is_zero(other, fin, fout, "%s (%s kernels)" % (what, label))
        _against(kept, [_np(x) for x in other], GPU_TOL, "%s default vs %s kernels" % (what, label), errs, label)
    _report("a", case, errs)


# ------------------------------------------------------------------------------------------------- b. gather against scatter
# (Fin = 3 has no accepted shape of 4 or 5 blocks: 3 -> 7 has 3, 3 -> 15 has 6)
FORMS = [c for c in cc.LATTICE if c[:2] in ((2, 16), (2, 17), (3, 7), (3, 15), (4, 8), (4, 11))]


@pytest.mark.parametrize("case", FORMS, ids=[cc.case_id(c) for c in FORMS])
def test_feature_gradient_gather_against_scatter(mc, oracle, case):
    """Fin = 2..4, one plane-form (nb <= 4) and one read-modify-write shape (nb > 4) each: the backward pass without a transposed
    list (float atomics) and with one (gather). Both feature gradients against the oracle; the gather bit-identical over two
    runs; the six parameter gradients bit-identical between the forms (the same sweep and reduce_partials, fixed order)."""
    import torch
    fin, fout, nb, _last, _r0, _why, _w = case
    assert len(FORMS) == 6 and (nb <= cc.DF_PLANES) == (fout in (16, 7, 8)) and cc.accepted(case)
    G = _geo(oracle, "A")
    R = _ref(oracle, G, fin, fout)
    what = cc.case_id(case)
    errs = {}
    sc = _run(mc, G, R, fin, fout, gather=False)
    ga = _run(mc, G, R, fin, fout, gather=True)
    ga2 = _run(mc, G, R, fin, fout, gather=True)
    _against(sc, R["want"], RTOL, what + " scatter", errs, "scatter:oracle")
    _against(ga, R["want"], RTOL, what + " gather", errs, "gather:oracle")
    _against(ga, [_np(x) for x in sc], GPU_TOL, what + " gather vs scatter", errs, "gather:scatter")
    assert torch.equal(ga[1], ga2[1]), what + ": the gathered feature gradient differs between two runs"
    assert torch.equal(ga[0], sc[0]) and torch.equal(ga[0], ga2[0]), what + ": the forward pass differs between runs"
    for nm, a, b, c in zip(NAMES[2:], sc[2:], ga[2:], ga2[2:]):
        assert torch.equal(a, b) and torch.equal(b, c), "%s: %s differs between the scatter and the gather form" % (what, nm)
    _report("b", case, errs)


# ------------------------------------------------------------------------------------------------- c. rows nobody writes
ROWS = [c for c in cc.LATTICE if c[:2] in ((2, 17), (3, 7), (4, 12), (7, 7), (9, 8), (16, 3))]


@pytest.mark.parametrize("case", ROWS, ids=[cc.case_id(c) for c in ROWS])
def test_rows_nobody_writes(mc, oracle, case):
    """The pooling geometry: 6 centres without neighbours (rows without an edge at the start, in the middle and at the end of
    the list), 38 points that are nobody's neighbour, outputs in memory that held NaNs. Such rows must be exactly zero --
    out by conv_stream's zero_rows, feat_grad by the ClearSpan of reduce_partials (n * Fin * 4 % 16 == 0), by
    launch_zero_words (otherwise) or by gather_edge_featgrad's own store of an empty sum."""
    fin, fout, _nb, _last, _r0, _why, _w = case
    G = _geo(oracle, "P")
    R = _ref(oracle, G, fin, fout)
    what = cc.case_id(case) + " pooling"
    span = {c[0]: (G["n"] * c[0] * 4) % 16 == 0 for c in ROWS}
    assert span == {2: False, 3: False, 4: True, 7: False, 9: False, 16: True}     # both clearing routes are in the case set
    assert len(ROWS) == 6 and cc.accepted(case) and (G["deg"] == 0).sum() == 6 and (G["tdeg"] == 0).sum() == 38 and G["m"] != G["n"]
    errs = {}
    for gather in ((False, True) if fin <= 4 else (False,)):
        for state in (True, False):
            got = _run(mc, G, R, fin, fout, state=state, gather=gather)
            w2 = "%s (%s, state %s)" % (what, "gather" if gather else "scatter", state)
            out, fg = _np(got[0]), _np(got[1])
            assert np.isfinite(out).all() and np.isfinite(fg).all(), w2
            assert np.all(out[G["deg"] == 0] == 0), w2 + ": a centre without neighbours has a non-zero row"
            assert np.all(fg[G["tdeg"] == 0] == 0), w2 + ": a point that is nobody's neighbour has a non-zero gradient row"
            _against(got, R["want"], RTOL, w2, errs, "oracle")
            _padding_is_zero(got, fin, fout, w2)
    _report("c", case, errs)


# ------------------------------------------------------------------------------------------------- d. rows off the 16-byte grid
OFFSET = [c for c in cc.LATTICE if c[:2] in ((3, 7), (7, 7))]     # (7 -> 7: the shape rule refuses 7 -> 5)


@pytest.mark.parametrize("which", ["feats", "outgrad", "both"])
@pytest.mark.parametrize("case", OFFSET, ids=[cc.case_id(c) for c in OFFSET])
def test_rows_off_the_16_byte_grid(mc, oracle, case, which):
    """Features, out-gradient or both 4 bytes behind an aligned allocation (contiguous views into a larger buffer). The
    combining kernels load the caller's rows as scalars only (rows of 3 or 7 floats are off the grid anyway, whatever the
    pointer); this shows it stays that way: the same values as on aligned clones at 2e-5, the oracle's at 1e-4."""
    fin, fout, _nb, _last, _r0, _why, _w = case
    G = _geo(oracle, "P")
    R = _ref(oracle, G, fin, fout)
    what = "%s %s +4 B" % (cc.case_id(case), which)
    errs = {}
    for gather in ((False, True) if fin <= 4 else (False,)):
        f_al, g_al = _t(R["feats"]).clone(), _t(R["og"]).clone()
        f_off = cc.off(f_al, 4) if which in ("feats", "both") else f_al.clone()
        g_off = cc.off(g_al, 4) if which in ("outgrad", "both") else g_al.clone()
        assert f_al.data_ptr() % 16 == 0 and g_al.data_ptr() % 16 == 0
        assert (f_off.data_ptr() % 16 == 4) == (which != "outgrad") and (g_off.data_ptr() % 16 == 4) == (which != "feats")
        got = _run(mc, G, R, fin, fout, gather=gather, feats=f_off, og=g_off)
        ref = _run(mc, G, R, fin, fout, gather=gather, feats=f_al, og=g_al)
        _against(got, R["want"], RTOL, what, errs, "oracle")
        _against(ref, R["want"], RTOL, what + " (aligned clone)", errs, "oracle")
        _against(got, [_np(x) for x in ref], GPU_TOL, what + " vs aligned", errs, "aligned")
    _report("d-" + which, case, errs)


# ------------------------------------------------------------------------------------------------- e. the native executor
NATIVE = [c for c in cc.LATTICE if c[:2] in ((2, 17), (3, 7), (7, 7), (16, 3))]     # (7 -> 7: the shape rule refuses 7 -> 5)


def test_native_executor_against_the_oracle_graph(mc, oracle):
    """2 -> 17, 3 -> 7, 7 -> 7 and 16 -> 3 as ONE ConvolutionBuilder(native=True) graph over one geometry (csrc/exec.hip:
    mccnn_conv_forward / mccnn_conv_backward call the same conv_fwd_impl / conv_bwd_impl, with the geometry's transposed
    list) against the identical graph on the oracle ops (tests/oracle_ops.py), as tests/test_gpu_native.py does for 3 -> 8
    and 2 -> 5. The executor evaluates its own single-precision KDE: 1e-4."""
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    from tests.oracle_ops import OracleOps
    assert len(NATIVE) == 4 and all(cc.accepted(c) for c in NATIVE)
    pts, bids = make_cloud(600, 2, 21, "clustered", True)
    B, radius = 2, 0.15
    n = len(pts)
    oo = OracleOps(oracle)
    P, Bi = _t(pts), _t(bids)
    ph = PointHierarchy(P, torch.ones((n, 1), device="cuda"), Bi, [], "PH", B, True)
    phc = PointHierarchy(torch.from_numpy(pts), torch.ones((n, 1)), torch.from_numpy(bids), [], "PH", B, True, ops=oo)
    torch.manual_seed(5)
    cb = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, native=True)
    cbc = ConvolutionBuilder(KDEWindow=0.25, relativeRadius=True, ops=oo)
    cb.reset()
    cbc.reset()
    assert cb.native_
    rng = np.random.default_rng(3)
    outs, outcs, ins, incs, pars, parcs, ogs = [], [], [], [], [], [], []
    for case in NATIVE:
        fin, fout = case[:2]
        name = "L" + cc.case_id(case)
        f = (2 * rng.random((n, fin)) - 1).astype(np.float32)
        ogs.append((2 * rng.random((n, fout)) - 1).astype(np.float32))
        F = _t(f).requires_grad_(True)
        outs.append(cb.create_convolution(name, ph, 0, F, fin, radius, ph, 0, True, fout))
        names = [name + s for s in ("_weights", "_biases", "_weights2", "_biases2", "_weights3", "_biases3")]
        gp = dict(cb.named_parameters())
        cbc.load_state_dict({k: gp[k].detach().cpu().clone() for k in names}, strict=False)
        Fc = torch.from_numpy(f).requires_grad_(True)
        outcs.append(cbc.create_convolution(name, phc, 0, Fc, fin, radius, phc, 0, True, fout))
        cp = dict(cbc.named_parameters())
        ins.append(F)
        incs.append(Fc)
        pars.append([gp[k] for k in names])
        parcs.append([cp[k] for k in names])
    assert len(cb.cacheGeo_) == 1, "the four layers did not share one native geometry"
    flat = lambda ll: [x for l in ll for x in l]
    g_gpu = torch.autograd.grad(outs, ins + flat(pars), [_t(g) for g in ogs])
    g_cpu = torch.autograd.grad(outcs, incs + flat(parcs), [torch.from_numpy(g) for g in ogs])
    torch.cuda.synchronize()
    (st, pk), (stc, pkc) = next(iter(cb.cacheNeighs_.values())), next(iter(cbc.cacheNeighs_.values()))
    assert np.array_equal(st.cpu().numpy(), stc.numpy()) and np.array_equal(pk.cpu().numpy(), pkc.numpy())
    e = pk.shape[0]
    deg = np.diff(np.append(stc.numpy().reshape(-1), e))
    print("geometry E: n, e, longest row = %s" % ((n, e, int(deg.max())),))
    assert (n, e, int(deg.max())) == (1086, 42392, 82) and deg.max() > 64 and e > 4 * 64
    L = len(NATIVE)
    for k, case in enumerate(NATIVE):
        errs = {}
        # NAMES order: out, featGrad, dw1 (weights), db1 (biases), dw2, db2, dw3, db3 = the builder's variable order
        got = [outs[k], g_gpu[k]] + list(g_gpu[L + 6 * k:L + 6 * k + 6])
        want = [outcs[k], g_cpu[k]] + list(g_cpu[L + 6 * k:L + 6 * k + 6])
        _against(got, [_np(x) for x in want], RTOL, "native " + cc.case_id(case), errs, "native")
        _padding_is_zero(got, case[0], case[1], "native " + cc.case_id(case))
        _report("e", case, errs)
