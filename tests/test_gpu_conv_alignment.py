"""Depth-wise convolutions whose feature rows or out-gradient do not start on a 16-byte boundary (contiguous views into a
larger buffer), on both surfaces: the Python ops (MCConvModule.spatial_conv, sorted rows and the sortIndex / featIndex form)
and the native step executor (ConvolutionBuilder(native=True), csrc/exec.hip behind csrc/torch_ext.cpp).

What decides the route (every 16-byte access to a caller's pointer sits behind one of these checks of the pointer's low bits):

  f32, 16 features (Fin % 8 == 0, so only the POINTER takes the layer off the vector path):
    * the row-per-lane kernels want aligned rows and out-gradients: MCConvModule._rows_shape / `rows_bwd`, exec.hip
      rows_shape / fwd_mode (`unsorted`) / mccnn_conv_backward (`rows_bwd`), and once more in conv_rows.hip rows_shape_ok;
    * the edge-streaming kernels pick their instantiation in conv.hip: vec = !combin && Fin % 8 == 0 && (feats | outGrad)
      & 15 == 0 (conv_fwd_impl: feats alone; conv_bwd_impl: both), vecD = Fin % 8 == 0 && outGrad & 15 == 0. A misaligned
      pointer => vec == false => conv_stream<false, 0, false> (forward), conv_bwd_mfma<false, 0, coop> (parameter
      gradients) and, for a misaligned out-gradient, conv_stream<false, 0, true> (feature gradient over the transposed
      list): scalar gathers of the caller's rows; outputs go to fresh allocations and keep their float4 stores;
    * the row permutations (grid.hip launch_permute) take float4 / float2 / scalar moves by the pointers' low bits.
    Offset features with sortIndex: the op sorts them into a fresh buffer, and the row kernels run on that. Aligned
    features + offset out-gradient with featIndex on a small level: the forward pass read the UNSORTED rows in place, the
    backward pass leaves the row kernels and sorts the rows after all (MCConvModule._feature_grads; exec.hip
    mccnn_conv_backward `if (f.unsorted)`, in scratch that requirements() sized for exactly this case). The executor has no
    counter that tells row launches from streaming launches (debug_counters() holds caller_orderings alone); its route
    follows from `rows_bwd = f.rows_bwd && m > 0 && (out_grad & 15) == 0` and `f.unsorted = ... && (feats & 15) == 0`.
    Found by reading while following the out-gradient: combining layers with one input feature read it in 16-byte pieces
    when Fout % 4 == 0 (the centre pass of conv_f1.hip, conv_bwd_mfma<true, 1>), and the streaming / factored forward
    kernels store their output rows as float4 -- by the row width alone. The ops hand the latter fresh allocations, but the
    out-gradient is the caller's: those accesses now look at the pointer as well (test_one_feature_layer_...).
  bf16 rows: the bf16 kernels move 16-byte pieces and have no scalar form; the C ABI answers MCCNN_E_SHAPE for a misaligned
    pointer (tests/test_capi_cpu.py). Both surfaces therefore copy a misaligned bf16 row tensor or out-gradient into an
    allocation of its own where it enters (MCConvModule._bf16_rows_aligned; torch_ext.cpp conv / ConvBackward::apply) and
    compute what the aligned clone computes, bit for bit -- before that the backward pass of such a layer raised
    MCCNN_E_SHAPE, and a tensor 2 bytes off failed in the 32-bit view of its rows.

Offsets: 4 bytes for f32, 8 and 2 bytes for bf16. Nothing here needs a misaligned wide access to be survivable.

Expected values: the CPU oracle on the same inputs (bf16: on the rounded values) at RTOL = 1e-4, norm-wise and per element;
bf16 rows equal to the rounded oracle rows or one bf16 step apart; f32 against the same call on aligned clones at 2e-5 (the
bound tests/test_gpu_parity.py::test_spatial_conv_fwd_bwd holds between two GPU implementations that share every
pre-activation: the vector and scalar forms multiply f * inv * o in another order), bf16 against it bit for bit.

MEASURED on an MI355X (worst max|diff| / max|ref| over the cases of this file): see MEASURED below.
"""
import numpy as np
import pytest

from tests import ref_cases as rc
from tests.combin_cases import off, pooling_cloud   # (shared with tests/test_gpu_combin_lattice.py)
from tests.helpers import make_mlp, conv_nb, run_chain, assert_float_close

pytestmark = pytest.mark.gpu

RTOL = 1e-4
FIN, B, RADIUS, SCALE_INV, AVG = 16, 1, 0.2, False, True
NAMES = ["featGrad", "dw1", "db1", "dw2", "db2", "dw3", "db3"]

MEASURED = """
MI355X, 909 points / 300 centres / 21 946 edges (longest row 157, 6 centres without neighbours, 38 points nobody's
neighbour), 16 features, 21 tests, each under a second after the first (which computes the oracle's values, ~1 s) but
the child process of the ctypes-binding case (a few seconds: a fresh interpreter).
Worst max|diff| / max|ref| over the cases:

    output     op surface, f32             native executor, f32        op, bf16 rows   native, bf16 rows
               vs oracle   vs aligned      vs oracle   vs aligned      vs oracle       vs oracle
    out        3.6e-7      1.8e-7          1.3e-6      0 (same bits)   2.3e-5 (*)      1.5e-6 (*)
    featGrad   1.3e-7      6.3e-8          8.9e-7      9.5e-8          2.0e-6 (*)      1.0e-6 (*)
    dw1        2.0e-7      1.2e-7          1.9e-6      2.0e-7          1.4e-7          1.9e-6
    db1        1.4e-7      9.5e-8          1.6e-6      1.9e-7          1.9e-7          1.3e-6
    dw2        2.6e-7      2.1e-7          1.8e-6      4.2e-7          1.0e-7          1.8e-6
    db2        2.6e-7      2.1e-7          7.5e-7      1.2e-7          9.6e-8          7.3e-7
    dw3        2.2e-7      1.9e-7          1.1e-6      2.2e-7          1.7e-7          1.1e-6
    db3        2.4e-7      2.0e-7          1.7e-6      2.4e-7          1.6e-7          1.7e-6

(*) rows equal to the bf16-rounded oracle rows or one bf16 step apart; the figure is the largest such step over max|ref|.
The native executor evaluates its own (single-precision) KDE, the op surface is handed the oracle's PDFs: hence ~1e-6 there.
bf16, offset against aligned clone: bit for bit on both surfaces, offsets of 8 and of 2 bytes. Before the aligned copy
(helper switched off, same inputs): aligned rows + out-gradient 8 bytes off -> "spatial_conv_grad(bf16) failed: ... (code
-5)"; rows 8 bytes off -> "spatial_conv(bf16) failed: ... (code -5)"; rows 2 bytes off with sortIndex -> torch's
"storage_offset() must be divisible by 2 to view BFloat16 as Float". The suspected MCCNN_E_SHAPE was real.
Oracle against float64 at the odd depth-wise widths: tests/test_oracle_depthwise_cpu.py (worst 2.9e-7, 1 % of the band).
"""

VARIANTS = [("f32", 4), ("bf16", 8), ("bf16", 2)]
WHICH = ["feats", "outgrad", "both"]


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_GEO = {}


def _geometry(oracle):
    """~900 points (a few of them nobody's neighbour), 300 pooling centres taken from the points plus far ones (rows without
    an edge at the start, in the middle and at the end): m != n. The oracle's chain, its convolution and gradients for f32
    and for bf16-rounded inputs -- computed once."""
    if _GEO:
        return _GEO
    pts, bids, centres, cb, rng = pooling_cloud()
    n = len(pts)
    feats = (2 * rng.random((n, FIN)) - 1).astype(np.float32)           # rows of the UNSORTED points
    og = (2 * np.random.default_rng(5).random((len(centres), FIN)) - 1).astype(np.float32)
    w = make_mlp(conv_nb(FIN, FIN, False), 7)
    o = run_chain(oracle, lambda a: a, lambda a: a, pts, bids, feats, B, RADIUS, SCALE_INV, centres=centres,
                  centre_bids=cb, fout=FIN, combin=False)
    deg = np.diff(np.append(o["startIndexs"].reshape(-1), len(o["packedNeighs"])))
    tdeg = np.bincount(o["packedNeighs"][:, 0], minlength=n)
    assert len(centres) == 300 and 800 <= n <= 1000 and (deg == 0).sum() == 6 and (tdeg == 0).sum() >= 24
    assert deg.max() > 64
    _GEO.update(pts=pts, bids=bids, centres=centres, cb=cb, w=w, o=o, deg=deg, tdeg=tdeg, n=n, m=len(centres),
                e=len(o["packedNeighs"]))
    inv = np.argsort(o["indexs"])       # sorted row -> unsorted row
    for dt in ("f32", "bf16"):
        f_, og_ = (feats, og) if dt == "f32" else (rc.bf16_round(feats), rc.bf16_round(og))
        sf = f_[inv]
        args = (o["sortPts"], sf, o["sortBatchs"], o["pdfs"], centres, o["startIndexs"], o["packedNeighs"], o["aabbMin"],
                o["aabbMax"], w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
        ref = oracle.spatial_conv(*args, FIN, False, B, RADIUS, SCALE_INV, AVG)
        rg = list(oracle.spatial_conv_grad(*args, og_, FIN, False, B, RADIUS, SCALE_INV, AVG))
        fg_unsorted = oracle.sort_points_step2_grad(o["indexs"], np.zeros_like(o["sortPts"]), rg[0])[1]
        _GEO[dt] = dict(feats=f_, sorted_feats=sf, og=og_, out=ref, grads=rg, fg_unsorted=fg_unsorted)
    return _GEO


def _np(t):
    return t.detach().float().cpu().numpy()


def _check(G, dt, out, grads, sorted_rows, what, errs):
    """out and the seven gradients (featGrad in sorted or unsorted row order) against the oracle; finite; rows and gradient
    rows nobody contributes to exactly zero."""
    R = G[dt]
    out, fg = _np(out), _np(grads[0])
    fg_ref = R["grads"][0] if sorted_rows else R["fg_unsorted"]
    tdeg = G["tdeg"] if sorted_rows else G["tdeg"][np.asarray(G["o"]["indexs"])]
    assert np.isfinite(out).all() and all(np.isfinite(_np(g)).all() for g in grads), what
    assert np.all(out[G["deg"] == 0] == 0), what + ": a centre without neighbours has a non-zero row"
    assert np.all(fg[tdeg == 0] == 0), what + ": a point that is nobody's neighbour has a non-zero gradient row"
    if dt == "bf16":
        errs["out"] = max(errs.get("out", 0.0), rc._bf16_close(out, R["out"], what + " out"))
        errs["featGrad"] = max(errs.get("featGrad", 0.0), rc._bf16_close(fg, fg_ref, what + " featGrad"))
    else:
        errs["out"] = max(errs.get("out", 0.0), assert_float_close(out, R["out"], RTOL, what + " out"))
        errs["featGrad"] = max(errs.get("featGrad", 0.0), assert_float_close(fg, fg_ref, RTOL, what + " featGrad"))
    for nm, a, b in zip(NAMES[1:], grads[1:], R["grads"][1:]):
        errs[nm] = max(errs.get(nm, 0.0), assert_float_close(_np(a).reshape(-1), np.asarray(b).reshape(-1), RTOL, what + " " + nm))


def _same_as_aligned(dt, got, ref, what, errs):
    """the offset call against the same call on aligned clones: bf16 bit for bit (the same kernels on a copy), f32 at 2e-5"""
    import torch
    for nm, a, b in zip(["out"] + NAMES, got, ref):
        if dt == "bf16":
            assert torch.equal(a, b), what + ": " + nm + " differs from the aligned clone's"
        else:
            e = assert_float_close(_np(a), _np(b), 2e-5, what + " vs aligned: " + nm)
            errs["aligned:" + nm] = max(errs.get("aligned:" + nm, 0.0), e)


def _inputs(G, dt, nbytes, which, values, og_values):
    """(features, out-gradient) tensors: offset where `which` says so, aligned clones elsewhere"""
    import torch
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    f, g = _t(values).to(tdt), _t(og_values).to(tdt)
    f = off(f, nbytes) if which in ("feats", "both") else f.clone()
    g = off(g, nbytes) if which in ("outgrad", "both") else g.clone()
    assert (f.data_ptr() % 16 != 0) == (which in ("feats", "both")) and (g.data_ptr() % 16 != 0) == (which in ("outgrad", "both"))
    return f, g


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("dt,nbytes", VARIANTS, ids=["%s_off%d" % v for v in VARIANTS])
def test_op_surface_rows_off_the_16_byte_grid(mc, oracle, dt, nbytes, which):
    """MCConvModule.spatial_conv: the plain call on sorted rows, and the sortIndex / featIndex call on the rows of the
    unsorted points (a small level: aligned rows are read in place by the row kernels; with an offset out-gradient the
    backward pass must sort them after all)."""
    import torch
    G = _geometry(oracle)
    o, w, n, m, e = G["o"], G["w"], G["n"], G["m"], G["e"]
    P, Bi, C, Cb = _t(G["pts"]), _t(G["bids"]), _t(G["centres"]), _t(G["cb"])
    mn, mx = mc.compute_aabb(P, Bi, B, SCALE_INV)
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, B, RADIUS, SCALE_INV)
    start, packed = mc.find_neighbors(C, Cb, sP, cells, mn, mx, RADIUS, B, SCALE_INV)
    assert np.array_equal(idx.cpu().numpy(), o["indexs"]) and np.array_equal(sP.cpu().numpy(), o["sortPts"])
    assert np.array_equal(start.cpu().numpy(), o["startIndexs"]) and np.array_equal(packed.cpu().numpy(), o["packedNeighs"])
    pdfs = _t(o["pdfs"])
    assert n <= mc.UNSORTED_MAX_POINTS and m != n
    errs = {}

    def call(feats, og, sort_index):
        tw = {k: _t(v).requires_grad_(True) for k, v in w.items()}
        F = feats.requires_grad_(True)
        kw = dict(sortIndex=idx, featIndex=inv) if sort_index else {}
        out = mc.spatial_conv(sP, F, sB, pdfs, C, start, packed, mn, mx, tw["w1"], tw["w2"], tw["w3"], tw["b1"], tw["b2"],
                              tw["b3"], FIN, False, B, RADIUS, SCALE_INV, AVG, **kw)
        grads = torch.autograd.grad([out], [F, tw["w1"], tw["b1"], tw["w2"], tw["b2"], tw["w3"], tw["b3"]], [og])
        torch.cuda.synchronize()
        return [out.detach()] + [g.detach() for g in grads]

    for sort_index in (False, True):
        what = "%s %s +%d B, %s" % (dt, which, nbytes, "sortIndex/featIndex" if sort_index else "sorted rows")
        values = G[dt]["feats"] if sort_index else G[dt]["sorted_feats"]
        f_off, g_off = _inputs(G, dt, nbytes, which, values, G[dt]["og"])
        f_al, g_al = _inputs(G, dt, nbytes, "none", values, G[dt]["og"])
        # the aligned rows take the row kernels; offset f32 rows do not (offset bf16 rows are copied first)
        assert mc._rows_shape(False, FIN, f_al, m, e) and mc._rows_shape(False, FIN, f_al, n, e, backward=True)
        if which != "outgrad":
            assert not mc._rows_shape(False, FIN, f_off, m, e)
        got = call(f_off, g_off, sort_index)
        ref = call(f_al, g_al, sort_index)
        _check(G, dt, got[0], got[1:], not sort_index, what, errs)
        _check(G, dt, ref[0], ref[1:], not sort_index, what + " (aligned clone)", errs)
        _same_as_aligned(dt, got, ref, what, errs)
    print("ALIGNERR op %s %s +%d: %s" % (dt, which, nbytes, " ".join("%s=%.1e" % kv for kv in sorted(errs.items()))))


@pytest.mark.parametrize("impl", [0, 2], ids=["factored", "general_mfma"])
def test_one_feature_layer_with_an_offset_out_gradient(mc, oracle, impl):
    """Combining layers with one input feature read the out-gradient in 16-byte pieces when Fout % 4 == 0: the centre pass
    of the factored kernels (conv_f1.hip) and conv_bwd_mfma<true, 1> (selected by debug_conv_impl(2)). Both look at the
    pointer's low bits as well: an out-gradient 4 bytes off takes their scalar loads. 1 -> 16 on the same geometry, against
    the oracle at RTOL and against the aligned clone at 2e-5."""
    import torch
    G = _geometry(oracle)
    o, n, m = G["o"], G["n"], G["m"]
    fout = 16
    rng = np.random.default_rng(17)
    f1 = (2 * rng.random((n, 1)) - 1).astype(np.float32)                 # rows of the sorted points
    og = (2 * rng.random((m, fout)) - 1).astype(np.float32)
    w = make_mlp(conv_nb(1, fout, True), 9)
    args = (o["sortPts"], f1, o["sortBatchs"], o["pdfs"], G["centres"], o["startIndexs"], o["packedNeighs"], o["aabbMin"],
            o["aabbMax"], w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
    ref = oracle.spatial_conv(*args, fout, True, B, RADIUS, SCALE_INV, AVG)
    rg = oracle.spatial_conv_grad(*args, og, fout, True, B, RADIUS, SCALE_INV, AVG)
    dev = [_t(o[k]) for k in ("sortPts", "sortBatchs", "pdfs", "startIndexs", "packedNeighs", "aabbMin", "aabbMax")]
    sP, sB, pdfs, start, packed, mn, mx = dev
    C = _t(G["centres"])
    res = []
    mc.debug_conv_impl(impl)
    try:
        for g in (off(_t(og), 4), _t(og).clone()):
            tw = {k: _t(v).requires_grad_(True) for k, v in w.items()}
            F = _t(f1).requires_grad_(True)
            out = mc.spatial_conv(sP, F, sB, pdfs, C, start, packed, mn, mx, tw["w1"], tw["w2"], tw["w3"], tw["b1"],
                                  tw["b2"], tw["b3"], fout, True, B, RADIUS, SCALE_INV, AVG)
            grads = torch.autograd.grad([out], [F, tw["w1"], tw["b1"], tw["w2"], tw["b2"], tw["w3"], tw["b3"]], [g])
            torch.cuda.synchronize()
            res.append([out.detach()] + [x.detach() for x in grads])
    finally:
        mc.debug_conv_impl(0)
    for k, label in enumerate(("offset", "aligned")):
        for nm, a, b in zip(["out"] + NAMES, res[k], [ref] + list(rg)):
            assert_float_close(_np(a).reshape(-1), np.asarray(b).reshape(-1), RTOL, "1to16 %s out-gradient: %s" % (label, nm))
    for nm, a, b in zip(["out"] + NAMES, res[0], res[1]):
        assert_float_close(_np(a), _np(b), 2e-5, "1to16 offset vs aligned: " + nm)


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("dt,nbytes", VARIANTS, ids=["%s_off%d" % v for v in VARIANTS])
def test_native_executor_rows_off_the_16_byte_grid(mc, oracle, dt, nbytes, which):
    """ConvolutionBuilder(native=True): two layers over ONE geometry (pooling: the centres are another hierarchy's points),
    the out-gradients handed in through torch.autograd.grad. Offset out-gradient with aligned features: the forward pass
    read the unsorted rows in place, mccnn_conv_backward leaves the row kernels, sorts the rows into its scratch and runs
    the streaming kernels; the second layer's backward pass finds the transposed list the first one built. Offset
    features: the executor takes the sorted copy in both passes (f32), or the extension's aligned copy (bf16)."""
    import torch
    from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
    G = _geometry(oracle)
    w, n, m = G["w"], G["n"], G["m"]
    P, Bi, C, Cb = _t(G["pts"]), _t(G["bids"]), _t(G["centres"]), _t(G["cb"])
    nb = conv_nb(FIN, FIN, False)
    errs = {}

    def run(which_):
        ph_in = PointHierarchy(P, torch.ones((n, 1), device="cuda"), Bi, [], "IN", B, SCALE_INV)
        ph_out = PointHierarchy(C, torch.ones((m, 1), device="cuda"), Cb, [], "OUT", B, SCALE_INV)
        cb = ConvolutionBuilder(KDEWindow=0.2, relativeRadius=SCALE_INV, native=True)
        sd = {}
        for name in ("A", "B"):
            sd.update({name + "_weights": _t(w["w1"]).reshape(3, 8 * nb), name + "_biases": _t(w["b1"]),
                       name + "_weights2": _t(w["w2"]).reshape(nb, 8, 8), name + "_biases2": _t(w["b2"]).reshape(nb, 8),
                       name + "_weights3": _t(w["w3"]).reshape(nb, 8, 8), name + "_biases3": _t(w["b3"]).reshape(nb, 8)})
        cb.load_state_dict(sd)
        cb.reset()
        outs, fts, ogs = [], [], []
        for name in ("A", "B"):
            f, g = _inputs(G, dt, nbytes, which_, G[dt]["feats"], G[dt]["og"])
            f.requires_grad_(True)
            outs.append(cb.create_convolution(name, ph_in, 0, f, FIN, RADIUS, ph_out, 0, False, FIN))
            fts.append(f)
            ogs.append(g)
        assert len(cb.cacheGeo_) == 1, "the two layers did not share one native geometry"
        geo = next(iter(cb.cacheGeo_.values()))
        named = dict(cb.named_parameters())
        params = [named[name + s] for name in ("A", "B") for s in ("_weights", "_biases", "_weights2", "_biases2", "_weights3", "_biases3")]
        grads = torch.autograd.grad(outs, fts + params, ogs)
        torch.cuda.synchronize()
        assert geo.e == G["e"]
        res = []
        for k in range(2):
            res.append([outs[k].detach(), grads[k].detach()] + [g.detach() for g in grads[2 + 6 * k:8 + 6 * k]])
        return res

    got, ref = run(which), run("none")
    for k, name in enumerate(("A", "B")):
        what = "native %s %s +%d B, layer %s" % (dt, which, nbytes, name)
        _check(G, dt, got[k][0], got[k][1:], False, what, errs)
        _check(G, dt, ref[k][0], ref[k][1:], False, what + " (aligned clone)", errs)
        _same_as_aligned(dt, got[k], ref[k], what, errs)
    print("ALIGNERR native %s %s +%d: %s" % (dt, which, nbytes, " ".join("%s=%.1e" % kv for kv in sorted(errs.items()))))


def test_native_executor_ctypes_binding_bf16_rows_off_the_16_byte_grid():
    """The same through the ctypes binding of the executor (MCCNN_TORCH_EXT=0: mccnn_amd.native._Conv makes the aligned
    copies itself): the bf16 case with rows AND out-gradient 2 bytes off, in a child process -- the binding is chosen when
    the package is imported."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MCCNN_TORCH_EXT="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_conv_alignment.py"), "-m", "gpu",
                          "-x", "-q", "-p", "no:cacheprovider", "-k",
                          "test_native_executor_rows_off_the_16_byte_grid and bf16_off2 and both"], env=env,
                         capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
