"""Depth-wise (combin=False) layers of the widths the vector kernels do not take -- 1, 3, 4, 5, 12, 20, 28, 524 features --
on the oracle's side: oracle.spatial_conv / spatial_conv_grad against float64 torch autograd of the definition
(tests/pointgrad_ref.py::spatial_conv), output and all seven gradients at the project bar RTOL = 1e-4 (norm-wise and per
element, tests/helpers.py::assert_float_close). The GPU tests of these widths (tests/test_gpu_parity.py::CONV_CASES "dw*",
tests/test_gpu_conv_alignment.py) compare the HIP kernels with the oracle; this pins what they compare against.

MEASURED (oracle against float64, worst over the eight cases of max|diff| / max|ref| and of elementwise_excess, <= 1 passes):
    out 2.9e-07 / 0.010   featGrad 2.2e-07 / 0.010   dw1 1.6e-07 / 0.008   db1 1.6e-07 / 0.004
    dw2 2.0e-07 / 0.008   db2 1.0e-07 / 0.005        dw3 1.7e-07 / 0.006   db3 1.7e-07 / 0.004
so the reference side holds the bar with two orders of magnitude to spare at every one of these widths. The clouds are small
(597 points / 13 231 or 12 077 edges; 189 points / 2 649 edges for 524 features; the longest row has 45 edges): the eight
cases together take about four seconds.
"""
import numpy as np
import pytest
import torch

from tests import pointgrad_ref as ref
from tests.helpers import make_cloud, make_mlp, conv_nb, run_chain, assert_float_close, elementwise_excess

RTOL = 1e-4
ident = lambda a: a

CASES = [
    # Fin, avg, scaleInv, radius
    (1, True, True, 0.15),
    (3, True, True, 0.15),
    (4, True, True, 0.15),
    (5, False, False, 0.12),
    (12, True, True, 0.15),
    (20, False, False, 0.12),
    (28, True, True, 0.15),
    (524, True, True, 0.3),
]
SIZES = {(597, 0.15): (597, 13231), (597, 0.12): (597, 12077), (189, 0.3): (189, 2649)}   # (points, radius) -> (points, edges)
NAMES = ["out", "featGrad", "dw1", "db1", "dw2", "db2", "dw3", "db3"]


@pytest.mark.parametrize("fin,avg,scaleInv,radius", CASES, ids=["dw%d" % c[0] for c in CASES])
def test_depthwise_oracle_against_float64_autograd(oracle, fin, avg, scaleInv, radius):
    B = 2
    pts, bids = make_cloud(150 if fin > 256 else 400, B, 21, "clustered", True)
    feats = (2 * np.random.default_rng(7).random((len(pts), fin)) - 1).astype(np.float32)
    o = run_chain(oracle, ident, ident, pts, bids, feats, B, radius, scaleInv, fout=fin, combin=False)
    w = make_mlp(conv_nb(fin, fin, False), 7)
    for k in w:
        assert np.array_equal(w[k], o["mlp"][k])
    og = (2 * np.random.default_rng(11).random((len(pts), fin)) - 1).astype(np.float32)
    args = (o["sortPts"], o["sortFeatures"], o["sortBatchs"], o["pdfs"], pts, o["startIndexs"], o["packedNeighs"],
            o["aabbMin"], o["aabbMax"], w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
    out = oracle.spatial_conv(*args, fin, False, B, radius, scaleInv, avg)
    grads = oracle.spatial_conv_grad(*args, og, fin, False, B, radius, scaleInv, avg)
    print("dw%d: %d points, %d edges" % (fin, len(pts), len(o["packedNeighs"])))
    assert (len(pts), len(o["packedNeighs"])) == SIZES[(len(pts), radius)]    # the inputs are the ones the figures belong to
    # float64 autograd of the definition on the same integer structure
    T = ref.t64
    f64 = T(o["sortFeatures"]).requires_grad_(True)
    tw = {k: T(v).requires_grad_(True) for k, v in w.items()}
    out64 = ref.spatial_conv(T(o["sortPts"]), f64, o["sortBatchs"], T(o["pdfs"]), T(pts), o["startIndexs"],
                             o["packedNeighs"], T(o["aabbMin"]), T(o["aabbMax"]), tw["w1"], tw["b1"], tw["w2"], tw["b2"],
                             tw["w3"], tw["b3"], fin, False, B, radius, scaleInv, avg)
    g64 = torch.autograd.grad(out64, [f64, tw["w1"], tw["b1"], tw["w2"], tw["b2"], tw["w3"], tw["b3"]],
                              grad_outputs=T(og))
    got = [out] + list(grads)
    want = [out64.detach().numpy()] + [g.numpy() for g in g64]
    assert len(got) == len(NAMES)
    for nm, a, b in zip(NAMES, got, want):
        a = np.asarray(a)
        if nm != "out" and nm != "featGrad":
            a, b = a.reshape(-1), b.reshape(-1)    # the six MLP tensors: flat layouts, w1[nu*3+d], w2/w3[q*64+o*8+k]
        err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
        print("dw%d %-8s max|diff|/max|ref| = %.2e   elementwise_excess = %.3f" % (fin, nm, err, elementwise_excess(a, b, RTOL)))
        assert_float_close(a, b, RTOL, "dw%d %s" % (fin, nm))
