"""Combining layers (combin=True) of every (Fin, Fout) of the lattice in tests/combin_cases.py on the oracle's side:
oracle.spatial_conv / spatial_conv_grad against float64 torch autograd of the definition (tests/pointgrad_ref.py::spatial_conv),
output and all seven gradients at the project bar RTOL = 1e-4 (norm-wise and per element, tests/helpers.py::assert_float_close).
tests/test_gpu_combin_lattice.py compares the HIP kernels with the oracle at these shapes; this pins what it compares against.

Inputs: the narrow shapes (nb <= 9) on 425 points / 7 055 edges (make_cloud(400, 2, 22, "clustered", True), radius 0.15), the
wide ones (nb = 50, 51, 64, 65) on 159 points / 1 887 edges (make_cloud(150, 2, 22, ...), radius 0.3). The 37 cases together
take about six seconds.

One input is NOT usable, and the reason is the reference, not either implementation: make_cloud(150, 2, 21, "clustered", True)
at radius 0.3 (189 points, 2 649 edges) with make_mlp(50, 7) has a layer-2 pre-activation at |pre2| / S2 = 4.0e-10
(pointgrad_ref.conv_preacts). The oracle's float32 chain and the float64 definition land on different sides of that ReLU, and
dw1, db1, dw2, db2 of EVERY layer with nb = 50 (4 -> 100, 2 -> 200, 5 -> 80, 1 -> 400: the pre-activations depend on the
geometry and on nb alone) come out about 1e-2 apart; out, dw3, db3 stay clean. That is the discontinuity of ReLU' showing
in the reference. The GPU kernels replay the oracle's fmaf chains bit for bit, so the GPU tests are not affected by it. Hence
seed 22 for the wide cloud, and hence the condition below ON THE INPUTS: the smallest |pre| / S over both ReLU layers and all
edges is printed and asserted to be >= 1e-7 (about two float32 roundings of the chain's largest term), so that a later change of
seed or weights cannot bring the flip back unseen. No element is excluded from any comparison. The same condition chose the
narrow cloud: the seed-21 cloud of that size (597 points, 13 231 edges) has 4.7e-8 with make_mlp(2, 7) -- no gradient was off
there, but the input does not hold the condition, so it is not used.

MEASURED (oracle against float64; worst over the 37 cases of max|diff| / max|ref| and of elementwise_excess, <= 1 passes):
    out 1.7e-06 / 0.022   featGrad 2.7e-06 / 0.059   dw1 2.2e-07 / 0.009   db1 1.4e-07 / 0.010
    dw2 2.6e-07 / 0.014   db2 1.7e-07 / 0.010        dw3 2.4e-07 / 0.008   db3 7.9e-08 / 0.005
so the reference side holds the bar with more than an order of magnitude to spare at every shape of the lattice.
Smallest |pre| / S per input (geometry, nb): narrow cloud 6.2e-6 (1), 3.4e-6 (2), 1.0e-6 (3), 9.4e-7 (4), 1.0e-6 (5), 5.1e-7 (6),
2.1e-7 (7), 1.1e-6 (9);
wide cloud 2.5e-7 (50), 8.2e-7 (51), 7.4e-7 (64), 2.0e-7 (65).
"""
import numpy as np
import pytest
import torch

from tests import combin_cases as cc
from tests import pointgrad_ref as ref
from tests.helpers import make_mlp, conv_nb, run_chain, assert_float_close, elementwise_excess

RTOL = 1e-4
MIN_PRE = 1e-7
ident = lambda a: a
SIZES = {"A": (425, 7055), "W": (159, 1887)}     # geometry of the case table -> (points, edges) the figures belong to
NAMES = ["out", "featGrad", "dw1", "db1", "dw2", "db2", "dw3", "db3"]

_CHAIN, _PRE = {}, {}


def _chain(oracle, which):
    """the oracle's chain on the small cloud of geometry `which` (the features do not enter the integer structure or the PDFs)"""
    if which not in _CHAIN:
        pts, bids, B, radius, scaleInv = cc.cloud_S() if which == "A" else cc.cloud_W()
        o = run_chain(oracle, ident, ident, pts, bids, np.zeros((len(pts), 1), np.float32), B, radius, scaleInv, fout=1)
        assert (len(pts), len(o["packedNeighs"])) == SIZES[which]    # the inputs are the ones the figures belong to
        _CHAIN[which] = (pts, bids, B, radius, scaleInv, o)
    return _CHAIN[which]


def _min_preact(which, pts, radius, scaleInv, o, nb):
    """smallest |pre| / S over the two ReLU layers, all edges and all neurons of make_mlp(nb, 7) on this geometry"""
    if (which, nb) not in _PRE:
        w = make_mlp(nb, 7)
        lo = np.inf
        e = len(o["packedNeighs"])
        for a in range(0, e, 8192):
            pre1, S1, pre2, S2 = ref.conv_preacts(o["sortPts"], pts, o["sortBatchs"], o["packedNeighs"], o["aabbMin"],
                                                  o["aabbMax"], w, radius, scaleInv, np.arange(a, min(a + 8192, e)))
            lo = min(lo, float((pre1.abs() / S1).min()), float((pre2.abs() / S2).min()))
        _PRE[(which, nb)] = lo
    return _PRE[(which, nb)]


def test_case_table_states_what_the_shapes_are():
    cc.check_table()
    assert len(cc.LATTICE) == 37 and len(set(c[:2] for c in cc.LATTICE)) == 37


def test_c_abi_refuses_the_shapes_the_rule_excludes():
    """spatial_conv.cc:290 as the library keeps it (conv.hip fill_args): a combining layer whose padded neuron count 8 * nb is no
    multiple of Fin is answered with MCCNN_E_SHAPE by both entry points -- before anything is launched or read, which is why
    made-up addresses and no GPU do here. Nine shapes of the lattice are such shapes (tests/combin_cases.py says which routes
    that leaves without a caller); the accepted ones run in tests/test_gpu_combin_lattice.py."""
    from mccnn_amd import _lib
    lib = _lib.load()
    E_SHAPE = -5
    A = 0x7f0000000000          # a made-up, 16-byte aligned address: never dereferenced by the calls below
    p = [A + 0x100000 * k for k in range(32)]
    n = m = 64
    e = 256
    refused = [c for c in cc.LATTICE if not cc.accepted(c)]
    assert len(refused) == 9
    for fin, fout, *_ in refused:
        assert lib.mccnn_spatial_conv_fwd(*p[0:15], n, m, e, fin, fout, 1, 1, 0.1, 0, 1, p[15], None, p[16], 1 << 20, None) == E_SHAPE
        assert lib.mccnn_spatial_conv_bwd(*p[0:15], p[17], n, m, e, fin, fout, 1, 1, 0.1, 0, 1, None, None, None, p[18],
                                          *p[19:25], p[16], 1 << 20, None) == E_SHAPE


def test_the_seed_21_wide_cloud_sits_on_a_relu_gate(oracle):
    """The input this file does NOT use (docstring): its smallest |pre| / S is far under the bar the used inputs must hold."""
    from tests.helpers import make_cloud
    pts, bids = make_cloud(150, 2, 21, "clustered", True)
    o = run_chain(oracle, ident, ident, pts, bids, np.zeros((len(pts), 1), np.float32), 2, 0.3, True, fout=1)
    assert (len(pts), len(o["packedNeighs"])) == (189, 2649)
    lo = _min_preact("seed21", pts, 0.3, True, o, 50)
    print("seed 21, nb = 50: min |pre| / S = %.2e" % lo)
    assert lo < 1e-8


@pytest.mark.parametrize("case", cc.LATTICE, ids=[cc.case_id(c) for c in cc.LATTICE])
def test_combin_oracle_against_float64_autograd(oracle, case):
    fin, fout, nb, _last, _r0, _why, which = case
    pts, bids, B, radius, scaleInv, o = _chain(oracle, which)
    avg = True
    n = len(pts)
    assert conv_nb(fin, fout, True) == nb
    w = make_mlp(nb, 7)
    lo = _min_preact(which, pts, radius, scaleInv, o, nb)
    print("%s: %d points, %d edges, nb = %d, min |pre| / S = %.2e" % (cc.case_id(case), n, len(o["packedNeighs"]), nb, lo))
    assert lo >= MIN_PRE, "an input on a ReLU gate: choose another seed (see the docstring), do not mask elements"
    feats, og = cc.layer_inputs(n, n, fin, fout)
    args = (o["sortPts"], feats, o["sortBatchs"], o["pdfs"], pts, o["startIndexs"], o["packedNeighs"], o["aabbMin"],
            o["aabbMax"], w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
    out = oracle.spatial_conv(*args, fout, True, B, radius, scaleInv, avg)
    grads = oracle.spatial_conv_grad(*args, og, fout, True, B, radius, scaleInv, avg)
    # float64 autograd of the definition on the same integer structure
    T = ref.t64
    f64 = T(feats).requires_grad_(True)
    tw = {k: T(v).requires_grad_(True) for k, v in w.items()}
    out64 = ref.spatial_conv(T(o["sortPts"]), f64, o["sortBatchs"], T(o["pdfs"]), T(pts), o["startIndexs"],
                             o["packedNeighs"], T(o["aabbMin"]), T(o["aabbMax"]), tw["w1"], tw["b1"], tw["w2"], tw["b2"],
                             tw["w3"], tw["b3"], fout, True, B, radius, scaleInv, avg)
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
        print("%s %-8s max|diff|/max|ref| = %.2e   elementwise_excess = %.3f" % (cc.case_id(case), nm, err, elementwise_excess(a, b, RTOL)))
        assert_float_close(a, b, RTOL, "%s %s" % (cc.case_id(case), nm))
    # the padded neurons of the last block take no part: exactly zero on both sides
    neurons = fin * fout
    assert np.all(np.asarray(grads[5]).reshape(-1)[neurons * 8:] == 0) and np.all(np.asarray(grads[6]).reshape(-1)[neurons:] == 0)
